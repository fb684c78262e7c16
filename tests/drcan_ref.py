"""An fp64-capable CPU restatement of RCAN, DRCAN's generator (SRADSGAN/model/drcan.py:35-226), in plain torch ops with the
reference's state_dict keys, for tests that compare the HIP model against it in double precision.  Written from the model's
equations: head conv; G residual groups, each n blocks of [conv, ReLU, conv, channel attention with biased 1x1 convs, + block input]
then a conv and + group input; a body conv and + head output; one conv + pixel shuffle per upsampling stage (untied); a last conv."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv(cin, cout, k=3, bias=True):
    return nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias)


class _Shuffle(nn.Module):
    def __init__(self, r):
        super().__init__()
        self.r = r

    def forward(self, x):
        return F.pixel_shuffle(x, self.r)


def upsampler(scale, n=64):
    if scale & (scale - 1) == 0:
        r, stages = 2, int(math.log(scale, 2))
    elif scale % 3 == 0:
        r, stages = 3, int(math.log(scale, 3))
    else:
        raise NotImplementedError
    mods = []
    for _ in range(stages):
        mods += [_conv(n, r * r * n), _Shuffle(r)]
    return nn.Sequential(*mods)


class Attention(nn.Module):
    """s = sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2); returns x * s.  Keys conv_du.0 / conv_du.2."""

    def __init__(self, c=64, reduction=16):
        super().__init__()
        self.conv_du = nn.Sequential(nn.Conv2d(c, c // reduction, 1), nn.ReLU(), nn.Conv2d(c // reduction, c, 1), nn.Sigmoid())

    def forward(self, x):
        return x * self.conv_du(x.mean(dim=(2, 3), keepdim=True))


class Block(nn.Module):
    def __init__(self, c=64, reduction=16):
        super().__init__()
        self.body = nn.Sequential(_conv(c, c), nn.ReLU(), _conv(c, c), Attention(c, reduction))

    def forward(self, x):
        return x + self.body(x)


class Group(nn.Module):
    def __init__(self, blocks, c=64, reduction=16):
        super().__init__()
        self.body = nn.Sequential(*[Block(c, reduction) for _ in range(blocks)], _conv(c, c))

    def forward(self, x):
        return x + self.body(x)


class Generator(nn.Module):
    def __init__(self, scale, groups=2, blocks=2, reduction=16, c=64):
        super().__init__()
        self.head = nn.Sequential(_conv(3, c))
        self.body = nn.Sequential(*[Group(blocks, c, reduction) for _ in range(groups)], _conv(c, c))
        self.tail = nn.Sequential(upsampler(scale, c), _conv(c, 3))

    def forward(self, x):
        h = self.head(x)
        return self.tail(h + self.body(h))


def loss(y, t, kind='L1'):
    return F.l1_loss(y, t) if kind == 'L1' else F.mse_loss(y, t)
