"""CPU restatement of the DSSR generator (stock torch ops, any dtype: the fp64 referee of the DSSR tests).

Written from the architecture: head conv 3 -> 64; G residual groups, each n WABs (conv 3x3 64 -> 256 + bias, ReLU, conv 3x3 256 -> 64
+ bias, average-pool channel attention with a bias-free 64 -> 4 -> 64 MLP and a sigmoid gate, + block input) followed by a conv 3x3
64 -> 64 + bias and the group skip; the upsampler (per stage conv 64 -> 64 r^2 + pixel shuffle, one weight set shared by all stages,
no activation) applied LITERALLY to the head output and to every group output, the G + 1 results summed; output conv 64 -> 3.
Parameter names follow the HIP model's state_dict, so state_dicts load both ways."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv(cin, cout, k=3, bias=True):
    return nn.Conv2d(cin, cout, k, 1, k // 2, bias=bias)


class Attention(nn.Module):
    def __init__(self, c=64, ratio=16):
        super().__init__()
        self.fc1 = _conv(c, c // ratio, 1, bias=False)
        self.fc2 = _conv(c // ratio, c, 1, bias=False)

    def forward(self, u):
        m = u.mean(dim=(2, 3), keepdim=True)
        return torch.sigmoid(self.fc2(F.relu(self.fc1(m)))) * u


class Block(nn.Module):
    def __init__(self, c=64):
        super().__init__()
        self.conv1 = _conv(c, 4 * c)
        self.conv2 = _conv(4 * c, c)
        self.ca = Attention(c)

    def forward(self, x):
        return self.ca(self.conv2(F.relu(self.conv1(x)))) + x


class Group(nn.Module):
    def __init__(self, blocks, c=64):
        super().__init__()
        self.conv = _conv(c, c)
        self.RG = nn.Sequential(*[Block(c) for _ in range(blocks)])

    def forward(self, x):
        return self.conv(self.RG(x)) + x


class Upsampler(nn.Module):
    def __init__(self, scale):
        super().__init__()
        if scale & (scale - 1) == 0:
            self.r, stages = 2, int(round(math.log2(scale)))
        elif scale % 3 == 0:
            self.r, stages = 3, int(round(math.log(scale, 3)))
        else:
            self.r, stages = 1, 0
        conv = _conv(64, 64 * self.r * self.r)
        self.upsampling = nn.Sequential(*([conv, nn.PixelShuffle(self.r)] * stages))

    def forward(self, x):
        return self.upsampling(x)


class Generator(nn.Module):
    def __init__(self, groups=3, blocks=10, scale=4):
        super().__init__()
        self.conv1 = nn.Sequential(_conv(3, 64))
        self.res_groups = nn.Sequential(*[Group(blocks) for _ in range(groups)])
        self.UP = Upsampler(scale)
        self.conv3 = nn.Sequential(_conv(64, 3))

    def forward(self, x):
        h = self.conv1(x)
        acc = self.UP(h)
        for g in self.res_groups:
            h = g(h)
            acc = acc + self.UP(h)
        return self.conv3(acc)


def unique_params(net):
    seen, out = set(), []
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append((k, p))
    return out


def step_digest(t):
    """the digest of post-step weights stored by tools/make_golden_dssr.py"""
    from oracle import sradsgan_ref as O
    return O.digest(t, full_max=512, nsample=256)
