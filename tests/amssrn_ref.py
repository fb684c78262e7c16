"""An fp64-capable CPU restatement of AMSSRN's generator (SRADSGAN/model/amssrn.py:74-334) in plain torch ops, with the reference's
state_dict keys, for tests that compare the HIP model against it in double precision.  Written from the reference's equations:
quadrant non-local attention at H // 2, W // 2, channel attention with biases and PReLU, RB = x + conv(x) + conv(prelu(conv(x))),
ASPP with dilations 1-3 and one shared PReLU, FPN fusion over 11 maps, `x + gamma * non_local_1` after every block."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv(cin, cout, k, bias=True):
    return nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias)


class Tail(nn.Sequential):
    def __init__(self, scale, n=64):
        mods = []
        if scale & (scale - 1) == 0:
            for _ in range(int(math.log(scale, 2))):
                mods += [_conv(n, 4 * n, 3), nn.PixelShuffle(2)]
        else:
            pair = [_conv(n, 9 * n, 3), nn.PixelShuffle(3)]
            for _ in range(int(math.log(scale, 3))):
                mods += pair                                  # one module pair, listed per stage (tied)
        super().__init__(*mods)


class NonLocal(nn.Module):
    def __init__(self, c=64, ci=8):
        super().__init__()
        self.g, self.W = nn.Conv2d(c, ci, 1), nn.Conv2d(ci, c, 1)
        self.theta, self.phi = nn.Conv2d(c, ci, 1), nn.Conv2d(c, ci, 1)

    def block(self, x):
        n, c, h, w = x.shape
        t = self.theta(x).flatten(2).transpose(1, 2)          # [n, hw, ci]
        p = self.phi(x).flatten(2)                            # [n, ci, hw]
        v = self.g(x).flatten(2).transpose(1, 2)
        y = torch.softmax(t @ p, dim=-1) @ v
        return self.W(y.transpose(1, 2).reshape(n, -1, h, w)) + x

    def forward(self, x):
        h1, w1 = x.shape[2] // 2, x.shape[3] // 2
        top = torch.cat([self.block(x[:, :, :h1, :w1]), self.block(x[:, :, :h1, w1:])], 3)
        bottom = torch.cat([self.block(x[:, :, h1:, :w1]), self.block(x[:, :, h1:, w1:])], 3)
        return torch.cat([top, bottom], 2)


class NonLocalCA(nn.Module):
    def __init__(self):
        super().__init__()
        self.non_local = NonLocal()

    def forward(self, x):
        return self.non_local(x)


class CA(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv_du = nn.Sequential(nn.Conv2d(c, c // 16, 1), nn.PReLU(), nn.Conv2d(c // 16, c, 1), nn.Sigmoid())

    def forward(self, x):
        return x * self.conv_du(x.mean(dim=(2, 3), keepdim=True))


class RB(nn.Module):
    def __init__(self, n=64):
        super().__init__()
        self.conv3X3 = nn.Conv2d(n, n, 3, padding=1)
        self.rb = nn.Sequential(nn.Conv2d(n, n, 3, padding=1), nn.PReLU(), nn.Conv2d(n, n, 3, padding=1))

    def forward(self, x):
        return x + self.conv3X3(x) + self.rb(x)


class ASPP(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.d1, self.d2, self.d3 = (nn.Conv2d(n, n, 3, padding=d, dilation=d) for d in (1, 2, 3))
        self.act = nn.PReLU()

    def forward(self, x):
        return torch.cat([self.act(self.d1(x)), self.act(self.d2(x)), self.act(self.d3(x))], 1)


class Block(nn.Module):
    def __init__(self, aspp, n=64):
        super().__init__()
        self.c1, self.c2, self.c3, self.c4 = RB(n), RB(n), RB(n), RB(n)
        if aspp:
            self.aspp = ASPP(4 * n)
        self.ca = CA(12 * n if aspp else 5 * n)
        self.c5 = nn.Conv2d(12 * n if aspp else 5 * n, n, 1)
        self.has_aspp = aspp

    def forward(self, x):
        o = [x]
        for m in (self.c1, self.c2, self.c3, self.c4):
            o.append(m(o[-1]))
        cat = self.aspp(torch.cat(o[1:], 1)) if self.has_aspp else torch.cat(o, 1)
        return self.c5(self.ca(cat)) + x


class FPN(nn.Module):
    def __init__(self, k, n=64):
        super().__init__()
        self.fusion = nn.Sequential(*[nn.Conv2d(n, n, 3, padding=1) for _ in range(k)])

    def forward(self, f):
        return [self.fusion[0](f[-1])] + [self.fusion[i + 1](f[-(i + 2)] + f[-(i + 1)]) for i in range(len(f) - 1)]


class Generator(nn.Module):
    def __init__(self, scale=4, n=64):
        super().__init__()
        self.fpn_fusion = FPN(11)
        self.feature_bank = nn.Conv2d(11 * n, n, 1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.non_local_1, self.non_local_2 = NonLocalCA(), NonLocalCA()
        self.head = nn.Sequential(_conv(3, n, 3))
        self.body = nn.Sequential(*[Block(False) for _ in range(4)], *[Block(True) for _ in range(4)])
        self.tail = Tail(scale)
        self.reconstruction = nn.Conv2d(n, 3, 3, padding=1)

    def forward(self, x):
        head = self.head(x)
        nl1 = self.non_local_1(head)
        feats, x = [head, nl1], nl1
        for b in self.body:
            x = b(x) + self.gamma * nl1
            feats.append(x)
        feats.append(self.non_local_2(x))
        bank = self.feature_bank(torch.cat(self.fpn_fusion(feats), 1))
        return self.reconstruction(self.tail(head + bank))


def loss(gen, hr, norm='L1'):
    return F.l1_loss(gen, hr) if norm == 'L1' else F.mse_loss(gen, hr)
