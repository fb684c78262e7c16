"""CPU restatement of NDSRGAN (stock torch ops, any dtype: the fp64 referee of the NDSRGAN tests).

Written from the architecture: head conv 3 -> 64; 23 DCRDBs, each three dense blocks (four conv 3x3 + LeakyReLU(.2) layers growing
64 -> 96 -> 128 -> 160 -> 192 channels by concatenation, then conv 3x3 192 -> 64, result x + .2 conv) on the running sums
t_i = t_(i-1) + .2 o_i, then conv 3x3 64 -> 64, block result .2 conv + x; the trunk is the running sum S_k = S_(k-1) + .2 m_k; conv
3x3 64 -> 64 and the skip from the head; per upsampling stage nearest x r, conv 3x3 64 -> 64, LeakyReLU(.2), one conv shared by
all stages; conv 3x3 64 -> 64, LeakyReLU(.2), conv 3x3 64 -> 3.  Discriminator: 4x4 convs 3 -> 64 s2, 64 -> 128 s2 + BN,
128 -> 256 s2 + BN, 256 -> 512 s1 + BN (each + LeakyReLU .2), 512 -> 1 s1.  Parameter names follow the HIP model's state_dict."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

SLOPE = 0.2


def _conv(cin, cout, k=3, stride=1, pad=1):
    return nn.Conv2d(cin, cout, k, stride, pad)


class Dense(nn.Module):
    def __init__(self, nf=64, nc=32):
        super().__init__()
        self.CL_blocks = nn.Sequential(*[nn.Sequential(_conv(nf + nc * j, nc), nn.LeakyReLU(SLOPE)) for j in range(4)])
        self.conv = _conv(nf + 4 * nc, nf)

    def forward(self, x):
        r = x
        for cl in self.CL_blocks:
            x = torch.cat((x, cl(x)), dim=1)
        return r + self.conv(x) * 0.2


class Dcrdb(nn.Module):
    def __init__(self):
        super().__init__()
        self.RDB1, self.RDB2, self.RDB3 = Dense(), Dense(), Dense()
        self.conv = _conv(64, 64)

    def forward(self, x):
        t = x + 0.2 * self.RDB1(x)
        t = t + 0.2 * self.RDB2(t)
        t = t + 0.2 * self.RDB3(t)
        return self.conv(t) * 0.2 + x


class Trunk(nn.Module):
    def __init__(self, blocks=23):
        super().__init__()
        self.blocks = blocks
        for k in range(1, blocks + 1):
            setattr(self, 'DRRDB%d' % k, Dcrdb())

    def forward(self, x):
        s = x
        for k in range(1, self.blocks + 1):
            s = s + 0.2 * getattr(self, 'DRRDB%d' % k)(s)
        return s


class Generator(nn.Module):
    def __init__(self, scale=4):
        super().__init__()
        self.conv1 = nn.Sequential(_conv(3, 64))
        self.DCRDB_block = Trunk()
        self.conv2 = _conv(64, 64)
        if scale & (scale - 1) == 0:
            r, stages = 2, int(round(math.log2(scale)))
        elif scale % 3 == 0:
            r, stages = 3, int(round(math.log(scale, 3)))
        else:
            r, stages = 1, 0
        stage = [nn.Upsample(scale_factor=r, mode='nearest'), _conv(64, 64), nn.LeakyReLU(SLOPE)]
        self.upsampling = nn.Sequential(*(stage * stages))
        self.conv3 = nn.Sequential(_conv(64, 64), nn.LeakyReLU(SLOPE), _conv(64, 3))

    def forward(self, x):
        out = self.conv1(x)
        out = out + self.conv2(self.DCRDB_block(out))
        return self.conv3(self.upsampling(out))


class Discriminator(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for cout, stride, norm in [(64, 2, False), (128, 2, True), (256, 2, True), (512, 1, True)]:
            layers.append(_conv(cin, cout, 4, stride, 1))
            if norm:
                layers.append(nn.BatchNorm2d(cout))
            layers.append(nn.LeakyReLU(SLOPE))
            cin = cout
        layers.append(_conv(cin, 1, 4, 1, 1))
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


def unique_params(net):
    seen, out = set(), []
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append((k, p))
    return out


def step_digest(t):
    """the digest of post-step weights stored by tools/make_golden_ndsrgan.py"""
    from oracle import sradsgan_ref as O
    return O.digest(t, full_max=16, nsample=8)


def grad_digest(t):
    """the digest of parameter gradients stored by tools/make_golden_ndsrgan.py"""
    from oracle import sradsgan_ref as O
    return O.digest(t, full_max=16, nsample=8)


def out_digest(t):
    """the digest of the generator output stored by tools/make_golden_ndsrgan.py"""
    from oracle import sradsgan_ref as O
    return O.digest(t, full_max=4096, nsample=4096)


def train_iteration(G, D, Fx, opt_G, opt_D, lr, hr):
    """ndsrgan.py:414-456 with nn.SmoothL1Loss; returns (loss_G, loss_D) as floats."""
    sl1 = F.smooth_l1_loss
    opt_G.zero_grad()
    gen = G(lr)
    v = D(gen)
    loss_gan = sl1(v, torch.ones_like(v))
    real = Fx(hr).detach()
    content = sl1(Fx(gen), real)
    loss_G = 1e-2 * sl1(gen, hr) + content + 2.5e-3 * loss_gan
    loss_G.backward()
    opt_G.step()
    opt_D.zero_grad()
    vr = D(hr)
    loss_real = sl1(vr, torch.ones_like(vr))
    vf = D(gen.detach())
    loss_fake = sl1(vf, torch.zeros_like(vf))
    loss_D = (loss_real + loss_fake) / 2
    loss_D.backward()
    opt_D.step()
    return float(loss_G), float(loss_D)
