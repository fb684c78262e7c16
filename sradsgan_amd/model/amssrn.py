"""AMSSRN generator on the HIP kernels.  Mirrors SRADSGAN/model/amssrn.py:74-334 (Upsampler, _NonLocalBlockND, Nonlocal_CA, CALayer,
RB, ASPP, DB, DB_ASPP, FPN_Fusion, GeneratorResNet) with the reference's constructor signatures and state_dict keys (weight-tied
`tail.{0,2}` stages at x9), and one generator iteration of its training loop (:510-532) as `train_step`.

Execution, exact in real arithmetic:
  * RB's `x + conv3X3(x) + rb(x)`: both adds ride in conv epilogues (conv3X3 + x, then rb[2] + that), in the reference's order;
  * ASPP's three convs are the dilated path (ops.conv2d_dil), their shared PReLU the device-slope pass (ops.prelu);
  * Nonlocal_CA: theta / phi / g are 1x1 convs over the whole map, the attention runs per quadrant in one kernel
    (ops.nonlocal_quadrants), and W (1x1) + bias + the `+ x` residual is one conv over the whole map (W is 1x1, so applying it to the
    assembled quadrants equals applying it per quadrant);
  * `x + gamma * non_local_1` is one pass with gamma on the device (ops.gamma_residual);
  * the concatenations are srhip_cat_channels passes, the FPN sums srhip_sum_n passes, c5 / feature_bank take their residual
    (`+ input`, `head +`) in the conv epilogue."""
import math

import torch
import torch.nn as nn

from .. import ops
from .dssr import _Shuffle
from .layers import HipConv2d, HipDilatedConv2d, HipPReLU


def default_conv(in_channels, out_channels, kernel_size, bias=True):
    """amssrn.py:69-72."""
    return HipConv2d(in_channels, out_channels, kernel_size, padding=kernel_size // 2, bias=bias)


class Upsampler(nn.Sequential):
    """amssrn.py:74-91: (conv n -> 4n, shuffle 2) per factor 2, or the SAME (conv n -> 9n, shuffle 3) pair per factor 3 (tied)."""

    def __init__(self, conv, scale, n_feats, bias=True):
        m = []
        three = [conv(n_feats, 9 * n_feats, 3, bias), _Shuffle(3)]
        if (scale & (scale - 1)) == 0:
            for _ in range(int(math.log(scale, 2))):
                m.append(conv(n_feats, 4 * n_feats, 3, bias))
                m.append(_Shuffle(2))
        elif scale % 3 == 0:
            for _ in range(int(math.log(scale, 3))):
                m += three
        else:
            raise NotImplementedError
        super().__init__(*m)


class _NonLocalBlockND(nn.Module):
    """amssrn.py:93-139 (embedded Gaussian, no energy scaling); W starts at zero, as in the reference.  Called on a whole map it runs
    the attention per quadrant (Nonlocal_CA's split), which is the only way the reference uses it."""

    def __init__(self, in_channels, inter_channels=None, dimension=2):
        super().__init__()
        if inter_channels != 8 or dimension != 2:
            raise NotImplementedError('_NonLocalBlockND: the HIP quadrant attention runs 8 inter channels in 2-D')
        self.dimension, self.in_channels, self.inter_channels = dimension, in_channels, inter_channels
        self.softmax = nn.Softmax(dim=-1)
        self.g = HipConv2d(in_channels, inter_channels, 1, 1, 0)
        self.W = HipConv2d(inter_channels, in_channels, 1, 1, 0)
        nn.init.constant_(self.W.weight, 0)
        nn.init.constant_(self.W.bias, 0)
        self.concat_project = None
        self.theta = HipConv2d(in_channels, inter_channels, 1, 1, 0)
        self.phi = HipConv2d(in_channels, inter_channels, 1, 1, 0)

    def forward_quadrants(self, x):
        y = ops.nonlocal_quadrants(self.theta(x), self.phi(x), self.g(x))
        return self.W(y, residual=x)


class Nonlocal_CA(nn.Module):
    """amssrn.py:141-165: the non-local block on the four quadrants split at H // 2, W // 2."""

    def __init__(self, in_feat=64, inter_feat=32):
        super().__init__()
        self.non_local = _NonLocalBlockND(in_channels=in_feat, inter_channels=inter_feat)

    def forward(self, x):
        return self.non_local.forward_quadrants(ops.nhwc(x))


class CALayer(nn.Module):
    """amssrn.py:167-183: x * sigmoid(conv(prelu(conv(avgpool x)))), both 1x1 convs with bias."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv_du = nn.Sequential(HipConv2d(channel, channel // reduction, 1, padding=0, bias=True), HipPReLU(),
                                     HipConv2d(channel // reduction, channel, 1, padding=0, bias=True), nn.Sigmoid())

    def forward(self, x):
        c1, act, c2 = self.conv_du[0], self.conv_du[1], self.conv_du[2]
        return ops.channel_attention_bias_prelu(x, c1.weight, c1.bias, act.weight, c2.weight, c2.bias)


class RB(nn.Module):
    """amssrn.py:185-198: x + conv3X3(x) + rb(x), rb = conv, PReLU, conv; both adds in conv epilogues."""

    def __init__(self, n_feats):
        super().__init__()
        self.conv3X3 = HipConv2d(n_feats, n_feats, 3, padding=1)
        self.rb = nn.Sequential(HipConv2d(n_feats, n_feats, 3, padding=1), HipPReLU(), HipConv2d(n_feats, n_feats, 3, padding=1))

    def forward(self, x):
        x = ops.nhwc(x)
        t = self.conv3X3(x, residual=x)
        return self.rb[2](self.rb[1](self.rb[0](x)), residual=t)


class ASPP(nn.Module):
    """amssrn.py:200-217: dilated 3x3 convs d = 1, 2, 3 sharing one PReLU, concatenated."""

    def __init__(self, n_feats):
        super().__init__()
        self.d1 = HipDilatedConv2d(n_feats, n_feats, 3, padding=1, dilation=1)
        self.d2 = HipDilatedConv2d(n_feats, n_feats, 3, padding=2, dilation=2)
        self.d3 = HipDilatedConv2d(n_feats, n_feats, 3, padding=3, dilation=3)
        self.act = HipPReLU()

    def forward(self, x):
        return ops.cat_channels([self.act(self.d1(x)), self.act(self.d2(x)), self.act(self.d3(x))])


class DB(nn.Module):
    """amssrn.py:219-238."""

    def __init__(self, in_channels):
        super().__init__()
        self.c1, self.c2, self.c3, self.c4 = RB(in_channels), RB(in_channels), RB(in_channels), RB(in_channels)
        self.ca = CALayer(in_channels * 5)
        self.c5 = HipConv2d(in_channels * 5, in_channels, 1)

    def forward(self, input):
        input = ops.nhwc(input)
        o1 = self.c1(input)
        o2 = self.c2(o1)
        o3 = self.c3(o2)
        o4 = self.c4(o3)
        return self.c5(self.ca(ops.cat_channels([input, o1, o2, o3, o4])), residual=input)


class DB_ASPP(nn.Module):
    """amssrn.py:240-261."""

    def __init__(self, in_channels):
        super().__init__()
        self.c1, self.c2, self.c3, self.c4 = RB(in_channels), RB(in_channels), RB(in_channels), RB(in_channels)
        self.aspp = ASPP(in_channels * 4)
        self.ca = CALayer(in_channels * 12)
        self.c5 = HipConv2d(in_channels * 12, in_channels, 1)

    def forward(self, input):
        input = ops.nhwc(input)
        o1 = self.c1(input)
        o2 = self.c2(o1)
        o3 = self.c3(o2)
        o4 = self.c4(o3)
        return self.c5(self.ca(self.aspp(ops.cat_channels([o1, o2, o3, o4]))), residual=input)


class FPN_Fusion(nn.Module):
    """amssrn.py:263-278: slot 0 = fusion[0](f[-1]), slot i + 1 = fusion[i + 1](f[-(i + 2)] + f[-(i + 1)])."""

    def __init__(self, num_features, n_feats=64):
        super().__init__()
        self.fusion = nn.Sequential(*[HipConv2d(n_feats, n_feats, 3, padding=1) for _ in range(num_features)])

    def forward(self, feature_list):
        out = [self.fusion[0](feature_list[-1])]
        for i in range(len(feature_list) - 1):
            out.append(self.fusion[i + 1](ops.sum_tensors([feature_list[-(i + 2)], feature_list[-(i + 1)]])))
        return out


class GeneratorResNet(nn.Module):
    """amssrn.py:280-334: 64 features, 4 DB + 4 DB_ASPP, two quadrant non-local blocks, FPN fusion of 11 maps, upsampler."""

    def __init__(self, conv=default_conv, scale=4):
        super().__init__()
        n_feats, n_blocks, kernel_size = 64, 8, 3
        self.n_blocks = n_blocks
        # registration order of the reference (named_parameters() order: gamma first, then the children in this order)
        self.fpn_fusion = FPN_Fusion(n_blocks + 3)
        self.feature_bank = HipConv2d((n_blocks + 3) * n_feats, n_feats, 1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.non_local_1 = Nonlocal_CA(in_feat=n_feats, inter_feat=n_feats // 8)
        self.non_local_2 = Nonlocal_CA(in_feat=n_feats, inter_feat=n_feats // 8)
        self.head = nn.Sequential(conv(3, n_feats, kernel_size))
        self.body = nn.Sequential(*([DB(n_feats) for _ in range(n_blocks // 2)] + [DB_ASPP(n_feats) for _ in range(n_blocks // 2)]))
        self.tail = Upsampler(conv, scale, n_feats)
        self.reconstruction = HipConv2d(n_feats, 3, 3, padding=1)

    def forward(self, x):
        head = self.head[0](ops.nhwc(x))
        nl1 = self.non_local_1(head)
        feats = [head, nl1]
        x = nl1
        for block in self.body:
            x = ops.gamma_residual(block(x), nl1, self.gamma)
            feats.append(x)
        feats.append(self.non_local_2(x))
        fused = self.fpn_fusion(feats)
        bank = ops.cat_channels([ops.cat_channels(fused[:8])] + fused[8:])
        bottleneck = self.feature_bank(bank, residual=head)
        return self.reconstruction(self.tail(bottleneck))


def train_step(G, opt_G, lr_img, hr_img, loss_Lp_norm='L1'):
    """One generator iteration of amssrn.py:510-532: loss_G = L1(gen, hr) ('L1') or MSE(gen, hr) (anything else), then
    opt_G.step().  The VGG content loss (:523-527) never enters loss_G: skipped.  Returns loss_G as a 0-d device tensor (no host
    sync)."""
    opt_G.zero_grad(set_to_none=True)
    gen_hr = G(lr_img)
    loss_G = ops.l1_mean(gen_hr, hr_img) if loss_Lp_norm == 'L1' else ops.mse_mean(gen_hr, hr_img)
    loss_G.backward()
    opt_G.step()
    ops.bump_weight_epoch()
    return loss_G.detach()
