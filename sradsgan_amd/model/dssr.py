"""DSSR generator on the same HIP kernels.  Mirrors SRADSGAN/model/dssr.py:69-177 (CA, WAB, ResGroup, UP, GeneratorResNet) with
the reference's constructor signatures (unused arguments included) and state_dict keys (weight-tied `UP.upsampling.{0,2,...}` stages),
and one iteration of its training loop (:362-374) as `train_step`.

Execution differs from the reference's graph in two places, both exact in real arithmetic:
  * WAB: conv2's epilogue leaves the channel sums of its output behind (split-bf16 arithmetic), and the average-pool channel
    attention and the block's `out += x` run as one scale-and-add pass (ops.ca_residual);
  * the multi-level reconstruction `UP(out0) + sum_i UP(y_i)` (:170-177) runs UP once: UP is affine (conv + pixel shuffle, no
    activation), so sum_{i=0..G} UP(x_i) = UP(sum_i x_i) + G UP(0), where UP(0) is computed on one zero image (its borders differ
    from UP's bias through the zero padding of the second stage) and broadcast over the batch.  The sum of the G + 1 trunk tensors
    is one pass (ops.sum_tensors)."""
import math

import torch
import torch.nn as nn

from .. import ops
from .layers import HipConv2d


class CA(nn.Module):
    """dssr.py:69-82: sigmoid(fc2(relu(fc1(avgpool x)))) * x.  pool_mode is accepted and ignored, as in the reference (the
    average pool is the only one it applies)."""

    def __init__(self, in_planes, ratio=16, pool_mode='Avg|Max'):
        super().__init__()
        self.pool_mode = pool_mode
        self.fc1 = HipConv2d(in_planes, in_planes // ratio, 1, bias=False)
        self.fc2 = HipConv2d(in_planes // ratio, in_planes, 1, bias=False)

    def forward(self, x, residual, pool=None):
        """CA(x) + residual; pool: the channel sums of x left by the conv that produced it (ops.conv2d_pool)."""
        return ops.ca_residual(x, residual, self.fc1.weight, self.fc2.weight, pool)


class WAB(nn.Module):
    """dssr.py:84-104: conv 3x3 inplanes -> 4 planes (+bias), ReLU, conv 3x3 -> planes (+bias), CA, += x.  act_type, la_mode and
    addconv are accepted and ignored, as in the reference."""

    def __init__(self, inplanes, planes, kernel_size=3, stride=1, padding=1, bias=True, dilation=1, act_type='lrelu',
                 la_mode='CA-SA', pool_mode='Avg|Max', addconv=True):
        super().__init__()
        if planes != 64 or inplanes != planes or stride != 1 or kernel_size != 2 * padding + 1:
            raise NotImplementedError('WAB: the HIP path runs 64 -> 256 -> 64 channels, stride 1, "same" padding')
        self.inplanes, self.planes = inplanes, planes
        self.conv1 = HipConv2d(inplanes, 4 * planes, kernel_size, stride, padding, bias=bias, dilation=dilation)
        self.conv2 = HipConv2d(4 * planes, planes, kernel_size, stride, padding, bias=bias, dilation=dilation)
        self.la_mode, self.addconv = la_mode, addconv
        self.ca = CA(planes, pool_mode=pool_mode)

    def forward(self, x):
        t = self.conv1(x, act_slope=0.0)                               # ReLU fused into conv1's epilogue
        c2 = self.conv2
        if c2.kernel_size == (3, 3) and c2.padding == (1, 1):
            u, pool = ops.conv2d_pool(t, c2.weight, c2.bias)           # + the channel sums of u when the epilogue can produce them
        else:
            u, pool = c2(t), None
        return self.ca(u, x, pool)


class ResGroup(nn.Module):
    """dssr.py:106-122: n_blocks blocks, conv 3x3 nc -> nc (+bias), += x (fused into the conv's epilogue)."""

    def __init__(self, block, n_blocks=10, nc=64, kernel_size=3, stride=1, bias=True, padding=1,
                 act_type='lrelu', mode='CNA', rla_mode='CA-SA', bla_mode='CA-SA', pool_mode='Avg|Max', addconv=True):
        super().__init__()
        self.conv = HipConv2d(nc, nc, kernel_size, stride, padding)
        self.RG = nn.Sequential(*[block(nc, nc, kernel_size=kernel_size, bias=bias, stride=stride, padding=padding,
                                        act_type='lrelu', la_mode=bla_mode, pool_mode=pool_mode, addconv=addconv)
                                  for _ in range(n_blocks)])

    def forward(self, x):
        return self.conv(self.RG(x), residual=x)


class _Shuffle(nn.Module):
    """The Sequential slot of nn.PixelShuffle, without an activation (dssr.py:129-132)."""

    slope = None

    def __init__(self, r):
        super().__init__()
        self.upscale_factor = r

    def forward(self, x):
        return ops.pixel_shuffle_act(x, self.upscale_factor, self.slope)


class UP(nn.Module):
    """dssr.py:124-145: conv 64 -> 64 r^2 + pixel shuffle per stage; the stages of x4 / x8 / x9 are ONE module pair repeated, so
    their weights are tied and state_dict lists them under every stage index, as in the reference."""

    def __init__(self, ga_mode='CA-SA', addconv=True, upscale_factor=4):
        super().__init__()
        if (upscale_factor & (upscale_factor - 1)) == 0:
            r, stages = 2, int(math.log(upscale_factor, 2))
        elif upscale_factor % 3 == 0:
            r, stages = 3, int(math.log(upscale_factor, 3))
        else:
            r, stages = 1, 0
        stage = [HipConv2d(64, 64 * r * r, 3, 1, 1), _Shuffle(r)]
        self.upsampling = nn.Sequential(*(stage * stages))

    def is_affine(self):
        """True when every slot is a conv or a pixel shuffle without activation (what the fold in GeneratorResNet relies on)."""
        return all(isinstance(m, HipConv2d) or (isinstance(m, _Shuffle) and m.slope is None) for m in self.upsampling)

    def forward(self, x):
        return self.upsampling(x)


class GeneratorResNet(nn.Module):
    """dssr.py:147-177.  buildingblock is the group class (ResGroup); rla/bla/ga_mode and addconv are accepted and ignored, as in
    the reference."""

    def __init__(self, buildingblock, in_channels=3, out_channels=3, n_residual_blocks=3, n_basic_blocks=10,
                 rla_mode='CA-SA', bla_mode='CA-SA', ga_mode='CA-SA', pool_mode='Avg|Max', addconv=True, upscale_factor=4):
        super().__init__()
        self.conv1 = nn.Sequential(HipConv2d(in_channels, 64, 3, 1, 1))
        self.res_groups = nn.Sequential(*[
            buildingblock(WAB, n_blocks=n_basic_blocks, nc=64, kernel_size=3, stride=1, padding=1, act_type='lrelu', mode='CNA',
                          rla_mode=rla_mode, bla_mode=bla_mode, pool_mode=pool_mode, addconv=addconv)
            for _ in range(n_residual_blocks)])
        self.UP = UP(ga_mode=ga_mode, addconv=addconv, upscale_factor=upscale_factor)
        self.conv3 = nn.Sequential(HipConv2d(64, out_channels, 3, 1, 1))

    def forward(self, x):
        # the fold below is exact only for an affine upsampler
        assert self.UP.is_affine(), 'DSSR upsampler fold: UP must be convs and pixel shuffles without activation'
        out = self.conv1[0](ops.nhwc(x))
        trunk = [out]
        for group in self.res_groups:
            out = group(out)
            trunk.append(out)
        g = len(trunk) - 1
        # UP(out0) + sum_i UP(y_i) = UP(out0 + sum_i y_i) + G UP(0)
        out_all = self.UP(ops.sum_tensors(trunk))
        if g:
            zero = torch.zeros((1,) + tuple(out.shape[1:]), device=out.device, dtype=out.dtype).contiguous(memory_format=ops.CL)
            out_all = ops.add_bcast_scaled(out_all, self.UP(zero), float(g))
        return self.conv3[0](out_all)


def train_step(G, opt_G, lr_img, hr_img, loss_Lp_norm='L1'):
    """One generator iteration of dssr.py:362-374: loss_G = L1(gen, hr) ('L1') or MSE(gen, hr) (anything else, :266-269), then
    opt_G.step().  The reference also computes VGG features of gen and hr (:367-369), which never enter loss_G and are not logged:
    they are skipped.  Returns loss_G as a 0-d device tensor (no host sync)."""
    opt_G.zero_grad(set_to_none=True)
    gen_hr = G(lr_img)
    loss_G = ops.l1_mean(gen_hr, hr_img) if loss_Lp_norm == 'L1' else ops.mse_mean(gen_hr, hr_img)
    loss_G.backward()
    opt_G.step()
    ops.bump_weight_epoch()
    return loss_G.detach()
