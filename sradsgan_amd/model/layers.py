"""Parameter containers whose forward runs on the HIP C ABI.  They subclass the torch.nn containers
only to keep constructor arguments, parameter names (`weight`, `bias`, BN buffers) and therefore
state_dict keys identical to the reference's nn.Conv2d / nn.BatchNorm2d."""
import torch
import torch.nn as nn

from .. import ops


class HipConv2d(nn.Conv2d):
    """nn.Conv2d replacement: implicit-GEMM MFMA conv with the call site's elementwise tail fused."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        k, s, p, d = self.kernel_size, self.stride, self.padding, self.dilation
        if k[0] != k[1] or s[0] != s[1] or p[0] != p[1] or d != (1, 1) or self.groups != 1:
            raise NotImplementedError('HipConv2d: square kernel/stride/pad, dilation 1, groups 1 only')

    def forward(self, x, act_slope=None, residual=None):
        return ops.conv2d(x, self.weight, self.bias, self.stride[0], self.padding[0], act_slope, residual)


class HipBatchNorm2d(nn.BatchNorm2d):
    """Train-mode BatchNorm2d (+ optional fused LeakyReLU) used by the discriminator
    (reference sradsgan.py:478-479).  Differentiable twice (gradient penalty)."""

    def forward(self, x, act_slope=None):
        return ops.batch_norm_act(x, self, act_slope)


class HipInstanceNorm2d(nn.InstanceNorm2d):
    """nn.InstanceNorm2d(C) as the reference's patch discriminator builds it (base_networks.py:1762-1763: no affine, no running
    statistics, hence no parameters, no buffers and no state_dict keys) + optional fused LeakyReLU.  Differentiable twice."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=False, track_running_stats=False):
        if affine or track_running_stats:
            raise NotImplementedError('HipInstanceNorm2d: nn.InstanceNorm2d(C) without affine and running statistics only')
        super().__init__(num_features, eps, momentum, False, False)

    def forward(self, x, act_slope=None):
        if x.shape[1] != self.num_features:
            raise ValueError('HipInstanceNorm2d: expected %d channels, got %d' % (self.num_features, x.shape[1]))
        return ops.group_norm_act(x, self.num_features, None, None, self.eps, False, act_slope)


class GroupNorm(nn.Module):
    """The reference's own GroupNorm (base_networks.py:12-31), class name and parameter shapes included: `num_groups` groups of
    adjacent channels, the UNBIASED variance (x.var(-1)) with eps inside the root, weight = ones and bias = zeros of shape
    (1, C, 1, 1) + optional fused LeakyReLU.  Differentiable twice."""

    def __init__(self, num_features, num_groups=32, eps=1e-5):
        super().__init__()
        if num_features % num_groups:
            raise ValueError('GroupNorm: %d channels do not divide into %d groups' % (num_features, num_groups))
        self.weight = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.bias = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.num_groups = num_groups
        self.eps = eps

    def forward(self, x, act_slope=None):
        return ops.group_norm_act(x, self.num_groups, self.weight, self.bias, self.eps, True, act_slope)


class HipDilatedConv2d(nn.Conv2d):
    """nn.Conv2d(k = 3, stride 1, padding = dilation) with dilation 1..3 (AMSSRN's ASPP, amssrn.py:200-209) on the HIP dilated path.
    HipConv2d keeps refusing dilation: its fused epilogues and data-gradient forms are the plain conv's."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        k, s, p, d = self.kernel_size, self.stride, self.padding, self.dilation
        if k != (3, 3) or s != (1, 1) or d[0] != d[1] or p != d or not 1 <= d[0] <= ops.DIL_MAX or self.groups != 1:
            raise NotImplementedError('HipDilatedConv2d: 3x3, stride 1, padding = dilation in 1..%d, groups 1 only' % ops.DIL_MAX)

    def forward(self, x):
        return ops.conv2d_dil(x, self.weight, self.bias, self.dilation[0])


class HipPReLU(nn.PReLU):
    """nn.PReLU() with one slope: y = z > 0 ? z : a z, the slope read on the device (no host synchronisation)."""

    def __init__(self, num_parameters=1, init=0.25):
        if num_parameters != 1:
            raise NotImplementedError('HipPReLU: one slope per module (nn.PReLU())')
        super().__init__(num_parameters, init)

    def forward(self, x):
        return ops.prelu(x, self.weight)
