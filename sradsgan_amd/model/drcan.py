"""DRCAN (RCAN) generator on the HIP kernels.  Mirrors SRADSGAN/model/drcan.py:35-226 (default_conv, Upsampler, CALayer, RCAB,
ResidualGroup, RCAN) with the reference's constructor signatures, defaults and state_dict keys, RCAN's own load_state_dict, and the
DRCAN trainer (drcan.py:486-1095): SRADSGAN's WGAN-GP loop (TrainStep) with RCAN and base_networks' discriminator.

Execution, exact in real arithmetic:
  * RCAB: conv1's epilogue applies the ReLU; conv2's epilogue leaves the channel sums of its output (ops.conv2d_pool); the channel
    attention with its biases and the block's `res += x` run as one scale-and-add pass (ops.ca_residual with fc1_b / fc2_b);
  * ResidualGroup's and RCAN's `res += x` ride in the epilogue of the conv that ends the body;
  * the upsampler is one conv + pixel shuffle per stage, the stages not weight-tied (unlike DSSR's UP)."""
import math

import torch
import torch.nn as nn

from .. import checkpoint as ckpt
from .. import ops
from .. import trainer as _trainer
from .base_networks import Discriminator
from .dssr import _Shuffle
from .layers import HipConv2d


def default_conv(in_channels, out_channels, kernel_size, bias=True):
    """drcan.py:35-38."""
    return HipConv2d(in_channels, out_channels, kernel_size, padding=kernel_size // 2, bias=bias)


class Upsampler(nn.Sequential):
    """drcan.py:66-91: (conv n -> 4n, shuffle 2) per factor 2 for 2^n scales, else int(log3(scale)) stages of (conv n -> 9n,
    shuffle 3) for scales divisible by 3 (scale 6 therefore builds ONE x3 stage, as in the reference); any other scale raises."""

    def __init__(self, conv, scale, n_feat, bn=False, act=False, bias=True):
        if bn or act:
            raise NotImplementedError('Upsampler: BatchNorm / activation stages are not built on the HIP path (RCAN uses neither)')
        m = []
        if (scale & (scale - 1)) == 0:
            for _ in range(int(math.log(scale, 2))):
                m += [conv(n_feat, 4 * n_feat, 3, bias), _Shuffle(2)]
        elif scale % 3 == 0:
            for _ in range(int(math.log(scale, 3))):
                m += [conv(n_feat, 9 * n_feat, 3, bias), _Shuffle(3)]
        else:
            raise NotImplementedError
        super().__init__(*m)


class CALayer(nn.Module):
    """drcan.py:94-111: x * sigmoid(conv_du(avgpool x)), conv_du = 1x1 (+bias), ReLU, 1x1 (+bias), Sigmoid.  64 channels and
    1..16 hidden units (reduction 4 and 16 for RCAN's 64 features) on the HIP path."""

    def __init__(self, channel, reduction=4):
        super().__init__()
        hidden = channel // reduction
        if channel != 64 or not 1 <= hidden <= 16:
            raise NotImplementedError('CALayer: the HIP channel attention serves 64 channels with 1..16 hidden units, got %d / %d'
                                      % (channel, hidden))
        self.conv_du = nn.Sequential(HipConv2d(channel, hidden, 1, padding=0, bias=True), nn.ReLU(inplace=True),
                                     HipConv2d(hidden, channel, 1, padding=0, bias=True), nn.Sigmoid())

    def forward(self, x, residual=None, pool=None):
        """CALayer(x) + residual (zero when None); pool: the channel sums of x left by the conv that produced it (ops.conv2d_pool)."""
        if residual is None:
            residual = torch.zeros_like(ops.nhwc(x), memory_format=ops.CL)
        fc1, fc2 = self.conv_du[0], self.conv_du[2]
        return ops.ca_residual(x, residual, fc1.weight, fc2.weight, pool, fc1.bias, fc2.bias)


class RCAB(nn.Module):
    """drcan.py:114-135: conv, ReLU, conv, CALayer, `res += x` (res_scale is accepted and unused, as in the reference)."""

    def __init__(self, conv, n_feat, kernel_size, reduction, bias=True, bn=False, act=nn.ReLU(True), res_scale=1):
        super().__init__()
        if bn:
            raise NotImplementedError('RCAB: BatchNorm in the block is not built on the HIP path (RCAN uses none)')
        _require_hip_shape(n_feat, kernel_size, 'RCAB')
        self.body = nn.Sequential(conv(n_feat, n_feat, kernel_size, bias=bias), act, conv(n_feat, n_feat, kernel_size, bias=bias),
                                  CALayer(n_feat, reduction))
        self.res_scale = res_scale

    def forward(self, x):
        t = self.body[0](x, act_slope=0.0)                             # ReLU fused into conv1's epilogue
        c2 = self.body[2]
        u, pool = ops.conv2d_pool(t, c2.weight, c2.bias)                # + the channel sums of u when the epilogue can produce them
        return self.body[3](u, x, pool)                                # sigmoid(conv_du(avg u)) * u + x in one pass


class ResidualGroup(nn.Module):
    """drcan.py:139-152: n_resblocks RCABs, conv, `res += x` (fused into the conv's epilogue)."""

    def __init__(self, conv, n_feat, kernel_size, reduction, act, res_scale, n_resblocks):
        super().__init__()
        _require_hip_shape(n_feat, kernel_size, 'ResidualGroup')
        body = [RCAB(conv, n_feat, kernel_size, reduction, bias=True, bn=False, act=nn.ReLU(True), res_scale=1)
                for _ in range(n_resblocks)]
        body.append(conv(n_feat, n_feat, kernel_size))
        self.body = nn.Sequential(*body)

    def forward(self, x):
        res = x
        for blk in self.body[:-1]:
            res = blk(res)
        return self.body[-1](res, residual=x)


def _require_hip_shape(n_feat, kernel_size, what):
    if n_feat != 64 or kernel_size != 3:
        raise NotImplementedError('%s: the HIP path runs 64 features with 3x3 convs (n_feats=64, kernel_size=3), got %d / %d'
                                  % (what, n_feat, kernel_size))


class RCAN(nn.Module):
    """drcan.py:156-226.  Keys head.0, body.0..G-1 (groups), body.G (conv), tail.0.* (upsampler), tail.1."""

    def __init__(self, n_colors=3, n_resgroups=5, n_resblocks=10, n_feats=64, kernel_size=3, reduction=4, scale=3,
                 conv=default_conv, res_scale=1):
        super().__init__()
        _require_hip_shape(n_feats, kernel_size, 'RCAN')
        act = nn.ReLU(True)
        self.head = nn.Sequential(conv(n_colors, n_feats, kernel_size))
        body = [ResidualGroup(conv, n_feats, kernel_size, reduction, act=act, res_scale=res_scale, n_resblocks=n_resblocks)
                for _ in range(n_resgroups)]
        body.append(conv(n_feats, n_feats, kernel_size))
        self.body = nn.Sequential(*body)
        self.tail = nn.Sequential(Upsampler(conv, scale, n_feats, act=False), conv(n_feats, n_colors, kernel_size))

    @property
    def res_groups(self):
        """The ResidualGroup modules in order (registers nothing: the state_dict is unchanged).  TrainStep._plan_g_parts uses them to
        hand the generator's gradients to the data-parallel exchange in parts during the backward."""
        return [m for m in self.body if isinstance(m, ResidualGroup)]

    def forward(self, x):
        x = self.head[0](ops.nhwc(x))
        res = x
        for grp in self.body[:-1]:
            res = grp(res)
        res = self.body[-1](res, residual=x)                           # `res += x` in the conv's epilogue
        for m in self.tail[0]:
            res = m(res)
        return self.tail[1](res)

    def load_state_dict(self, state_dict, strict=False):
        """drcan.py:201-226: copy every key the model has; a copy that fails (shape) is skipped, with a message for tail keys (the
        upsampler of another scale); strict=True raises KeyError on unexpected non-tail keys and on missing keys."""
        own_state = self.state_dict()
        with torch.no_grad():
            for name, param in state_dict.items():
                if name in own_state:
                    if isinstance(param, nn.Parameter):
                        param = param.data
                    try:
                        own_state[name].copy_(param)
                    except Exception:
                        if name.find('tail') >= 0:
                            print('Replace pre-trained upsampler to new one...')
                elif strict:
                    if name.find('tail') == -1:
                        ckpt._after_load()
                        raise KeyError('unexpected key "{}" in state_dict'.format(name))
        ckpt._after_load()                                             # convs re-pack their weights
        if strict:
            missing = set(own_state.keys()) - set(state_dict.keys())
            if len(missing) > 0:
                raise KeyError('missing keys in state_dict: "{}"'.format(missing))


def default_args(**overrides):
    """main_drcan.py:16-61: SRADSGAN's flags with DRCAN's defaults (model DRCAN, x4, batch 16, test batch 16, 4 loader threads,
    8 CPUs)."""
    d = dict(model_name='DRCAN', scale_factor=4, batch_size=16, test_batch_size=16, num_threads=4, n_cpu=8)
    d.update(overrides)
    return _trainer.default_args(**d)


class DRCAN(_trainer.SRADSGAN):
    """drcan.py:486-1095: SRADSGAN's trainer (same loss terms, WGAN-GP step, clip, plateau control, checkpoint names) with
    RCAN(n_colors=3, n_resgroups=10, n_resblocks=20, reduction=16, scale) and Discriminator(norm_type='batch',
    use_spectralnorm=False, attention=False) (:507-508).  Validation lines of mfeNew_validate carry drcan_* keys.  `n_resgroups` /
    `n_resblocks` on args override the depth (tests).  The loss options stay at the reference defaults here: no iteration of the
    reference's DRCAN step is recorded with another set, so anything else raises NotImplementedError."""

    eval_label = 'drcan'

    def _check_loss_options(self):
        if self.penalty_type != 'LS' or self.grad_penalty_Lp_norm != 'L2' or self.loss_Lp_norm != 'L1' or self.relative:
            raise NotImplementedError('DRCAN runs the reference defaults: LS penalty, L2 gradient norm, L1 content loss, '
                                      'non-relativistic GAN; SRADSGAN and SRAGAN take the options')
        if getattr(self, 'weight_lpips', 0.0) > 0:
            raise NotImplementedError('DRCAN runs the reference defaults: no LPIPS term in the generator loss (weight_lpips = 0); '
                                      'SRADSGAN and SRAGAN take args.weight_lpips')
        if getattr(self, 'weight_contrast', 0.0) > 0:
            raise NotImplementedError('DRCAN runs the reference defaults: no contrastive term in the generator loss (weight_contrast = '
                                      '0); SRADSGAN and SRAGAN take args.weight_contrast')

    def __init__(self, args, train_loader=None, test_loader=None):
        if getattr(args, 'd_norm_type', None) is not None or getattr(args, 'd_attention', False) or getattr(args, 'd_spectralnorm', False):
            raise NotImplementedError("DRCAN trains against Discriminator(norm_type='batch', attention=False) (drcan.py:507-508); "
                                      'SRADSGAN takes args.d_norm_type / args.d_attention / args.d_spectralnorm')
        super().__init__(args, train_loader=train_loader, test_loader=test_loader)
        self.n_resgroups = getattr(args, 'n_resgroups', 10)
        self.n_resblocks = getattr(args, 'n_resblocks', 20)

    def _new_generator(self):
        return RCAN(n_colors=3, n_resgroups=self.n_resgroups, n_resblocks=self.n_resblocks, reduction=16, scale=self.scale_factor)

    def _new_discriminator(self):
        return Discriminator(norm_type='batch', use_spectralnorm=False, attention=False)
