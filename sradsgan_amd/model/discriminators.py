"""The reference's patch discriminator with its choice of normalisation (base_networks.py:1747-1805):
Discriminator(in_channels=3, norm_type='', use_spectralnorm=False, attention=False), on the HIP path for norm_type '' (none),
'instance', 'group' and 'batch'.  Same constructor signature and, per norm_type, the same state_dict keys in the same order with the
same shapes, so `from sradsgan_amd.model.discriminators import PatchDiscriminator as Discriminator` replaces the reference class.

The nn.Sequential indices differ per variant, as they do in the reference: '' has no norm slot in a block, 'instance' has a slot
without keys (nn.InstanceNorm2d(C): no affine, no running statistics), 'group' a slot with weight and bias of shape (1, C, 1, 1)
(the reference's own GroupNorm, unbiased variance), 'batch' a BatchNorm2d.  Block 1 never has a norm.  A per-sample norm ('instance',
'group') or none makes D(x)[i] independent of the other samples of the batch -- what a per-sample gradient penalty assumes.

use_spectralnorm=True is refused HERE: the reference's SpectralNorm advances its power-iteration vectors u and v on EVERY forward, so
D(fake) in the discriminator phase no longer equals D(gen_hr) in the generator phase, and TrainStep (reuse_d_fake, the one-walk
backward) rests on that equality.  The spectral discriminator is its own class, model.spectral.SpectralPatchDiscriminator (same keys as
the reference's Discriminator(..., use_spectralnorm=True, ...)), which TrainStep runs on its plain order."""
import torch.nn as nn

from .. import ops
from .base_networks import ChannelAttention, SpatialAttention
from .layers import GroupNorm, HipBatchNorm2d, HipConv2d, HipInstanceNorm2d

NORM_TYPES = ('', 'instance', 'group', 'batch')

_NORMS = {'instance': HipInstanceNorm2d, 'group': GroupNorm, 'batch': HipBatchNorm2d}


class PatchDiscriminator(nn.Module):
    _PLAN = [(64, 1, False), (64, 2, True), (128, 1, True), (128, 2, True), (256, 1, True), (256, 2, True), (512, 1, True), (512, 2, True)]

    def __init__(self, in_channels=3, norm_type='', use_spectralnorm=False, attention=False):
        super().__init__()
        if use_spectralnorm:
            raise NotImplementedError('PatchDiscriminator: spectral norm is not built on the HIP path: the reference\'s SpectralNorm '
                                      'advances u and v on every forward, so D(fake) of the D phase differs from D(gen_hr) of the G '
                                      'phase, the equality TrainStep (reuse_d_fake, the one-walk backward) rests on')
        if norm_type not in NORM_TYPES:
            raise ValueError('PatchDiscriminator: norm_type must be one of %r, got %r' % (NORM_TYPES, norm_type))
        self.norm_type, self.attention = norm_type, attention
        if norm_type == 'batch':                 # the existing blocks, unchanged
            from .sradsgan import Discriminator as _BatchD
            d = _BatchD(in_channels, attention=attention)
            self.model, self._blocks = d.model, d._blocks
            return
        layers, cin = [], in_channels
        self._blocks = []                        # (conv idx, norm idx or None, [attention idxs])
        for idx, (cout, stride, norm) in enumerate(self._PLAN, start=1):
            entry = [len(layers), None, []]
            layers.append(HipConv2d(cin, cout, 3, stride, 1))
            if norm and norm_type:
                entry[1] = len(layers)
                layers.append(_NORMS[norm_type](cout))
            layers.append(nn.Identity())         # slot of LeakyReLU(0.2): fused into the conv / the norm
            if attention and idx == 6:
                entry[2] = [len(layers), len(layers) + 1]
                layers += [ChannelAttention(256), SpatialAttention()]
            self._blocks.append(tuple(entry))
            cin = cout
        layers.append(HipConv2d(cin, 1, 3, 1, 1))
        self.model = nn.Sequential(*layers)

    def forward(self, img):
        x = ops.nhwc(img)
        m = self.model
        for conv_i, norm_i, extra in self._blocks:
            if norm_i is None:
                x = m[conv_i](x, act_slope=0.2)
            else:
                x = m[norm_i](m[conv_i](x), act_slope=0.2)
            for e in extra:
                x = m[e](x)
        return m[len(m) - 1](x)
