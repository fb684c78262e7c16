"""The blocks of the reference's model/base_networks.py that the HIP path reaches: ChannelAttention (base_networks.py:366-403)
and SpatialAttention (:424-457), used by the discriminator (sradsgan.py:495-496) and arithmetically the generator's CLAM / SLAM;
and the patch Discriminator (:1747-1805) that DRCAN trains against."""
import torch.nn as nn

from .. import ops
from .layers import HipConv2d


class _Clam(nn.Module):
    """sigmoid(sum over the pools in pool_mode of MLP(pool x)) * x with a shared bias-free 1x1 MLP C -> C/ratio -> C."""

    def __init__(self, in_planes, ratio=16, pool_mode='Avg|Max'):
        super().__init__()
        if pool_mode not in ops.POOL_MODES:      # fail at construction, not at the first forward
            raise ValueError("CLAM / ChannelAttention: pool_mode must be 'Avg', 'Max' or 'Avg|Max', got %r" % (pool_mode,))
        self.pool_mode = pool_mode
        self.fc1 = HipConv2d(in_planes, in_planes // ratio, 1, bias=False)
        self.fc2 = HipConv2d(in_planes // ratio, in_planes, 1, bias=False)

    def forward(self, x):
        return ops.clam(x, self.fc1.weight, self.fc2.weight, self.pool_mode)


class _Slam(nn.Module):
    """sigmoid(conv kxk(the maps in pool_mode of [mean_c x, max_c x])) * x, k in (3, 7), no bias."""

    def __init__(self, kernel_size=7, pool_mode='Avg|Max'):
        super().__init__()
        assert kernel_size in (3, 7), 'kernel size must be 3 or 7'
        if pool_mode not in ops.POOL_MODES:
            raise ValueError("SLAM / SpatialAttention: pool_mode must be 'Avg', 'Max' or 'Avg|Max', got %r" % (pool_mode,))
        self.pool_mode = pool_mode
        self.conv1 = HipConv2d(2 if pool_mode == 'Avg|Max' else 1, 1, kernel_size, padding=3 if kernel_size == 7 else 1, bias=False)

    def forward(self, x):
        return ops.slam(x, self.conv1.weight, self.pool_mode)


class ChannelAttention(_Clam):
    pass


class SpatialAttention(_Slam):
    pass


class Discriminator(nn.Module):
    """base_networks.py:1747-1805: the 8-block patch discriminator with a choice of normalisation, spectral norm and the attention
    pair after block 6.  With norm_type='batch' and no spectral norm it is, layer for layer and key for key, sradsgan.py's
    discriminator (DRCAN's D is `attention=False`, drcan.py:507-508), and it runs on the same HIP blocks.  The other normalisations
    and spectral norm are not built on the HIP path."""

    def __init__(self, in_channels=3, norm_type='', use_spectralnorm=False, attention=False):
        super().__init__()
        if use_spectralnorm:
            raise NotImplementedError('Discriminator: spectral norm is not built on the HIP path')
        if norm_type != 'batch':
            raise NotImplementedError("Discriminator: norm_type %r is not built on the HIP path; 'batch' is (DRCAN's "
                                      "Discriminator(norm_type='batch'))" % (norm_type,))
        from .sradsgan import Discriminator as _PatchD          # (imported here: sradsgan.py imports this module)
        d = _PatchD(in_channels, attention=attention)
        self.norm_type, self.attention = norm_type, attention
        self.model, self._blocks = d.model, d._blocks

    def forward(self, img):
        from .sradsgan import Discriminator as _PatchD
        return _PatchD.forward(self, img)
