"""HAT generator on the HIP kernels.  Mirrors SRADSGAN/model/hat.py:74-875 (DropPath, ChannelAttention, CAB, Mlp, WindowAttention,
HAB, OCAB, AttenBlocks, RHAG, PatchEmbed, PatchUnEmbed, Upsample, GeneratorResNet) with the reference's constructor signatures,
defaults and state_dict keys (the relative_position_index_SA / _OCA buffers included, the upsampler's stages weight-tied as in the
reference), and one iteration of its training loop (:1058-1074) as `train_step`.

Execution, exact in real arithmetic:
  * tokens are the NHWC rows of a channels_last image, so patch embed / unembed, roll, window partition, nn.Unfold, rearrange and
    window reverse are addressing inside the attention kernels (ops.window_attention); nn.Linear runs on the 1x1 conv route;
  * HAB: `x + drop_path(attn_x) + conv_scale * CAB(xn)` with CAB's channel attention is one pass (ops.hab_combine); the MLP's
    `x + mlp(..)` rides in fc2's epilogue unless a drop-path factor applies (then the same combine pass without CAB);
  * OCAB's `proj(x) + shortcut`, RHAG's `conv(..) + x` and `conv_after_body(..) + x` ride in the epilogues of their convs;
  * `/ img_range + mean` folds into conv_last's bias when img_range == 1.
The reflect padding of check_image_size and `(x - mean) * img_range` on the 3-channel input are torch ops on the LR image."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .dssr import _Shuffle
from .layers import HipConv2d

HEAD_DIM = 16
# The two families the kernels serve, nothing in between: the reference's (embed_dim 96, six heads of 16 channels, window 8 or 9;
# srhip_hat_*) and the published HAT / HAT-L / HAT-S (embed_dim 180 or 144, six heads of 30 or 24, window 16, overlap 0.5; srhip_hatw_*)
WIDE_DIMS = (144, 180)
WIDE_WINDOW = 16
FAMILIES = ('embed_dim 96 with six heads of 16 channels and window_size 8 or 9 (the reference), or embed_dim 144 / 180 with six '
            'heads of 24 / 30 channels, window_size 16 and overlap_ratio 0.5 (HAT-S, HAT, HAT-L)')


def _family_ok(dim, window_size):
    return (dim == 96 and window_size in (8, 9)) or (dim in WIDE_DIMS and window_size == WIDE_WINDOW)


def to_2tuple(x):
    """basicsr.archs.arch_util.to_2tuple."""
    if isinstance(x, (tuple, list)):
        return tuple(x)
    return (x, x)


def _refuse(cond, msg):
    if cond:
        raise NotImplementedError('HAT on the HIP path: ' + msg)


class HipLinear(nn.Linear):
    """nn.Linear over the channels of every pixel (NHWC tokens) on the 1x1 conv route; residual: + r in the epilogue."""

    def forward(self, x, residual=None):
        return ops.linear(x, self.weight, self.bias, residual)


class HipLayerNorm(nn.LayerNorm):
    """nn.LayerNorm(C) over the channels of every pixel, C = 96, 144 or 180."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True):
        super().__init__(normalized_shape, eps=eps, elementwise_affine=elementwise_affine)
        _refuse(tuple(self.normalized_shape) not in ((96,),) + tuple((c,) for c in WIDE_DIMS) or eps != 1e-5
                or not elementwise_affine, 'LayerNorm(96 / 144 / 180, eps=1e-5) with its affine parameters only')

    def forward(self, x):
        return ops.layer_norm(x, self.weight, self.bias)


def _norm(norm_layer, dim):
    _refuse(norm_layer not in (nn.LayerNorm, HipLayerNorm), 'norm_layer must be nn.LayerNorm')
    return HipLayerNorm(dim)


class DropPath(nn.Module):
    """hat.py:74-91.  In train() mode with drop_prob > 0 the factors floor(keep + U[0, 1)) / keep, one per sample, are drawn
    with torch.rand((b, 1, 1)) on the device; factors(b, device) returns them as [b] (None when the path is the identity)."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def factors(self, b, device):
        if not self.drop_prob or not self.training:
            return None
        keep = 1 - self.drop_prob
        r = keep + torch.rand((b, 1, 1), dtype=torch.float32, device=device)
        return (r.floor_() / keep).view(b)


class ChannelAttention(nn.Module):
    """hat.py:94-107: x * sigmoid(conv(relu(conv(avgpool x)))), both 1x1 convs with biases (run inside ops.hab_combine)."""

    def __init__(self, num_feat, squeeze_factor=16):
        super().__init__()
        hidden = num_feat // squeeze_factor
        _refuse(not 1 <= hidden <= 16 or num_feat % 4 or (num_feat > 128 and num_feat not in WIDE_DIMS),
                'channel attention with C %% 4 == 0, C <= 128 or C = 144 / 180, and 1..16 hidden units, got %d / %d'
                % (num_feat, hidden))
        self.attention = nn.Sequential(nn.AdaptiveAvgPool2d(1), HipConv2d(num_feat, hidden, 1, padding=0), nn.ReLU(inplace=True),
                                       HipConv2d(hidden, num_feat, 1, padding=0), nn.Sigmoid())

    def params(self):
        a = self.attention
        return a[1].weight, a[1].bias, a[3].weight, a[3].bias


class CAB(nn.Module):
    """hat.py:109-121: conv3x3, GELU, conv3x3, ChannelAttention.  forward returns the second conv's output u; the attention's
    scale is applied by HAB's combine pass."""

    def __init__(self, num_feat, compress_ratio=3, squeeze_factor=30):
        super().__init__()
        self.cab = nn.Sequential(HipConv2d(num_feat, num_feat // compress_ratio, 3, 1, 1), nn.GELU(),
                                 HipConv2d(num_feat // compress_ratio, num_feat, 3, 1, 1), ChannelAttention(num_feat, squeeze_factor))

    def forward(self, x):
        return self.cab[2](ops.gelu(self.cab[0](x)))


class Mlp(nn.Module):
    """hat.py:123-140: fc1, GELU, fc2 (dropout 0 only)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _refuse(drop > 0, 'dropout rates above 0')
        _refuse(act_layer is not nn.GELU, 'the MLP activation is nn.GELU')
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        _refuse(hidden_features % 4 != 0, 'MLP hidden width must be a multiple of 4')
        self.fc1 = HipLinear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = HipLinear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, residual=None):
        return self.fc2(ops.gelu(self.fc1(x)), residual=residual)


class WindowAttention(nn.Module):
    """hat.py:151-199.  forward(xn, shift) takes the normalised tokens as an image and returns proj(attention) at the pixels' own
    positions (the roll and window reverse included)."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim = dim
        self.window_size = window_size
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        _refuse(attn_drop > 0 or proj_drop > 0, 'dropout rates above 0')
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        self.qkv = HipLinear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = HipLinear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, xn, shift=0):
        ws = self.window_size[0]
        _refuse(self.window_size[1] != ws or not _family_ok(self.dim, ws) or self.num_heads != 6,
                'got dim %d, %d heads, window %s; supported: %s' % (self.dim, self.num_heads, self.window_size, FAMILIES))
        o = ops.window_attention(self.qkv(xn), self.relative_position_bias_table, ops.HAT_SA, ws, shift)
        return self.proj(o)


class HAB(nn.Module):
    """hat.py:201-293, with HAB.__init__'s clamp: a window larger than min(input_resolution) (from img_size) becomes that size
    and the shift 0."""

    def __init__(self, dim, input_resolution, num_heads, window_size=7, shift_size=0, compress_ratio=3, squeeze_factor=30,
                 conv_scale=0.01, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.num_heads = num_heads
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        if min(self.input_resolution) <= self.window_size:
            self.shift_size = 0
            self.window_size = min(self.input_resolution)
        assert 0 <= self.shift_size < self.window_size, 'shift_size must in 0-window_size'
        self.norm1 = _norm(norm_layer, dim)
        self.attn = WindowAttention(dim, window_size=to_2tuple(self.window_size), num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.conv_scale = conv_scale
        self.conv_block = CAB(num_feat=dim, compress_ratio=compress_ratio, squeeze_factor=squeeze_factor)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = _norm(norm_layer, dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.last_drop_factors = (None, None)   # the factors of the last train-mode forward (attention, MLP), for replay
        self.replay_drop_factors = None         # when set: (attention, MLP) factors used instead of fresh draws

    def _factors(self, b, device):
        if self.replay_drop_factors is not None:
            return self.replay_drop_factors
        if not isinstance(self.drop_path, DropPath):
            return None, None
        ka = self.drop_path.factors(b, device)
        km = self.drop_path.factors(b, device)
        return ka, km

    def forward(self, x, x_size=None, rpi_sa=None, attn_mask=None):
        xn = self.norm1(x)
        u = self.conv_block(xn)
        a = self.attn(xn, self.shift_size)
        ka, km = self._factors(x.shape[0], x.device)
        self.last_drop_factors = (ka, km)
        w1, b1, w2, b2 = self.conv_block.cab[3].params()
        x = ops.hab_combine(x, a, u, w1, b1, w2, b2, kb=ka, conv_scale=self.conv_scale)
        if km is None:
            return self.mlp(self.norm2(x), residual=x)
        return ops.hab_combine(x, self.mlp(self.norm2(x)), kb=km)


class OCAB(nn.Module):
    """hat.py:326-411: overlapping cross-attention (queries ws x ws, keys / values the (ws + ws * overlap_ratio)^2 unfold of the
    qkv output with zero padding), proj + shortcut, then `x + mlp(norm2(x))`.  No drop path."""

    def __init__(self, dim, input_resolution, window_size, overlap_ratio, num_heads, qkv_bias=True, qk_scale=None, mlp_ratio=2,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.window_size = window_size
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.overlap_win_size = int(window_size * overlap_ratio) + window_size
        _refuse(self.overlap_win_size != window_size + window_size // 2, 'overlap_ratio 0.5 only')
        self.norm1 = _norm(norm_layer, dim)
        self.qkv = HipLinear(dim, dim * 3, bias=qkv_bias)
        self.unfold = nn.Unfold(kernel_size=(self.overlap_win_size, self.overlap_win_size), stride=window_size,
                                padding=(self.overlap_win_size - window_size) // 2)
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((window_size + self.overlap_win_size - 1) * (window_size + self.overlap_win_size - 1), num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        self.softmax = nn.Softmax(dim=-1)
        self.proj = HipLinear(dim, dim)
        self.norm2 = _norm(norm_layer, dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=nn.GELU)

    def forward(self, x, x_size=None, rpi=None):
        _refuse(not _family_ok(self.dim, self.window_size) or self.num_heads != 6,
                'got dim %d, %d heads, window %d; supported: %s' % (self.dim, self.num_heads, self.window_size, FAMILIES))
        o = ops.window_attention(self.qkv(self.norm1(x)), self.relative_position_bias_table, ops.HAT_OCA, self.window_size)
        x = self.proj(o, residual=x)
        return self.mlp(self.norm2(x), residual=x)


class AttenBlocks(nn.Module):
    """hat.py:413-487: depth HABs (odd ones shifted by ws // 2), then one OCAB."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, compress_ratio, squeeze_factor, conv_scale,
                 overlap_ratio, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        _refuse(use_checkpoint, 'use_checkpoint')
        _refuse(downsample is not None, 'patch merging (downsample)')
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            HAB(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size,
                shift_size=0 if (i % 2 == 0) else window_size // 2, compress_ratio=compress_ratio, squeeze_factor=squeeze_factor,
                conv_scale=conv_scale, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, norm_layer=norm_layer)
            for i in range(depth)])
        self.overlap_attn = OCAB(dim=dim, input_resolution=input_resolution, window_size=window_size, overlap_ratio=overlap_ratio,
                                 num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, mlp_ratio=mlp_ratio,
                                 norm_layer=norm_layer)
        self.downsample = None

    def forward(self, x, x_size=None, params=None):
        for blk in self.blocks:
            x = blk(x)
        return self.overlap_attn(x)


class PatchEmbed(nn.Module):
    """hat.py:551-580: flatten (free in NHWC) and the optional LayerNorm."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        patches_resolution = [img_size[0] // patch_size[0], img_size[1] // patch_size[1]]
        self.img_size = img_size
        self.patch_size = patch_size
        self.patches_resolution = patches_resolution
        self.num_patches = patches_resolution[0] * patches_resolution[1]
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.norm = _norm(norm_layer, embed_dim) if norm_layer is not None else None

    def forward(self, x):
        return self.norm(x) if self.norm is not None else x


class PatchUnEmbed(nn.Module):
    """hat.py:582-598: the identity on NHWC tokens."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        patches_resolution = [img_size[0] // patch_size[0], img_size[1] // patch_size[1]]
        self.img_size = img_size
        self.patch_size = patch_size
        self.patches_resolution = patches_resolution
        self.num_patches = patches_resolution[0] * patches_resolution[1]
        self.in_chans = in_chans
        self.embed_dim = embed_dim

    def forward(self, x, x_size=None):
        return x


class RHAG(nn.Module):
    """hat.py:489-549: conv3x3(AttenBlocks(x)) + x (the residual in the conv's epilogue)."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, compress_ratio, squeeze_factor, conv_scale,
                 overlap_ratio, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False, img_size=224, patch_size=4, resi_connection='1conv'):
        super().__init__()
        _refuse(resi_connection != '1conv', "resi_connection='1conv' only")
        self.dim = dim
        self.input_resolution = input_resolution
        self.residual_group = AttenBlocks(dim=dim, input_resolution=input_resolution, depth=depth, num_heads=num_heads,
                                          window_size=window_size, compress_ratio=compress_ratio, squeeze_factor=squeeze_factor,
                                          conv_scale=conv_scale, overlap_ratio=overlap_ratio, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                          qk_scale=qk_scale, drop=drop, attn_drop=attn_drop, drop_path=drop_path,
                                          norm_layer=norm_layer, downsample=downsample, use_checkpoint=use_checkpoint)
        self.conv = HipConv2d(dim, dim, 3, 1, 1)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=0, embed_dim=dim, norm_layer=None)
        self.patch_unembed = PatchUnEmbed(img_size=img_size, patch_size=patch_size, in_chans=0, embed_dim=dim, norm_layer=None)

    def forward(self, x, x_size=None, params=None):
        return self.conv(self.residual_group(x), residual=x)


class Upsample(nn.Sequential):
    """hat.py:600-615: (conv 64 -> 64 r^2, pixel shuffle r) per stage, no activation; the stages are ONE module pair repeated, so
    their weights are tied and state_dict lists them under every stage index, as in the reference."""

    def __init__(self, upscale_factor):
        super().__init__()
        upsampling = []
        upsampling_two = [HipConv2d(64, 64 * 4, 3, 1, 1), _Shuffle(2)]
        upsampling_three = [HipConv2d(64, 64 * 9, 3, 1, 1), _Shuffle(3)]
        if (upscale_factor & (upscale_factor - 1)) == 0:
            for _ in range(int(math.log(upscale_factor, 2))):
                upsampling += upsampling_two
        elif upscale_factor % 3 == 0:
            for _ in range(int(math.log(upscale_factor, 3))):
                upsampling += upsampling_three
        self.upsampling = nn.Sequential(*upsampling)

    def forward(self, x):
        return self.upsampling(x)


class GeneratorResNet(nn.Module):
    """hat.py:617-875 with the same arguments and defaults.  The HIP path runs two families: embed_dim 96 with six heads of 16
    channels and windows of 8 or 9 (what the reference's trainer builds), and the published HAT / HAT-L (embed_dim 180) and HAT-S
    (embed_dim 144) with six heads, window 16 and overlap_ratio 0.5, at any depths, compress_ratio, squeeze_factor (1..16 hidden
    units) and mlp_ratio; any other width / heads / window combination, ape, dropout rates above 0, upsampler != 'pixelshuffle',
    resi_connection != '1conv', use_checkpoint and in_chans != 3 raise NotImplementedError."""

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6),
                 window_size=9, compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False,
                 patch_norm=True, use_checkpoint=False, upscale=2, img_range=1., upsampler='pixelshuffle', resi_connection='1conv',
                 **kwargs):
        super().__init__()
        _refuse(ape, 'absolute position embedding (ape)')
        _refuse(drop_rate > 0 or attn_drop_rate > 0, 'dropout rates above 0')
        _refuse(upsampler != 'pixelshuffle', "upsampler='pixelshuffle' only")
        _refuse(resi_connection != '1conv', "resi_connection='1conv' only")
        _refuse(use_checkpoint, 'use_checkpoint')
        _refuse(in_chans != 3, 'in_chans=3 only')
        _refuse(not _family_ok(embed_dim, window_size) or any(h != 6 for h in num_heads)
                or (embed_dim in WIDE_DIMS and int(window_size * overlap_ratio) != window_size // 2),
                'got embed_dim %d, num_heads %s, window_size %s; supported: %s' % (embed_dim, tuple(num_heads), window_size, FAMILIES))
        _refuse(qk_scale not in (None, (embed_dim // 6) ** -0.5), 'qk_scale None (head_dim ** -0.5)')
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.overlap_ratio = overlap_ratio
        num_in_ch = in_chans
        num_out_ch = in_chans
        num_feat = 64
        self.img_range = img_range
        self.mean = torch.Tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1)
        self.upscale = upscale
        self.upsampler = upsampler
        self.register_buffer('relative_position_index_SA', self.calculate_rpi_sa())
        self.register_buffer('relative_position_index_OCA', self.calculate_rpi_oca())
        self.conv_first = HipConv2d(num_in_ch, embed_dim, 3, 1, 1)
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.num_features = embed_dim
        self.mlp_ratio = mlp_ratio
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=embed_dim, embed_dim=embed_dim,
                                      norm_layer=norm_layer if self.patch_norm else None)
        patches_resolution = self.patch_embed.patches_resolution
        self.patches_resolution = patches_resolution
        self.patch_unembed = PatchUnEmbed(img_size=img_size, patch_size=patch_size, in_chans=embed_dim, embed_dim=embed_dim,
                                          norm_layer=norm_layer if self.patch_norm else None)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths), device='cpu')]   # (host values also under a meta default device)
        self.layers = nn.ModuleList()
        for i_layer in range(self.num_layers):
            self.layers.append(RHAG(
                dim=embed_dim, input_resolution=(patches_resolution[0], patches_resolution[1]), depth=depths[i_layer],
                num_heads=num_heads[i_layer], window_size=window_size, compress_ratio=compress_ratio, squeeze_factor=squeeze_factor,
                conv_scale=conv_scale, overlap_ratio=overlap_ratio, mlp_ratio=self.mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[sum(depths[:i_layer]):sum(depths[:i_layer + 1])],
                norm_layer=norm_layer, downsample=None, use_checkpoint=use_checkpoint, img_size=img_size, patch_size=patch_size,
                resi_connection=resi_connection))
        self.norm = _norm(norm_layer, self.num_features)
        self.conv_after_body = HipConv2d(embed_dim, embed_dim, 3, 1, 1)
        self.conv_before_upsample = nn.Sequential(HipConv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
        self.upsample = Upsample(upscale)
        self.conv_last = HipConv2d(num_feat, num_out_ch, 3, 1, 1)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @property
    def res_groups(self):
        """The RHAG modules in order (registers nothing: the state_dict is unchanged)."""
        return list(self.layers)

    @property
    def habs(self):
        """Every HAB in forward order (drop-path factors: last_drop_factors / replay_drop_factors)."""
        return [blk for layer in self.layers for blk in layer.residual_group.blocks]

    def calculate_rpi_sa(self):
        """hat.py:767-779."""
        coords_h = torch.arange(self.window_size)
        coords_w = torch.arange(self.window_size)
        coords = torch.stack(torch.meshgrid([coords_h, coords_w], indexing='ij'))
        coords_flatten = torch.flatten(coords, 1)
        relative_coords = coords_flatten[:, :, None] - coords_flatten[:, None, :]
        relative_coords = relative_coords.permute(1, 2, 0).contiguous()
        relative_coords[:, :, 0] += self.window_size - 1
        relative_coords[:, :, 1] += self.window_size - 1
        relative_coords[:, :, 0] *= 2 * self.window_size - 1
        return relative_coords.sum(-1)

    def calculate_rpi_oca(self):
        """hat.py:781-800 (holds negative indices: table[idx] wraps them)."""
        window_size_ori = self.window_size
        window_size_ext = self.window_size + int(self.overlap_ratio * self.window_size)
        coords_ori = torch.stack(torch.meshgrid([torch.arange(window_size_ori), torch.arange(window_size_ori)], indexing='ij'))
        coords_ori_flatten = torch.flatten(coords_ori, 1)
        coords_ext = torch.stack(torch.meshgrid([torch.arange(window_size_ext), torch.arange(window_size_ext)], indexing='ij'))
        coords_ext_flatten = torch.flatten(coords_ext, 1)
        relative_coords = coords_ext_flatten[:, None, :] - coords_ori_flatten[:, :, None]
        relative_coords = relative_coords.permute(1, 2, 0).contiguous()
        relative_coords[:, :, 0] += window_size_ori - window_size_ext + 1
        relative_coords[:, :, 1] += window_size_ori - window_size_ext + 1
        relative_coords[:, :, 0] *= window_size_ori + window_size_ext - 1
        return relative_coords.sum(-1)

    def calculate_mask(self, x_size):
        """hat.py:802-821: the SW-MSA mask (-100 across regions) for an h x w image (the kernels compute it from coordinates)."""
        h, w = x_size
        img_mask = torch.zeros((1, h, w, 1))
        slices = (slice(0, -self.window_size), slice(-self.window_size, -self.shift_size), slice(-self.shift_size, None))
        cnt = 0
        for hs in slices:
            for wsl in slices:
                img_mask[:, hs, wsl, :] = cnt
                cnt += 1
        ws = self.window_size
        mw = img_mask.view(1, h // ws, ws, w // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws)
        attn_mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        return attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))

    def no_weight_decay(self):
        return {'absolute_pos_embed'}

    def no_weight_decay_keywords(self):
        return {'relative_position_bias_table'}

    def check_image_size(self, x):
        _, _, h, w = x.size()
        mod_pad_h = (self.window_size - h % self.window_size) % self.window_size
        mod_pad_w = (self.window_size - w % self.window_size) % self.window_size
        if mod_pad_h or mod_pad_w:
            x = F.pad(x, (0, mod_pad_w, 0, mod_pad_h), 'reflect')
        return x

    def forward_features(self, x):
        x = self.patch_embed(x)
        for layer in self.layers:
            x = layer(x)
        return self.norm(x)

    def forward(self, x):
        x = self.check_image_size(x)
        mean = self.mean.to(device=x.device, dtype=x.dtype)
        x = ops.nhwc((x - mean) * self.img_range)
        x = self.conv_first(x)
        x = self.conv_after_body(self.forward_features(x), residual=x)
        x = self.conv_before_upsample[0](x, act_slope=self.conv_before_upsample[1].negative_slope)
        x = self.upsample(x)
        cl = self.conv_last
        if self.img_range == 1:
            return ops.conv2d(x, cl.weight, cl.bias + mean.view(3), 1, 1)   # conv_last(x) / 1 + mean
        return cl(x) / self.img_range + mean


def train_step(G, opt_G, lr_img, hr_img):
    """One generator iteration of hat.py:1058-1074: loss_G = L1(G(lr), hr), backward, opt_G.step().  The VGG features the
    reference computes never enter loss_G: they are skipped.  Raises ValueError when G's output and hr differ in shape (x9 with
    window 9: the 24 x 24 input is padded to 27 x 27).  Returns loss_G as a 0-d device tensor (no host sync)."""
    opt_G.zero_grad(set_to_none=True)
    gen_hr = G(lr_img)
    if tuple(gen_hr.shape) != tuple(hr_img.shape):
        raise ValueError('HAT train_step: output %s and target %s differ in shape' % (tuple(gen_hr.shape), tuple(hr_img.shape)))
    loss_G = ops.l1_mean(gen_hr, hr_img)
    loss_G.backward()
    opt_G.step()
    ops.bump_weight_epoch()
    return loss_G.detach()
