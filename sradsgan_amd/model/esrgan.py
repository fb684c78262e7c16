"""ESRGAN on the HIP kernels.  Mirrors SRADSGAN/model/architecture.py (RRDBNet, Discriminator_VGG_96 / 128 / 192 / 256,
VGGFeatureExtractor) and model/block.py (conv_block, ResidualDenseBlock_5C, RRDB, upconv_blcok, pixelshuffle_block) with the
reference's constructor signatures and state_dict keys, GANLoss of model/sradsgan.py:35-67 with its 'vanilla' and 'lsgan' criteria,
and one iteration of the training loop (:829-892, `self.gp` off) as `TrainStep`, driven by the `ESRGAN` trainer.

Execution differs from the reference's graph, exactly in fp32:
  * an RRDB is ONE autograd node (rrdb_step) on NDSRGAN's concat-free dense blocks: each ResidualDenseBlock_5C keeps its input and
    its four conv outputs in one [n, h, w, 192] buffer, `x5 * 0.2 + x` is written straight into channels 0:64 of the next block's
    buffer, and the RRDB's own `out * 0.2 + x` into the next RRDB's buffer -- no torch.cat, no leaky_relu, no ATen add;
  * the first conv writes into the first dense buffer, `x + LR_conv(trunk)` rides in LR_conv's epilogue, an upconv stage is one
    nearest-upsampling pass and a conv with its LeakyReLU fused;
  * the discriminators' flatten + Linear + LeakyReLU + Linear is csrc/esrgan.hip's head (srhip_dhead_*), which reads the NHWC
    features in the reference's NCHW flatten order by addressing; it is differentiable once, so no gradient penalty runs through it;
  * the GAN criteria, plain and relativistic, are one kernel each for value and gradients (srhip_gan_loss_fwd_bwd), float64 inside;
  * VGGFeatureExtractor's `(x - mean) / std` is one pass (srhip_input_norm_*); it cannot be folded into conv1_1, whose zero padding
    lives in the normalised space."""
import math
import re
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.autograd import Function

from .. import _hip
from .. import checkpoint as ckpt
from .. import ops
from .. import trainer as _trainer
from ..dp import ParamArena
from ..ops import _p, _stream
from .layers import HipBatchNorm2d, HipConv2d

SLOPE = 0.2
NF, GC, W = ops.DENSE_NF, ops.DENSE_NC, ops.DENSE_W
SCALES = (2, 3, 4, 8)
D_SIZES = (96, 128, 192, 256)


# ---------------------------------------------------------------------- RRDB ----------------------- #
class _RrdbStep(Function):
    """block.py:211-231: t1 = x + .2 c5_1, t2 = t1 + .2 c5_2, t3 = t2 + .2 c5_3 (each ResidualDenseBlock_5C's `x5.mul(0.2) + x`,
    product then add), out = x + .2 t3.  t1 and t2 land in channels 0:64 of the next dense block's buffer, t3 stays in registers of
    the pass that writes out, and out lands in the next RRDB's buffer when `chain`.  Backward: _DcrdbStep's without the fourth conv
    -- per dense block one srhip_scaled_res_bwd pass (conv5's gradient and the buffer's initial gradient), conv5's wgrad and
    accumulating dgrad, then per conv (last first) the strided LeakyReLU backward in place, wgrad and accumulating dgrad; the RRDB's
    own skip `+ x` joins in block 1's pass."""

    @staticmethod
    def forward(ctx, x, chain, *params):
        ops._require_gpu(x, 'rrdb_step')
        x, ldx = ops._rowld(x)
        n, _, h, w = x.shape
        rows = n * h * w
        s = ops.RES_SCALE
        bufs = [ops._adopt_or_fill(x, ldx, n, h, w)]
        out = None
        for k in range(3):
            buf = bufs[k]
            c5 = ops._dense_fwd(buf, params[10 * k:10 * k + 10], n, h, w, ops.LRELU_SLOPE)
            if k < 2:
                nxt = ops._dense_buffer(n, h, w, x)
                ops.scaled_res_raw(buf, W, c5, NF, None, 0, s, 0.0, nxt, W, None, 0, rows)
                bufs.append(nxt)
            else:
                out, ldo = ops._result_tensor(x, chain)
                ops.scaled_res_raw(buf, W, c5, NF, x, ldx, s, s, None, 0, out, ldo, rows)
        ctx.save_for_backward(*bufs, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dS):
        b1, b2, b3, *params = ctx.saved_tensors
        dS, lds = ops._rowld(dS)
        n, _, h, w = dS.shape
        s = ops.RES_SCALE
        dz, ldz = dS, lds
        per_block = [None, None, None]
        # (ka, kb): the factors the gradient at a block's result reaches its conv5 / its input with; block 3's result t3 enters
        # out through `.2 t3`, so both carry one more .2 there
        for k, buf, ka, kb in ((2, b3, s * s, s), (1, b2, s, 1.0), (0, b1, s, 1.0)):
            grads = []
            e, lde, kc = (dS, lds, 1.0) if k == 0 else (None, 0, 0.0)      # the RRDB's skip: out = x + ..
            dbuf = ops._dense_bwd(buf, params[10 * k:10 * k + 10], dz, ldz, e, lde, ka, kb, kc, n, h, w, ops.LRELU_SLOPE, grads)
            per_block[k] = grads
            dz, ldz = dbuf[:, :NF], W
        return (dz, None) + tuple(per_block[0] + per_block[1] + per_block[2])


def rrdb_step(x, params, chain=False):
    """One RRDB (block.py:211-231) for nf = 64, gc = 32.  params: its 30 tensors in state_dict order (RDB1..3, each conv1..5 weight,
    bias).  chain: the result is written into the next RRDB's dense buffer (the caller feeds it to another rrdb_step)."""
    if len(params) != 30:
        raise ValueError('rrdb_step: an RRDB has 30 tensors (3 dense blocks x 5 convs x weight, bias), got %d' % len(params))
    return _RrdbStep.apply(x, bool(chain), *params)


def _check_block(nc, gc, norm_type, act_type, mode, what):
    if nc != NF or gc != GC:
        raise NotImplementedError('%s: the HIP dense blocks run nf = 64, gc = 32 (what the [n, h, w, 192] dense buffer holds), got nf = '
                                  '%r, gc = %r' % (what, nc, gc))
    if norm_type is not None:
        raise NotImplementedError('%s: norm_type=%r is not built (ESRGAN removes the normalisation layers: norm_type=None)' % (what, norm_type))
    if act_type != 'leakyrelu':
        raise NotImplementedError("%s: act_type=%r is not built (the dense block kernels fuse LeakyReLU(0.2): act_type='leakyrelu')"
                                  % (what, act_type))
    if mode != 'CNA':
        raise NotImplementedError("%s: mode=%r is not built (conv -> activation, mode='CNA', is what the fused conv epilogues compute)"
                                  % (what, mode))


class ResidualDenseBlock_5C(nn.Module):
    """block.py:176-208; keys conv{1..5}.0.{weight,bias} (slot 1 of conv1..4 is the LeakyReLU, fused into the conv)."""

    def __init__(self, nc, kernel_size=3, gc=32, stride=1, bias=True, pad_type='zero', norm_type=None, act_type='leakyrelu', mode='CNA'):
        super().__init__()
        _check_block(nc, gc, norm_type, act_type, mode, 'ResidualDenseBlock_5C')
        if kernel_size != 3 or stride != 1 or not bias or pad_type != 'zero':
            raise NotImplementedError('ResidualDenseBlock_5C: 3x3 stride-1 zero-padded convs with bias only')
        for j in range(4):
            setattr(self, 'conv%d' % (j + 1), nn.Sequential(HipConv2d(nc + j * gc, gc, 3, 1, 1), nn.Identity()))
        self.conv5 = nn.Sequential(HipConv2d(nc + 4 * gc, nc, 3, 1, 1))

    def tensors(self):
        out = []
        for j in range(5):
            conv = getattr(self, 'conv%d' % (j + 1))[0]
            out += [conv.weight, conv.bias]
        return out

    def forward(self, x):
        return ops.dense_block(ops.nhwc(x), self.tensors())


class RRDB(nn.Module):
    """block.py:211-231."""

    def __init__(self, nc, kernel_size=3, gc=32, stride=1, bias=True, pad_type='zero', norm_type=None, act_type='leakyrelu', mode='CNA'):
        super().__init__()
        for j in (1, 2, 3):
            setattr(self, 'RDB%d' % j, ResidualDenseBlock_5C(nc, kernel_size, gc, stride, bias, pad_type, norm_type, act_type, mode))

    def tensors(self):
        return self.RDB1.tensors() + self.RDB2.tensors() + self.RDB3.tensors()

    def forward(self, x, chain=False):
        return rrdb_step(x, self.tensors(), chain)


class ShortcutBlock(nn.Module):
    """block.py:76-90: x + sub(x); RRDBNet evaluates the sum in the epilogue of sub's last conv."""

    def __init__(self, submodule):
        super().__init__()
        self.sub = submodule

    def forward(self, x):
        return x + self.sub(x)


class _Upsample(nn.Module):
    """The Sequential slot of nn.Upsample(scale_factor = r, mode = 'nearest') (block.py:259)."""

    def __init__(self, scale_factor):
        super().__init__()
        self.scale_factor = scale_factor

    def forward(self, x):
        return ops.upsample_nearest(x, self.scale_factor)


class _PixelShuffle(nn.Module):
    """The Sequential slot of nn.PixelShuffle(r) (block.py:248); the stage's LeakyReLU rides in the same pass."""

    def __init__(self, upscale_factor):
        super().__init__()
        self.upscale_factor = upscale_factor

    def forward(self, x, slope=None):
        return ops.pixel_shuffle_act(x, self.upscale_factor, slope)


class RRDBNet(nn.Module):
    """architecture.py:47-78.  Keys model.0 (first conv), model.1.sub.{i}.RDB{j}.conv{k}.0 (trunk), model.1.sub.{nb} (LR conv), then the
    upsampler and the two HR convs at the reference's Sequential indices (x4 upconv: model.3, model.6, model.8, model.10): the
    slots of nn.Upsample / nn.PixelShuffle and of the activations stay in the Sequential as parameter-free modules."""

    def __init__(self, in_nc, out_nc, nf, nb, gc=32, upscale=4, norm_type=None, act_type='leakyrelu', mode='CNA', upsample_mode='upconv'):
        super().__init__()
        _check_block(nf, gc, norm_type, act_type, mode, 'RRDBNet')
        if isinstance(nb, bool) or not isinstance(nb, int) or nb < 1:
            raise ValueError('RRDBNet: nb must be an integer >= 1, got %r' % (nb,))
        if upscale not in SCALES:
            raise NotImplementedError('RRDBNet: upscale must be one of %s, got %r (the reference builds int(log2(upscale))  x2 stages for '
                                      'anything but 3: upscale=9 would be an x8 network under an x9 name)' % (SCALES, upscale))
        if upsample_mode not in ('upconv', 'pixelshuffle'):
            raise NotImplementedError('upsample mode [{:s}] is not found'.format(str(upsample_mode)))
        self.nb, self.upscale = nb, upscale
        r, stages = (3, 1) if upscale == 3 else (2, int(math.log(upscale, 2)))
        layers = [HipConv2d(in_nc, nf, 3, 1, 1),
                  ShortcutBlock(nn.Sequential(*([RRDB(nf, 3, gc, 1, True, 'zero', norm_type, act_type, 'CNA') for _ in range(nb)]
                                                + [HipConv2d(nf, nf, 3, 1, 1)])))]
        self._plan = []                     # ('up', index) | ('conv', index, slope) | ('shuffle', index, slope), in forward order
        for _ in range(stages):
            if upsample_mode == 'upconv':
                self._plan += [('up', len(layers)), ('conv', len(layers) + 1, SLOPE)]
                layers += [_Upsample(r), HipConv2d(nf, nf, 3, 1, 1), nn.Identity()]
            else:
                self._plan += [('conv', len(layers), None), ('shuffle', len(layers) + 1, SLOPE)]
                layers += [HipConv2d(nf, nf * r * r, 3, 1, 1), _PixelShuffle(r), nn.Identity()]
        self._plan += [('conv', len(layers), SLOPE), ('conv', len(layers) + 2, None)]
        layers += [HipConv2d(nf, nf, 3, 1, 1), nn.Identity(), HipConv2d(nf, out_nc, 3, 1, 1)]
        self.model = nn.Sequential(*layers)

    @property
    def rrdbs(self):
        return list(self.model[1].sub)[:self.nb]

    def forward(self, x):
        m = self.model
        sub = m[1].sub
        fea = ops.conv2d_into_dense(ops.nhwc(x), m[0].weight, m[0].bias)       # written into channels 0:64 of the first dense buffer
        t = fea
        for k in range(self.nb):
            t = rrdb_step(t, sub[k].tensors(), chain=k < self.nb - 1)
        out = ops.conv2d_residual_strided(t, sub[self.nb].weight, sub[self.nb].bias, fea)      # fea + LR_conv(trunk), in the epilogue
        for step in self._plan:
            if step[0] == 'up':
                out = m[step[1]](out)
            elif step[0] == 'conv':
                out = m[step[1]](out, act_slope=step[2])
            else:
                out = m[step[1]](out, step[2])
        return out

    def load_state_dict(self, state_dict, strict=True):
        """Takes the reference's layout, the ESRGAN "new architecture" layout and BasicSR's (convert_state_dict); convs re-pack their
        weights afterwards."""
        result = super().load_state_dict(convert_state_dict(state_dict), strict=strict)
        ckpt._after_load(self)
        return result


# ---------------------------------------------------------------------- checkpoints ---------------- #
_NEW_ARCH = (('conv_first', 'model.0'), ('trunk_conv', 'model.1.sub.{nb}'), ('upconv1', 'model.3'), ('upconv2', 'model.6'),
             ('HRconv', 'model.8'), ('conv_last', 'model.10'))
_BASICSR = (('conv_first', 'model.0'), ('conv_body', 'model.1.sub.{nb}'), ('conv_up1', 'model.3'), ('conv_up2', 'model.6'),
            ('conv_hr', 'model.8'), ('conv_last', 'model.10'))
_TRUNK_NEW = re.compile(r'^RRDB_trunk\.(\d+)\.RDB([123])\.conv([1-5])\.(weight|bias)$')
_TRUNK_BASICSR = re.compile(r'^body\.(\d+)\.rdb([123])\.conv([1-5])\.(weight|bias)$')


def _convert(sd, trunk, named, what):
    blocks = [int(m.group(1)) for m in (trunk.match(k) for k in sd) if m]
    if not blocks:
        raise ValueError('convert_state_dict: the %s layout has no trunk keys' % what)
    nb = max(blocks) + 1
    fixed = {}
    for src, dst in named:
        for leaf in ('weight', 'bias'):
            fixed['%s.%s' % (src, leaf)] = '%s.%s' % (dst.format(nb=nb), leaf)
    out = OrderedDict()
    for k, v in sd.items():
        m = trunk.match(k)
        if m:
            out['model.1.sub.%s.RDB%s.conv%s.0.%s' % m.groups()] = v
        elif k in fixed:
            out[fixed[k]] = v
        else:
            raise ValueError('convert_state_dict: key %r does not belong to the %s layout' % (k, what))
    return out


def convert_state_dict(sd):
    """A generator state dict in the reference's key layout.  Recognised: the reference's own (`model.*`: returned as a copy of the
    mapping), the ESRGAN "new architecture" layout (conv_first, RRDB_trunk.{i}.RDB{j}.conv{k}, trunk_conv, upconv1, upconv2, HRconv,
    conv_last) and BasicSR's (conv_first, body.{i}.rdb{j}.conv{k}, conv_body, conv_up1, conv_up2, conv_hr, conv_last) -- the latter
    two are x4 upconv networks.  Tensors are not copied.  Anything else is a ValueError."""
    keys = list(sd.keys())
    if keys and all(k.startswith('model.') for k in keys):
        return OrderedDict(sd)
    if any(k.startswith('RRDB_trunk.') for k in keys):
        return _convert(sd, _TRUNK_NEW, _NEW_ARCH, 'ESRGAN new-architecture')
    if any(k.startswith('body.') for k in keys):
        return _convert(sd, _TRUNK_BASICSR, _BASICSR, 'BasicSR')
    raise ValueError("convert_state_dict: unknown key layout (first keys %r); known: the reference's `model.*`, ESRGAN's `RRDB_trunk.*`, "
                     "BasicSR's `body.*`" % (keys[:3],))


def interpolate_networks(sd_a, sd_b, alpha):
    """ESRGAN's network interpolation: (1 - alpha) a + alpha b per tensor (alpha = 0: a, 1: b).  Returns a new dict of new tensors."""
    if list(sd_a.keys()) != list(sd_b.keys()):
        raise ValueError('interpolate_networks: the two state dicts must have the same keys in the same order')
    out = OrderedDict()
    for k, a in sd_a.items():
        b = sd_b[k]
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError('interpolate_networks: %s has shapes %s and %s' % (k, tuple(a.shape), tuple(b.shape)))
        out[k] = (1 - alpha) * a + alpha * b
    return out


# ---------------------------------------------------------------------- discriminators ------------- #
class _DHead(Function):
    """classifier(x.view(B, -1)) (architecture.py:125-129) on csrc/esrgan.hip's head: Linear(C S S -> H), LeakyReLU(0.2), Linear(H -> 1)
    from the NHWC features and the NCHW-flattened weight as they are."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, slope):
        ops._require_gpu(x, 'dhead')
        x = ops.nhwc(x)
        bsz, c, s, s2 = x.shape
        hdim = w0.shape[0]
        if s != s2 or tuple(w0.shape) != (hdim, c * s * s) or tuple(b0.shape) != (hdim,) or tuple(w1.shape) != (1, hdim) \
                or tuple(b1.shape) != (1,):
            raise ValueError('dhead: features %s do not fit Linear%s -> Linear%s' % (tuple(x.shape), tuple(w0.shape), tuple(w1.shape)))
        w0c, b0c, w1c, b1c = (t.detach().contiguous() for t in (w0, b0, w1, b1))
        hidden = torch.empty(bsz, hdim, device=x.device, dtype=torch.float32)
        y = torch.empty(bsz, 1, device=x.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_dhead_fwd(_p(x), _p(w0c), _p(b0c), _p(w1c), _p(b1c), _p(hidden), _p(y), bsz, c, s, hdim, float(slope),
                                              _stream()), 'dhead_fwd')
        ctx.save_for_backward(x, hidden, w0, b0, w1, b1)
        ctx.slope = float(slope)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, hidden, w0, b0, w1, b1 = ctx.saved_tensors
        bsz, c, s, _ = x.shape
        hdim = w0.shape[0]
        want_p = any(ctx.needs_input_grad[1:5]) and not ops._skip_param_grads(w0, b0, w1, b1)
        want_x = ctx.needs_input_grad[0]
        if not (want_p or want_x):
            return None, None, None, None, None, None
        dev = x.device
        dz = torch.empty(bsz, hdim, device=dev, dtype=torch.float32)
        dx = ops.empty_nhwc(bsz, c, s, s, x) if want_x else None
        dw0 = db0 = dw1 = db1 = None
        if want_p:
            dw0, db0, dw1, db1 = (torch.empty(tuple(t.shape), device=dev, dtype=torch.float32) for t in (w0, b0, w1, b1))
        _hip.check(_hip.lib().srhip_dhead_bwd(_p(dy.contiguous()), _p(x), _p(hidden), _p(w0.detach().contiguous()),
                                              _p(w1.detach().contiguous()), _p(dz), _p(dx), _p(dw0), _p(db0), _p(dw1), _p(db1), bsz, c, s,
                                              hdim, ctx.slope, _stream()), 'dhead_bwd')
        return dx, dw0, db0, dw1, db1, None


def dhead(x, w0, b0, w1, b1, slope=SLOPE):
    """x: [B, C, S, S] features (NHWC memory) -> [B, 1] = Linear(w1, b1)(LeakyReLU(Linear(w0, b0)(x.view(B, -1)))), the view taken in
    NCHW order as the reference does.  Differentiable once."""
    return _DHead.apply(x, w0, b0, w1, b1, slope)


class _DiscriminatorVGG(nn.Module):
    """architecture.py:87-319: conv0 (3x3, LeakyReLU), then pairs of (4x4 stride 2) / (3x3) convs with BatchNorm and LeakyReLU(0.2),
    widths base_nf .. 8 base_nf, down to S x S, and the classifier Linear(512 S S -> 100), LeakyReLU(0.2), Linear(100 -> 1).  Keys
    features.{i}.* (BatchNorm buffers included) and classifier.{0,2}.*."""

    size = None          # the input side the class is built for
    n_convs = None       # 10 (96 / 128) or 12 (192 / 256)

    def __init__(self, in_nc, base_nf, norm_type='batch', act_type='leakyrelu', mode='CNA'):
        super().__init__()
        name = type(self).__name__
        if base_nf != 64:
            raise NotImplementedError('%s: base_nf = 64 only (the reference hard-codes the classifier input 512 * S * S), got %r'
                                      % (name, base_nf))
        if norm_type != 'batch' or act_type != 'leakyrelu' or mode != 'CNA':
            raise NotImplementedError("%s: norm_type='batch', act_type='leakyrelu', mode='CNA' is what the fused conv / BatchNorm "
                                      'kernels compute, got %r / %r / %r' % (name, norm_type, act_type, mode))
        widths = [(in_nc, base_nf), (base_nf, base_nf), (base_nf, 2 * base_nf), (2 * base_nf, 2 * base_nf),
                  (2 * base_nf, 4 * base_nf), (4 * base_nf, 4 * base_nf), (4 * base_nf, 8 * base_nf), (8 * base_nf, 8 * base_nf)]
        widths += [(8 * base_nf, 8 * base_nf)] * (self.n_convs - 8)
        layers, self._blocks = [], []
        for i, (cin, cout) in enumerate(widths):
            k, stride = (4, 2) if i % 2 else (3, 1)
            conv_at = len(layers)
            layers.append(HipConv2d(cin, cout, k, stride, 1))
            bn_at = None
            if i > 0:
                bn_at = len(layers)
                layers.append(HipBatchNorm2d(cout))
            layers.append(nn.Identity())                 # slot of LeakyReLU(0.2): fused into the conv / the BatchNorm pass
            self._blocks.append((conv_at, bn_at))
        self.features = nn.Sequential(*layers)
        self.side = self.size >> (self.n_convs // 2)
        self.classifier = nn.Sequential(nn.Linear(8 * base_nf * self.side * self.side, 100), nn.Identity(), nn.Linear(100, 1))

    def forward(self, x):
        if x.dim() != 4 or tuple(x.shape[2:]) != (self.size, self.size):
            raise ValueError('%s takes %d x %d images (its classifier is Linear(512 * %d * %d, 100)), got %s; the four classes are built '
                             'for %s' % (type(self).__name__, self.size, self.size, self.side, self.side, tuple(x.shape), D_SIZES))
        x, f = ops.nhwc(x), self.features
        for conv_at, bn_at in self._blocks:
            x = f[conv_at](x, act_slope=SLOPE) if bn_at is None else f[bn_at](f[conv_at](x), act_slope=SLOPE)
        c = self.classifier
        return dhead(x, c[0].weight, c[0].bias, c[2].weight, c[2].bias, SLOPE)


class Discriminator_VGG_96(_DiscriminatorVGG):
    size, n_convs = 96, 10


class Discriminator_VGG_128(_DiscriminatorVGG):
    size, n_convs = 128, 10


class Discriminator_VGG_192(_DiscriminatorVGG):
    size, n_convs = 192, 12


class Discriminator_VGG_256(_DiscriminatorVGG):
    size, n_convs = 256, 12


DISCRIMINATORS = {96: Discriminator_VGG_96, 128: Discriminator_VGG_128, 192: Discriminator_VGG_192, 256: Discriminator_VGG_256}


def discriminator_for(crop_size):
    if crop_size not in DISCRIMINATORS:
        raise ValueError('ESRGAN: no Discriminator_VGG_* for crop_size %r; the reference has them for %s' % (crop_size, D_SIZES))
    return DISCRIMINATORS[crop_size]


# ---------------------------------------------------------------------- GAN criteria --------------- #
GAN_MODES = {'vanilla': 0, 'lsgan': 1}        # SRHIP_GAN_* of include/sradsgan_hip.h
GAN_TYPES = ('vanilla', 'lsgan', 'wgan-gp')


class _GanLoss(Function):
    """mean_i f(a_i - [mean(b)], label) (srhip_gan_loss_fwd_bwd): the gradient goes to a and, in the relativistic form, to b through
    its mean."""

    @staticmethod
    def forward(ctx, a, b, mode, label, relativistic):
        ops._require_gpu(a, 'gan_loss')
        a = a.contiguous()
        if relativistic:
            ops._require_gpu(b, 'gan_loss')
            b = b.contiguous()
        else:
            b = None
        out = torch.empty((), device=a.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_gan_loss_fwd_bwd(_p(a), a.numel(), _p(b), b.numel() if b is not None else 0, mode, float(label),
                                                     int(relativistic), None, _p(out), None, None, _stream()), 'gan_loss (value)')
        ctx.save_for_backward(a, b)
        ctx.mode, ctx.label, ctx.relativistic = mode, float(label), relativistic
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        need_a = ctx.needs_input_grad[0]
        need_b = b is not None and ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return None, None, None, None, None
        da = torch.empty_like(a) if need_a else None
        db = torch.empty_like(b) if need_b else None
        gout = gout.detach().to(torch.float32).contiguous()
        _hip.check(_hip.lib().srhip_gan_loss_fwd_bwd(_p(a), a.numel(), _p(b), b.numel() if b is not None else 0, ctx.mode, ctx.label,
                                                     int(ctx.relativistic), _p(gout), None, _p(da), _p(db), _stream()),
                   'gan_loss (gradients)')
        return da, db, None, None, None


def _gan_type(gan_type):
    t = gan_type.lower()
    if t not in GAN_TYPES:
        raise NotImplementedError('GAN type [{:s}] is not found'.format(t))
    return t


def gan_loss(x, target_is_real, gan_type, real_label_val=1.0, fake_label_val=0.0):
    """GANLoss(gan_type)(x, target_is_real) (sradsgan.py:56-67): BCEWithLogitsLoss ('vanilla') or MSELoss ('lsgan') against a tensor
    filled with the label, mean-reduced -- the label is a scalar of the kernel, no tensor is filled; 'wgan-gp': -mean / +mean."""
    t = _gan_type(gan_type)
    if t == 'wgan-gp':
        m = ops.mean(x)
        return -m if target_is_real else m
    return _GanLoss.apply(x, None, GAN_MODES[t], real_label_val if target_is_real else fake_label_val, False)


def _relativistic(x, other, target_is_real, t, real_label_val, fake_label_val):
    """criterion(x - mean(other), target_is_real)"""
    if t == 'wgan-gp':
        m = ops.mean(x) - ops.mean(other)
        return -m if target_is_real else m
    return _GanLoss.apply(x, other, GAN_MODES[t], real_label_val if target_is_real else fake_label_val, True)


def ragan_pair_d(pred_real, pred_fake, gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0):
    """The discriminator's relativistic loss (sradsgan.py:871-873): (c(real - mean(fake), True) + c(fake - mean(real), False)) / 2."""
    t = _gan_type(gan_type)
    l_real = _relativistic(pred_real, pred_fake, True, t, real_label_val, fake_label_val)
    l_fake = _relativistic(pred_fake, pred_real, False, t, real_label_val, fake_label_val)
    return (l_real + l_fake) / 2


def ragan_pair_g(pred_real_detached, pred_fake, gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0):
    """The generator's relativistic loss (sradsgan.py:843-844): (c(real - mean(fake), False) + c(fake - mean(real), True)) / 2 with the
    real predictions detached: the gradient reaches pred_fake directly (second term) and through mean(pred_fake) (first term)."""
    t = _gan_type(gan_type)
    real = pred_real_detached.detach()
    l_real = _relativistic(real, pred_fake, False, t, real_label_val, fake_label_val)
    l_fake = _relativistic(pred_fake, real, True, t, real_label_val, fake_label_val)
    return (l_real + l_fake) / 2


class GANLoss(nn.Module):
    """sradsgan.py:35-67 with all three criteria ('vanilla', 'lsgan', 'wgan-gp')."""

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0):
        super().__init__()
        self.gan_type = _gan_type(gan_type)
        self.real_label_val, self.fake_label_val = real_label_val, fake_label_val

    def forward(self, input, target_is_real):
        return gan_loss(input, target_is_real, self.gan_type, self.real_label_val, self.fake_label_val)


# ---------------------------------------------------------------------- perceptual extractor ------- #
class _InputNorm(Function):
    @staticmethod
    def forward(ctx, x, mean, std):
        ops._require_gpu(x, 'input_norm')
        x = ops.nhwc(x)
        c = x.shape[1]
        if mean.numel() != c or std.numel() != c or c > 4:
            raise ValueError('input_norm: %d-channel images need %d means and deviations (at most 4 channels), got %d / %d'
                             % (c, c, mean.numel(), std.numel()))
        mean, std = mean.detach().reshape(-1).contiguous(), std.detach().reshape(-1).contiguous()
        y = torch.empty_like(x, memory_format=ops.CL)
        _hip.check(_hip.lib().srhip_input_norm_fwd(_p(x), _p(mean), _p(std), _p(y), x.numel(), c, _stream()), 'input_norm_fwd')
        ctx.save_for_backward(std)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (std,) = ctx.saved_tensors
        dy = ops.nhwc(dy)
        dx = torch.empty_like(dy, memory_format=ops.CL)
        _hip.check(_hip.lib().srhip_input_norm_bwd(_p(dy), _p(std), _p(dx), dy.numel(), dy.shape[1], _stream()), 'input_norm_bwd')
        return dx, None, None


def input_norm(x, mean, std):
    """(x - mean[c]) / std[c] per channel (architecture.py:354), one pass forward and one scale pass backward."""
    return _InputNorm.apply(x, mean, std)


# torchvision.models.vgg19().features[:35]: conv index -> (cin, cout); a ReLU follows every conv but the last; MaxPool2d(2) at POOLS
VGG_CONVS = OrderedDict([(0, (3, 64)), (2, (64, 64)), (5, (64, 128)), (7, (128, 128)), (10, (128, 256)), (12, (256, 256)),
                         (14, (256, 256)), (16, (256, 256)), (19, (256, 512)), (21, (512, 512)), (23, (512, 512)), (25, (512, 512)),
                         (28, (512, 512)), (30, (512, 512)), (32, (512, 512)), (34, (512, 512))])
VGG_POOLS = (4, 9, 18, 27)


class VGGFeatureExtractor(nn.Module):
    """architecture.py:328-356: VGG19 features[:35] -- conv5_4 before its ReLU, four 2 x 2 max pools -- behind the ImageNet input
    normalisation.  Buffers mean, std; keys features.{i}.{weight,bias}.  Nothing is downloaded: the weights come from
    `load_torchvision_vgg19` (a torchvision VGG19 state dict of the user's) or stay at whatever the caller initialises.  Frozen."""

    def __init__(self, feature_layer=34, use_bn=False, use_input_norm=True, device=torch.device('cpu')):
        super().__init__()
        if use_bn:
            raise NotImplementedError('VGGFeatureExtractor: use_bn=True (vgg19_bn) is not built; ESRGAN uses vgg19')
        if feature_layer != 34:
            raise NotImplementedError('VGGFeatureExtractor: feature_layer=34 (conv5_4 before its ReLU, ESRGAN\'s choice) only, got %r'
                                      % (feature_layer,))
        self.use_input_norm = use_input_norm
        if use_input_norm:
            self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1).to(device))
            self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1).to(device))
        self.features = nn.Sequential(*[HipConv2d(*VGG_CONVS[i], 3, 1, 1) if i in VGG_CONVS else nn.Identity()
                                        for i in range(feature_layer + 1)])
        for p in self.features.parameters():
            p.requires_grad_(False)

    def load_torchvision_vgg19(self, state_dict):
        """torchvision VGG19 state dict: `features.N.{weight,bias}` of the 16 convs are taken, every other key is ignored."""
        own = {k: v for k, v in state_dict.items() if k.startswith('features.') and int(k.split('.')[1]) in VGG_CONVS}
        for k, v in self.state_dict().items():
            if k.startswith('features.') and k not in own:
                raise KeyError('load_torchvision_vgg19: %s is missing' % k)
        result = self.load_state_dict(own, strict=False)
        ckpt._after_load(self)
        return result

    def forward(self, x):
        x = ops.nhwc(x)
        if self.use_input_norm:
            x = input_norm(x, self.mean, self.std)
        last = next(reversed(VGG_CONVS))
        for i, m in enumerate(self.features):
            if i in VGG_CONVS:
                x = m(x, act_slope=None if i == last else 0.0)          # conv + ReLU fused
            elif i in VGG_POOLS:
                x = ops.max_pool2x2(x)
        return x


# ---------------------------------------------------------------------- the step ------------------- #
class TrainStep:
    """One iteration of sradsgan.py:829-892 with `self.gp` off, for ESRGAN's networks:
        loss_G = weight_pixel c(gen, hr) + weight_content c(F(gen), F(hr)) + weight_gan loss_gan, Adam(G);
        loss_D by the relativistic (:868-873) or the plain (:876-878, real + fake unhalved) branch, Adam(D), optional clamp of D.
    The discriminator passes run in the reference's sequence -- G phase: D(gen_hr) with a graph, D(imgs_hr) without one (relativistic
    only); D phase: D(imgs_hr), D(gen_hr.detach()) -- so BatchNorm's running statistics advance as the reference's do.  D's weight
    gradients of loss_G, which the reference zeroes before the D step, are not computed.  Adam is the fused arena kernel; the clamp
    (clip_value, None = off) rides in D's.  Nothing synchronises with the host; the returned scalars are 0-d device tensors."""

    def __init__(self, generator, discriminator, feature_extractor, lr=2e-4, b1=0.9, b2=0.999, weight_pixel=1.0, weight_content=1e-2,
                 weight_gan=1e-3, gan_type='vanilla', relative=True, loss_Lp_norm='L1', clip_value=None, real_label_val=1.0,
                 fake_label_val=0.0, use_gp=False):
        if use_gp:
            raise NotImplementedError('esrgan.TrainStep: no gradient penalty runs through the Discriminator_VGG_* classes: their dense '
                                      'head (srhip_dhead_*) is differentiable once, and the penalty needs a double backward')
        if loss_Lp_norm not in ('L1', 'L2'):
            raise ValueError("esrgan.TrainStep: loss_Lp_norm must be 'L1' or 'L2', got %r" % (loss_Lp_norm,))
        self.gan_type = _gan_type(gan_type)
        self.G, self.D, self.F = generator, discriminator, feature_extractor
        self.relative = bool(relative)
        self._crit = ops.l1_mean if loss_Lp_norm == 'L1' else ops.mse_mean
        self.weight_pixel, self.weight_content, self.weight_gan = weight_pixel, weight_content, weight_gan
        self.real_label_val, self.fake_label_val = real_label_val, fake_label_val
        self.clip_value = clip_value
        self.lr_G = self.lr_D = lr
        self.b1, self.b2, self.eps = b1, b2, 1e-8
        self.arena_G, self.arena_D = ParamArena(self.G), ParamArena(self.D)
        self._d_params = list(self.arena_D.params)
        for p in self.F.parameters():
            p.requires_grad_(False)
        ops.mark_static(self.F)

    def _labels(self):
        return dict(gan_type=self.gan_type, real_label_val=self.real_label_val, fake_label_val=self.fake_label_val)

    def __call__(self, imgs_lr, imgs_hr, alpha=None, negatives=None):
        """alpha, negatives: accepted and unused (the trainer's loop passes the penalty's interpolation weights to every step)."""
        G, D, F = self.G, self.D, self.F
        # ------------------ generator (sradsgan.py:829-858) ------------------
        self.arena_G.zero_grad()
        gen_hr = G(imgs_lr)
        pixel = self._crit(gen_hr, imgs_hr)
        with torch.no_grad():
            real_features = F(imgs_hr)
        content = self._crit(F(gen_hr), real_features)
        if self.relative:
            pred_g_fake = D(gen_hr)
            with torch.no_grad():
                pred_d_real = D(imgs_hr)
            loss_gan = ragan_pair_g(pred_d_real, pred_g_fake, **self._labels())
        else:
            loss_gan = gan_loss(D(gen_hr), True, **self._labels())
        loss_G = self.weight_pixel * pixel + self.weight_content * content + self.weight_gan * loss_gan
        with ops.backward_scope(skip_params=self._d_params):
            loss_G.backward()
        self.arena_G.adam_step(self.lr_G, self.b1, self.b2, self.eps)
        ops.bump_weight_epoch()
        # ---------------- discriminator (sradsgan.py:865-892) ----------------
        self.arena_D.zero_grad()
        fake = gen_hr.detach()
        if self.relative:
            pred_d_real = D(imgs_hr)
            pred_d_fake = D(fake)
            loss_D = ragan_pair_d(pred_d_real, pred_d_fake, **self._labels())
        else:
            loss_real = gan_loss(D(imgs_hr), True, **self._labels())
            loss_fake = gan_loss(D(fake), False, **self._labels())
            loss_D = loss_real + loss_fake
        loss_D.backward()
        self.arena_D.adam_step(self.lr_D, self.b1, self.b2, self.eps, 1.0, float(self.clip_value) if self.clip_value else 0.0)
        ops.bump_weight_epoch()
        return dict(loss_G=loss_G.detach(), loss_D=loss_D.detach(), pixel=pixel.detach(), content=content.detach(),
                    loss_gan=loss_gan.detach())


# ---------------------------------------------------------------------- the trainer ---------------- #
def default_args(**overrides):
    """SRADSGAN's flags with ESRGAN's defaults: x4, HR crops of 128, 23 RRDBs, the relativistic vanilla criterion, no gradient penalty,
    no weight clamp, loss weights 1e-2 (pixel), 1 (content), 5e-3 (GAN) and lr 1e-4 as in the ESRGAN paper."""
    d = dict(model_name='ESRGAN', scale_factor=4, crop_size=128, hr_height=128, hr_width=128, test_crop_size=128, batch_size=16, nb=23,
             gan_type='vanilla', relativeGan=True, gp=False, clip_value=None, weight_pixel=1e-2, weight_content=1.0, weight_gan=5e-3,
             lr=1e-4, esrgan_vgg19=None)
    d.update(overrides)
    return _trainer.default_args(**d)


class ESRGAN(_trainer.SRADSGAN):
    """SRADSGAN's trainer (data, epoch loop, plateau control, checkpoint names, validation) around ESRGAN's networks and step:
    RRDBNet(3, 3, 64, args.nb, upscale=scale_factor), the Discriminator_VGG_* of args.crop_size, VGGFeatureExtractor (weights from
    args.esrgan_vgg19, a torchvision VGG19 state-dict file of the user's, or their init) and esrgan.TrainStep with args.gan_type
    (default 'vanilla'), args.relativeGan (default True), args.weight_pixel (default 1.0).  Validation lines of mfeNew_validate carry
    esrgan_* keys.  What the step has no recorded reference iteration for is refused."""

    eval_label = 'esrgan'

    def _check_loss_options(self):
        if getattr(self, 'weight_lpips', 0.0) > 0:
            raise NotImplementedError('ESRGAN: no LPIPS term in the generator loss (weight_lpips = 0); SRADSGAN and SRAGAN take '
                                      'args.weight_lpips')
        if getattr(self, 'weight_contrast', 0.0) > 0:
            raise NotImplementedError('ESRGAN: no contrastive term in the generator loss (weight_contrast = 0); SRADSGAN and SRAGAN take '
                                      'args.weight_contrast')

    def __init__(self, args, train_loader=None, test_loader=None):
        if getattr(args, 'd_norm_type', None) is not None or getattr(args, 'd_attention', False) or getattr(args, 'd_spectralnorm', False):
            raise NotImplementedError('ESRGAN trains against the Discriminator_VGG_* classes (BatchNorm, dense head); SRADSGAN takes '
                                      'args.d_norm_type / args.d_attention / args.d_spectralnorm')
        if getattr(args, 'gp', False):
            raise NotImplementedError('ESRGAN: gp=True is refused: the Discriminator_VGG_* dense head is differentiable once, and the '
                                      'gradient penalty needs a double backward through the discriminator')
        self.gan_type = _gan_type(getattr(args, 'gan_type', 'vanilla'))
        discriminator_for(args.crop_size)                         # ValueError before anything is built
        if args.scale_factor not in SCALES:
            raise NotImplementedError('ESRGAN: scale_factor must be one of %s, got %r' % (SCALES, args.scale_factor))
        if not hasattr(args, 'relativeGan'):
            args.relativeGan = True
        super().__init__(args, train_loader=train_loader, test_loader=test_loader)
        self.relative = bool(getattr(args, 'relativeGan', True))
        self.nb = getattr(args, 'nb', 23)
        self.weight_pixel = getattr(args, 'weight_pixel', 1.0)
        self.esrgan_vgg19 = getattr(args, 'esrgan_vgg19', None)

    def _new_generator(self):
        return RRDBNet(3, 3, 64, self.nb, upscale=self.scale_factor)

    def _new_discriminator(self):
        return discriminator_for(self.crop_size)(3, 64)

    def _new_feature_extractor(self):
        fx = VGGFeatureExtractor()
        if self.esrgan_vgg19:
            fx.load_torchvision_vgg19(torch.load(self.esrgan_vgg19, map_location='cpu'))
        return fx

    def _build(self):
        """trainer.SRADSGAN._build with ESRGAN's extractor and step (no data-parallel exchange: esrgan.TrainStep is single-GPU)."""
        if self.world > 1:
            raise NotImplementedError('ESRGAN: the step is single-GPU (no gradient exchange is wired into esrgan.TrainStep)')
        self.generator = self._new_generator()
        self.discriminator = self._new_discriminator()
        self.feature_extractor = self._new_feature_extractor()
        model_dir = self.save_dir + '/model'
        if self.epoch != 0:
            self.load_epoch_network(model_dir + '/generator_param_epoch_%d.pkl' % self.epoch, self.generator, strict=True)
            self.load_epoch_network(model_dir + '/discriminator_param_epoch_%d.pkl' % self.epoch, self.discriminator, strict=True)
        else:
            self.generator.apply(_trainer.weights_init_normal)
            self.discriminator.apply(_trainer.weights_init_normal)
            self.chain_report = {}
            for label, net in (('generator', self.generator), ('discriminator', self.discriminator)):
                path = getattr(self, 'pretrained_' + label, None)
                if path:
                    sd = torch.load(path, map_location='cpu')
                    self.chain_report[label] = ckpt.load_compatible(net, convert_state_dict(sd) if label == 'generator' else sd)
        self.generator.to(self.device), self.discriminator.to(self.device), self.feature_extractor.to(self.device)
        self.feature_extractor.eval()
        self.step = TrainStep(self.generator, self.discriminator, self.feature_extractor, lr=self.lr, b1=self.b1, b2=self.b2,
                              weight_pixel=self.weight_pixel, weight_content=self.weight_content, weight_gan=self.weight_gan,
                              gan_type=self.gan_type, relative=self.relative, loss_Lp_norm=self.loss_Lp_norm,
                              clip_value=self.clip_value)
