"""The reference's contrastive VGG19 losses on the device (model/loss.py:121-298): `Vgg19Taps` is its `Vgg19` (torchvision
vgg19.features[:30] cut into five slices, taps relu1_1 .. relu5_1) and `ContrastLoss`, `NContrastLoss`, `ContrastCosineLoss`,
`NContrastCosineLoss` keep its names, constructor and arithmetic: the super-resolved image is the anchor `a`, the ground truth the positive
`p`, one or several degraded images the negatives `n`; the anchor is pulled towards the positive and pushed from the negatives in the
five feature spaces, tap weights 1/32, 1/16, 1/8, 1/4, 1.

Structure here, weights from the user -- the precedent of FeatureExtractor.load_torchvision_vgg19 and LPIPS.load_torchvision_alexnet:
the pretrained VGG19 file is torchvision's to download, `load_torchvision_vgg19` takes its state dict.  Until it is loaded the module
holds a deterministic init and its numbers mean nothing.  The reference feeds the images unnormalised, and so does this.

The arithmetic (csrc/contrast.hip): ONE backbone forward over the stacked batch [a; p; n_1 .. n_N] through the ordinary conv kernels
(bias + ReLU epilogue) and the 2 x 2 max pools (the floor-mode pool where H or W is odd), per tap one distance pass that reads the anchor
once beside all its operands and leaves float64 partial sums, one finish launch that forms the scalar and the coefficients of the
backward on the device; the backward is one distance-gradient pass per tap and one backbone backward over the anchor's slice alone
(conv2d_dgrad with each tap's ReLU mask and distance gradient fused in).  No host synchronisation anywhere."""
import ctypes
import math

import torch
import torch.nn as nn

from . import _hip, ops
from .ops import _p, _stream

# torchvision.models.vgg19().features[:30]: index -> (cin, cout); ReLU follows each conv, MaxPool2d(2) sits at 4, 9, 18, 27
CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 16: (256, 256),
         19: (256, 512), 21: (512, 512), 23: (512, 512), 25: (512, 512), 28: (512, 512)}
POOLS = (4, 9, 18, 27)
SLICES = ((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))           # loss.py:130-139
TAPS = (0, 5, 10, 19, 28)                                        # the conv whose ReLU output ends each slice
CHANNELS = (64, 128, 256, 512, 512)
WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)            # loss.py:181
TEMPERATURE = 0.07                                               # loss.py:244
MIN_SIDE = 16                                                    # relu5_1 is 1 x 1
MAX_NEGATIVES = 8


def tap_sizes(h, w):
    """(h, w) of the five taps for an H x W image."""
    out = [(h, w)]
    for _ in range(4):
        h, w = h // 2, w // 2
        out.append((h, w))
    return out


# ---------------------------------------------------------------------- launch wrappers ------------ #
def max_pool2x2_floor_raw(x):
    """nn.MaxPool2d(2) for any H, W >= 2 (srhip_maxpool2x2_floor_fwd): an odd last row or column belongs to no window."""
    ops._require_gpu(x, 'max_pool2x2_floor')
    x = ops.nhwc(x)
    n, c, h, w = x.shape
    if h < 2 or w < 2 or c % 4:
        raise ValueError('max_pool2x2_floor: needs H, W >= 2 and C %% 4 == 0, got %s' % (tuple(x.shape),))
    y = ops.empty_nhwc(n, c, h // 2, w // 2, x)
    _hip.check(_hip.lib().srhip_maxpool2x2_floor_fwd(_p(x), _p(y), n, h, w, c, _stream()), 'maxpool2x2_floor_fwd')
    return y


def max_pool2x2_floor_bwd_raw(x, dy, relu=False, residual=None):
    """Backward of nn.MaxPool2d(2) in gather form (srhip_maxpool2x2_floor_bwd): dx = gather(dy) [* (x > 0)] [+ residual], x the pool's
    input.  The first maximum of a window takes its gradient, as in ATen; an odd last row or column gets none."""
    ops._require_gpu(x, 'max_pool2x2_floor_bwd')
    ops._require_gpu(dy, 'max_pool2x2_floor_bwd')
    x, dy = ops.nhwc(x), ops.nhwc(dy)
    n, c, h, w = x.shape
    if h < 2 or w < 2 or c % 4 or tuple(dy.shape) != (n, c, h // 2, w // 2):
        raise ValueError('max_pool2x2_floor_bwd: dy %s is not the pooled shape of x %s' % (tuple(dy.shape), tuple(x.shape)))
    if residual is not None:
        ops._require_gpu(residual, 'max_pool2x2_floor_bwd')
        residual = ops.nhwc(residual)
        if residual.shape != x.shape:
            raise ValueError('max_pool2x2_floor_bwd: residual %s must have the shape of x %s' % (tuple(residual.shape), tuple(x.shape)))
    dx = ops.empty_nhwc(n, c, h, w, x)
    _hip.check(_hip.lib().srhip_maxpool2x2_floor_bwd(_p(x), _p(dy), _p(residual), _p(dx), n, h, w, c, int(bool(relu)), _stream()),
               'maxpool2x2_floor_bwd')
    return dx


def _tap_dims(f, kops, what):
    ops._require_gpu(f, what)
    m, c, h, w = f.shape
    if not f.is_contiguous(memory_format=ops.CL) or not 1 <= kops <= MAX_NEGATIVES + 1 or m % (kops + 1) or c % 4:
        raise ValueError('%s: needs a dense NHWC tap of (1 + %d) * B images with C %% 4 == 0, got %s' % (what, kops, tuple(f.shape)))
    return m // (kops + 1), c, h, w


def _device_f64(t, numel, what):
    if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError('%s: needs a dense float64 device tensor of %d elements' % (what, numel))


def _upstream(t, what):
    if t.dtype != torch.float32 or not t.is_cuda or t.numel() != 1:
        raise ValueError('%s: upstream must be a float32 device scalar' % what)


def l1_parts():
    return _hip.lib().srhip_contrast_l1_parts()


def cos_parts():
    return _hip.lib().srhip_contrast_cos_parts()


def contrast_l1_fwd_raw(f, kops, partial):
    """One tap's L1 sums (srhip_contrast_l1_fwd).  f: [(1 + kops) B, C, h, w], the stacked [a; x_1 .. x_kops]; partial: float64
    [kops, l1_parts()] that receives the partial sums of |a - x_k|."""
    b, c, h, w = _tap_dims(f, kops, 'contrast_l1_fwd')
    _device_f64(partial, kops * l1_parts(), 'contrast_l1_fwd')
    _hip.check(_hip.lib().srhip_contrast_l1_fwd(_p(f), _p(partial), b, kops, h, w, c, _stream()), 'contrast_l1_fwd')
    return partial


def contrast_l1_bwd_raw(f, kops, coef, upstream):
    """da = upstream * (coef[0] sign(a - x_1) - sum_{k >= 1} coef[k] sign(a - x_{k+1})) through the tap's ReLU (srhip_contrast_l1_bwd).
    coef: float64 [kops] on the device; upstream: a float32 device scalar -> [B, C, h, w]."""
    b, c, h, w = _tap_dims(f, kops, 'contrast_l1_bwd')
    _device_f64(coef, kops, 'contrast_l1_bwd')
    _upstream(upstream, 'contrast_l1_bwd')
    da = ops.empty_nhwc(b, c, h, w, f)
    _hip.check(_hip.lib().srhip_contrast_l1_bwd(_p(f), _p(coef), _p(upstream), _p(da), b, kops, h, w, c, _stream()), 'contrast_l1_bwd')
    return da


def contrast_l1_finish_raw(partial, tap_counts, ablation):
    """partial: float64 [5, kops, l1_parts()]; tap_counts: the element count B C h w of each anchor tap -> (loss, coef): a 0-d float32
    tensor and float64 [5, kops], the (alpha, beta ..) of each tap's backward."""
    kops = partial.shape[1]
    _device_f64(partial, 5 * kops * l1_parts(), 'contrast_l1_finish')
    loss = torch.empty((), device=partial.device, dtype=torch.float32)
    coef = torch.empty(5, kops, device=partial.device, dtype=torch.float64)
    counts = (ctypes.c_long * 5)(*[int(v) for v in tap_counts])
    _hip.check(_hip.lib().srhip_contrast_l1_finish(_p(partial), counts, kops, int(bool(ablation)), _p(loss), _p(coef), _stream()),
               'contrast_l1_finish')
    return loss, coef


def contrast_cos_fwd_raw(f, kops, partial):
    """One tap's cosine sums (srhip_contrast_cos_fwd).  partial: float64 [B, kops, cos_parts()] that receives, per sample, the partial
    pixel sums of cos(a, x_k)."""
    b, c, h, w = _tap_dims(f, kops, 'contrast_cos_fwd')
    _device_f64(partial, b * kops * cos_parts(), 'contrast_cos_fwd')
    _hip.check(_hip.lib().srhip_contrast_cos_fwd(_p(f), _p(partial), b, kops, h, w, c, _stream()), 'contrast_cos_fwd')
    return partial


def contrast_cos_bwd_raw(f, kops, gamma, upstream):
    """da = upstream / (h w) * sum_k gamma[s, k] * d cos(a, x_k) / d a through the tap's ReLU (srhip_contrast_cos_bwd).  gamma: float64
    [B, kops] on the device -> [B, C, h, w]."""
    b, c, h, w = _tap_dims(f, kops, 'contrast_cos_bwd')
    _device_f64(gamma, b * kops, 'contrast_cos_bwd')
    _upstream(upstream, 'contrast_cos_bwd')
    da = ops.empty_nhwc(b, c, h, w, f)
    _hip.check(_hip.lib().srhip_contrast_cos_bwd(_p(f), _p(gamma), _p(upstream), _p(da), b, kops, h, w, c, _stream()), 'contrast_cos_bwd')
    return da


def contrast_cos_finish_raw(partial, tap_pixels, n_form, ablation):
    """partial: float64 [5, B, kops, cos_parts()]; tap_pixels: h w of each tap; n_form: NContrastCosineLoss's denominator -> (loss,
    gamma): a 0-d float32 tensor and float64 [5, B, kops], the coefficients of each tap's backward."""
    b, kops = partial.shape[1], partial.shape[2]
    _device_f64(partial, 5 * b * kops * cos_parts(), 'contrast_cos_finish')
    loss = torch.empty((), device=partial.device, dtype=torch.float32)
    gamma = torch.empty(5, b, kops, device=partial.device, dtype=torch.float64)
    terms = torch.empty(5 * b, device=partial.device, dtype=torch.float64)
    counts = (ctypes.c_long * 5)(*[int(v) for v in tap_pixels])
    _hip.check(_hip.lib().srhip_contrast_cos_finish(_p(partial), counts, b, kops, int(bool(n_form)), int(bool(ablation)), _p(loss),
                                                    _p(gamma), _p(terms), _stream()), 'contrast_cos_finish')
    return loss, gamma


# ---------------------------------------------------------------------- the backbone --------------- #
class _Conv(nn.Module):
    """Parameter holder with nn.Conv2d's names (weight OIHW, bias)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout), requires_grad=False)


def _even(x):
    return x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0


class Vgg19Taps(nn.Module):
    """The reference's `Vgg19` (loss.py:121-171): slice1 .. slice5 with torchvision's layer indices as names, so the state dict has its
    keys (`slice1.0`, `slice2.{2,5}`, `slice3.{7,10}`, `slice4.{12,14,16,19}`, `slice5.{21,23,25,28}`, each `.weight` and `.bias`);
    ReLUs and pools carry no keys.  Frozen."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)                       # deterministic init; real use loads the state dict
        for s, (lo, hi) in enumerate(SLICES):
            mods = nn.Module()
            for i in range(lo, hi):
                if i in CONVS:
                    conv = _Conv(*CONVS[i])
                    with torch.no_grad():
                        bound = math.sqrt(6.0 / (CONVS[i][0] * 9))
                        conv.weight.copy_((torch.rand(conv.weight.shape, generator=g) * 2 - 1) * bound)
                        conv.bias.zero_()
                    mods.add_module(str(i), conv)
            setattr(self, 'slice%d' % (s + 1), mods)
        ops.mark_static(self)
        self.eval()

    def conv(self, i):
        for s, (lo, hi) in enumerate(SLICES):
            if lo <= i < hi:
                return getattr(getattr(self, 'slice%d' % (s + 1)), str(i))
        raise KeyError(i)

    def load_torchvision_vgg19(self, state_dict):
        """torchvision VGG19 state dict: `features.N.{weight,bias}` of the 13 convs up to relu5_1 are taken, every other key is
        ignored."""
        named = {}
        for i in CONVS:
            for leaf in ('weight', 'bias'):
                key = 'features.%d.%s' % (i, leaf)
                if key not in state_dict:
                    raise KeyError('load_torchvision_vgg19: %s is missing' % key)
                param = getattr(self.conv(i), leaf)
                if tuple(state_dict[key].shape) != tuple(param.shape):
                    raise ValueError('load_torchvision_vgg19: %s has shape %s, expected %s'
                                     % (key, tuple(state_dict[key].shape), tuple(param.shape)))
                named[key] = (param, state_dict[key])
        with torch.no_grad():
            for param, value in named.values():
                param.copy_(value)                                 # bumps the version: packed images are rebuilt on next use
        return sorted(named)

    def forward(self, x, keep=None):
        """x: [M,3,H,W] on the device -> the five ReLU taps (no autograd: the losses below own the backward).  keep: a slice of the batch
        whose pool inputs are appended to `keep[1]` (the backward's saved tensors)."""
        ops._require_gpu(x, 'Vgg19Taps')
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('Vgg19Taps: images must be [M, 3, H, W], got %s' % (tuple(x.shape),))
        if min(x.shape[2:]) < MIN_SIDE:
            raise ValueError('Vgg19Taps: images must be at least %d x %d (relu5_1 is 1 x 1 there), got %d x %d'
                             % ((MIN_SIDE, MIN_SIDE) + tuple(x.shape[2:])))
        f, taps = ops.nhwc(x.detach()), []
        for i in range(SLICES[-1][1]):
            if i in CONVS:
                conv = self.conv(i)
                f = ops.conv2d_fwd_raw(f, conv.weight, conv.bias, 1, 1, slope=0.0)
                if i in TAPS:
                    taps.append(f)
                elif keep is not None:
                    keep[1].append(f[keep[0]])
            elif i in POOLS:
                f = ops.max_pool2x2_raw(f) if _even(f) else max_pool2x2_floor_raw(f)
        return taps


# ---------------------------------------------------------------------- the losses ----------------- #
class _Loss(torch.autograd.Function):
    """A contrastive loss as one autograd node, differentiable in the anchor alone."""

    @staticmethod
    def forward(ctx, a, stacked, model, kind, n_form, ablation, mode):
        b, kops = a.shape[0], stacked.shape[0] // a.shape[0] - 1
        inner = []                                    # the anchor's non-tap ReLU outputs, in layer order
        with ops.conv_math(mode):
            taps = model(stacked, keep=(slice(0, b), inner) if ctx.needs_input_grad[0] else None)
        dev = stacked.device
        if kind == 'l1':
            partial = torch.empty(5, kops, l1_parts(), device=dev, dtype=torch.float64)
            for t, f in enumerate(taps):
                contrast_l1_fwd_raw(f, kops, partial[t])
            loss, coef = contrast_l1_finish_raw(partial, [b * f.shape[1] * f.shape[2] * f.shape[3] for f in taps], ablation)
        else:
            partial = torch.empty(5, b, kops, cos_parts(), device=dev, dtype=torch.float64)
            for t, f in enumerate(taps):
                contrast_cos_fwd_raw(f, kops, partial[t])
            loss, coef = contrast_cos_finish_raw(partial, [f.shape[2] * f.shape[3] for f in taps], n_form, ablation)
        ctx.model, ctx.kind, ctx.mode, ctx.kops = model, kind, mode, kops
        ctx.taps, ctx.inner, ctx.coef, ctx.image_shape = taps, inner, coef, tuple(a.shape)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        model, taps, kops = ctx.model, ctx.taps, ctx.kops
        b = ctx.image_shape[0]
        grad = grad.detach().to(torch.float32).contiguous()
        bwd = contrast_l1_bwd_raw if ctx.kind == 'l1' else contrast_cos_bwd_raw
        hg = [bwd(f, kops, ctx.coef[t], grad) for t, f in enumerate(taps)]      # each arrives through its tap's ReLU
        ta = {i: f[:b] for i, f in zip(TAPS, taps)}                             # the anchor's taps, by conv index
        inner = dict(zip([i for i in CONVS if i not in TAPS], ctx.inner))       # the anchor's other ReLU outputs
        act = lambda i: ta[i] if i in ta else inner[i]
        order = sorted(CONVS)
        with ops.conv_math(ctx.mode):
            # walk down from relu5_1: g is the gradient at the OUTPUT of conv `i` (ReLU applied: the mask rides in whatever produced g)
            g = hg[4]
            for at in range(len(order) - 1, 0, -1):
                i, below = order[at], order[at - 1]
                x_in = act(below)                                               # the ReLU output that feeds conv i, before any pool
                pooled = (i - 1) in POOLS
                res = hg[TAPS.index(below)] if below in ta else None
                if not pooled:
                    g = ops.conv2d_dgrad_raw(g, model.conv(i).weight, tuple(x_in.shape), 1, 1, residual=res, actmask=x_in)
                else:                                                           # no tap feeds a pool: res is None here
                    ph, pw = x_in.shape[2] // 2, x_in.shape[3] // 2
                    g = ops.conv2d_dgrad_raw(g, model.conv(i).weight, (b, x_in.shape[1], ph, pw), 1, 1)
                    g = ops.max_pool2x2_bwd_raw(g, x_in, True) if _even(x_in) else max_pool2x2_floor_bwd_raw(x_in, g, relu=True)
            dx = ops.conv2d_dgrad_raw(g, model.conv(0).weight, ctx.image_shape, 1, 1)
        return dx, None, None, None, None, None, None


class _Contrast(nn.Module):
    """The shared implementation.  `kind`: 'l1' or 'cosine'; `many`: the negatives arrive as [B,N,3,H,W]."""
    kind, many = 'l1', False

    def __init__(self, ablation=False, vgg=None):
        super().__init__()
        self.vgg = Vgg19Taps() if vgg is None else vgg
        self.ab = bool(ablation)
        self.weights = list(WEIGHTS)
        self.T = TEMPERATURE

    def _check(self, a, p, n):
        name = type(self).__name__
        for t, what in ((a, 'a'), (p, 'p'), (n, 'n')):
            if not torch.is_tensor(t):
                raise ValueError('%s: %s must be a tensor' % (name, what))
        if p.requires_grad or n.requires_grad:
            raise ValueError('%s: the gradient goes to the anchor only; detach the positive and the negatives' % name)
        if a.dim() != 4 or a.shape[1] != 3 or p.shape != a.shape:
            raise ValueError('%s: a and p must be [B, 3, H, W] of one shape, got %s and %s' % (name, tuple(a.shape), tuple(p.shape)))
        if self.many:
            if n.dim() != 5 or n.shape[0] != a.shape[0] or tuple(n.shape[2:]) != tuple(a.shape[1:]) \
                    or not 1 <= n.shape[1] <= MAX_NEGATIVES:
                raise ValueError('%s: n must be [B, N, 3, H, W] with 1 <= N <= %d and the images of a, got %s'
                                 % (name, MAX_NEGATIVES, tuple(n.shape)))
        elif n.shape != a.shape:
            raise ValueError('%s: n must have the shape of a %s, got %s' % (name, tuple(a.shape), tuple(n.shape)))
        if min(a.shape[2:]) < MIN_SIDE:
            raise ValueError('%s: images must be at least %d x %d (relu5_1 is 1 x 1 there), got %d x %d'
                             % ((name, MIN_SIDE, MIN_SIDE) + tuple(a.shape[2:])))
        for t in (a, p, n):
            ops._require_gpu(t, name)

    def forward(self, a, p, n):
        """a, p: [B,3,H,W]; n: [B,3,H,W] (or [B,N,3,H,W] for the N* classes) -> a 0-d float32 tensor.  The gradient goes to `a` alone;
        under no_grad, or for an `a` without grad, only the forward runs.  Conv arithmetic follows ops.conv_math, 'half' mapped to
        'bf16x3'; the mode of the forward is the mode of the backward.

        The cosine forms restate F.cosine_similarity as the installed torch computes it: sum_c (a_c / max(|a|, 1e-8)) * (x_c /
        max(|x|, 1e-8)), each norm clamped on its own.  A zero-norm pixel therefore has cosine 0, and its gradient is x_c / (1e-8 max(|x|,
        1e-8)) -- finite, no 0 / 0 -- which the tap's ReLU mask then zeroes, because a ReLU output of zero norm is zero in every
        channel."""
        self._check(a, p, n)
        mode = ops.get_conv_math()
        mode = 'bf16x3' if mode == 'half' else mode
        negs = n.detach().transpose(0, 1).reshape((-1,) + tuple(a.shape[1:])) if self.many else n.detach()
        stacked = torch.cat([a.detach(), p.detach(), negs], 0)
        args = (self.vgg, self.kind, self.many, self.ab and not self.many, mode)     # the N* classes never read `ablation`
        if not (torch.is_grad_enabled() and a.requires_grad):
            with torch.no_grad():
                return _Loss.apply(a, stacked, *args)
        return _Loss.apply(a, stacked, *args)


class ContrastLoss(_Contrast):
    """loss.py:173-198: sum_t w_t * L1(a, p) / (L1(a, n) + 1e-7); ablation: sum_t w_t * L1(a, p)."""
    kind, many = 'l1', False


class NContrastLoss(_Contrast):
    """loss.py:200-232: sum_t w_t * L1(a, p) / (sum_j L1(a, n_j) + 1e-7).  The reference stores `ablation` and never reads it here; so
    does this."""
    kind, many = 'l1', True


class ContrastCosineLoss(_Contrast):
    """loss.py:234-263: with E_x = exp(mean_hw cos(a, x) / 0.07) per sample, mean_b sum_t w_t * -log(E_p / (E_n + 1e-7)); ablation:
    -log(E_p)."""
    kind, many = 'cosine', False


class NContrastCosineLoss(_Contrast):
    """loss.py:265-298: mean_b sum_t w_t * -log(E_p / (sum_j E_nj + E_p)).  The reference stores `ablation` and never reads it here; so
    does this."""
    kind, many = 'cosine', True


LOSSES = {('l1', False): ContrastLoss, ('l1', True): NContrastLoss, ('cosine', False): ContrastCosineLoss,
          ('cosine', True): NContrastCosineLoss}
