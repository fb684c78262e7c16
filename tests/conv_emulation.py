"""fp64 emulation of what the HIP conv kernels compute, and an element-wise checker sized to it.

The kernels round their operands to 16 bits (or split them into two bf16 halves) and then accumulate exact products in
fp32.  Comparing a kernel with an fp64 conv of the UNROUNDED operands therefore needs a bar the size of the operand
rounding (~2^-8 .. 2^-16 of the output), far above what a dropped tap or a wrong packed section moves.  Here the operands
are rounded exactly as the kernel rounds them (conv_dev.h split_bf16x8 / round16x8, conv_internal.h fast_pack_store,
conv_wgrad_flat.hip convert) and the contraction is done in fp64: what is left between the kernel and this reference is
fp32 accumulation and the fp32 epilogue, i.e. a small multiple of 2^-24 of the conv of the absolute values.

Arithmetics (ops.set_conv_math mode -> what one multiply a * b is):
  'fp32'    a * b                                   fp32 MFMA / VALU kernels, every mode's exact-fp32 fallbacks
  'bf16x3'  ah*bh + ah*bl + al*bh                   ah = bf16(a), al = bf16(a - ah); the al*bl term is dropped
  'bf16'    bf16(a) * bf16(b)                       'half' mode on gradient data (dgrad, wgrad, GRADDATA forward)
  'fp16'    fp16(a) * fp16(b)                       'half' mode on activations (forward)
All roundings are to nearest even.  Everything works on CPU or GPU tensors (the GPU tests keep it on the device).
"""
import torch
import torch.nn.functional as F

ARITHS = ('fp32', 'bf16x3', 'bf16', 'fp16')
U24 = 2.0 ** -24


def round_bf16(t):
    """fp32 values -> nearest-even bf16, returned as float64 (bit arithmetic on the fp32 pattern; finite inputs)."""
    u = t.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF     # the unsigned fp32 pattern
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return r.view(torch.float32).double()


def round_fp16(t, flush_subnormals=False):
    """fp32 values -> nearest-even fp16 (gradual underflow unless flush_subnormals), returned as float64."""
    h = t.float().half().double()
    if flush_subnormals:
        h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
    return h


def split_bf16(t):
    """(hi, lo) of the split-bf16 operand: hi = bf16(v), lo = bf16(v - hi) (v - hi is exact in fp32)."""
    hi = round_bf16(t)
    lo = round_bf16((t.double() - hi).float())
    return hi, lo


def operand_terms(a, b, arith, flush_fp16=False):
    """[(a_i, b_i)] whose summed contractions are the kernel's contraction of a with b."""
    if arith == 'fp32':
        return [(a.double(), b.double())]
    if arith == 'bf16x3':
        ah, al = split_bf16(a)
        bh, bl = split_bf16(b)
        return [(ah, bh), (ah, bl), (al, bh)]
    if arith == 'bf16':
        return [(round_bf16(a), round_bf16(b))]
    if arith == 'fp16':
        return [(round_fp16(a, flush_fp16), round_fp16(b, flush_fp16))]
    raise ValueError('unknown arithmetic %r' % (arith,))


# ---- fp64 contractions (unfold + matmul: F.conv2d in double is not served everywhere) ------------------------------- #
def _chunks(n, per):
    return [(i, min(n, i + per)) for i in range(0, n, per)]


def _fwd64(x, w, stride, pad, dil):
    n, c, h, wd = x.shape
    co, _, kh, kw = w.shape
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (wd + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    wm = w.reshape(co, -1)
    per = max(1, int(2 ** 27 // max(1, c * kh * kw * ho * wo)))
    out = []
    for a, b in _chunks(n, per):
        cols = F.unfold(x[a:b], (kh, kw), dilation=dil, padding=pad, stride=stride)
        out.append((wm @ cols).reshape(b - a, co, ho, wo))
    return torch.cat(out)


def _dgrad64(dy, w, x_shape, stride, pad, dil):
    n, c, h, wd = x_shape
    co, _, kh, kw = w.shape
    wt = w.reshape(co, -1).t()
    per = max(1, int(2 ** 27 // max(1, c * kh * kw * dy.shape[2] * dy.shape[3])))
    out = []
    for a, b in _chunks(n, per):
        cols = wt @ dy[a:b].reshape(b - a, co, -1)
        out.append(F.fold(cols, (h, wd), (kh, kw), dilation=dil, padding=pad, stride=stride))
    return torch.cat(out)


def _wgrad64(x, dy, w_shape, stride, pad, dil):
    co, c, kh, kw = w_shape
    n = x.shape[0]
    per = max(1, int(2 ** 27 // max(1, c * kh * kw * dy.shape[2] * dy.shape[3])))
    acc = None
    for a, b in _chunks(n, per):
        cols = F.unfold(x[a:b], (kh, kw), dilation=dil, padding=pad, stride=stride)
        part = torch.einsum('nol,nkl->ok', dy[a:b].reshape(b - a, co, -1), cols)
        acc = part if acc is None else acc + part
    return acc.reshape(co, c, kh, kw)


def conv_fwd(x, w, stride=1, pad=0, arith='fp32', dil=1, flush_fp16=False, with_abs=True):
    """(ref, absref) of y = conv2d(x, w) as the kernel computes it; x may already carry an operand scale (chanscale).
    absref is the same conv of |x| and |w| (None when with_abs is False)."""
    ref = sum(_fwd64(a, b, stride, pad, dil) for a, b in operand_terms(x, w, arith, flush_fp16))
    return ref, _fwd64(x.double().abs(), w.double().abs(), stride, pad, dil) if with_abs else None


def conv_dgrad(dy, w, x_shape, stride=1, pad=0, arith='fp32', dil=1, with_abs=True):
    """(ref, absref) of dx = conv_transpose2d(dy, w) as the kernel computes it."""
    ref = sum(_dgrad64(a, b, x_shape, stride, pad, dil) for a, b in operand_terms(dy, w, arith))
    return ref, _dgrad64(dy.double().abs(), w.double().abs(), x_shape, stride, pad, dil) if with_abs else None


def conv_wgrad(x, dy, w_shape, stride=1, pad=0, arith='fp32', dil=1, with_abs=True):
    """(ref, absref) of dw = the weight gradient of conv2d(x, w) for the output gradient dy."""
    ref = sum(_wgrad64(a, b, w_shape, stride, pad, dil) for a, b in operand_terms(x, dy, arith))
    return ref, _wgrad64(x.double().abs(), dy.double().abs(), w_shape, stride, pad, dil) if with_abs else None


def epilogue(ref, absref, rowscale=None, bias=None, slope=None, actmask=None, mask_slope=None, residual=None, prev=None):
    """The kernels' fp32 epilogue, in fp64 and in their order: *rowscale, +bias, LeakyReLU(slope), * (actmask > 0 ? 1 : mask_slope),
    +residual, +prev (the accumulate destination's previous contents).
    The abs reference grows by every added term (the epilogue's own roundings are relative to those)."""
    ref, absref = ref.clone(), absref.clone()
    if rowscale is not None:
        rs = rowscale.double()
        ref, absref = ref * rs, absref * rs.abs()
    if bias is not None:
        b = bias.double().view(1, -1, 1, 1)
        ref, absref = ref + b, absref + b.abs()
    if slope is not None:
        ref = torch.where(ref > 0, ref, ref * slope)
    if actmask is not None:
        ref = torch.where(actmask.double() > 0, ref, ref * mask_slope)
    for t in (residual, prev):
        if t is not None:
            ref, absref = ref + t.double(), absref + t.double().abs()
    return ref, absref


# ---- the checker ---------------------------------------------------------------------------------------------------- #
def bound(ref, absref, tau, floor=1e-37):
    return tau * absref + 2 * U24 * ref.abs() + floor


def l2_dist(got, ref):
    return float((got.detach().to(ref.device).double() - ref).norm())


def worst(got, ref, absref, tau, floor=1e-37):
    """(largest |got - ref| / bound, (image, channel, row, col) of that element, its values)."""
    got = got.detach().to(ref.device).double()
    r = (got - ref).abs() / bound(ref, absref, tau, floor)
    r = torch.nan_to_num(r, nan=float('inf'))
    flat = int(torch.argmax(r))
    idx = []
    for s in reversed(ref.shape):
        idx.append(flat % s)
        flat //= s
    idx = tuple(reversed(idx))
    return float(r[idx]), idx, (float(got[idx]), float(ref[idx]), float(absref[idx]))


def assert_conv_close(got, ref, absref, tau, floor=1e-37, what='conv'):
    """|got - ref| <= tau * absref + 2 * 2^-24 * |ref| + floor element by element; returns the largest err / bound."""
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, tuple(got.shape), tuple(ref.shape))
    ratio, idx, (g, e, a) = worst(got, ref, absref, tau, floor)
    if not ratio <= 1.0:
        where = ('image %d, channel %d, pixel (%d, %d)' % idx) if len(idx) == 4 else 'element %s' % (idx,)
        raise AssertionError('%s: %s: got %.9g, expected %.9g (abs ref %.4g): err / bound = %.3g (tau = %.3g * 2^-24)'
                             % (what, where, g, e, a, ratio, tau / U24))
    return ratio
