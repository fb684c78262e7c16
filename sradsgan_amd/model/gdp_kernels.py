"""The kernels of csrc/diffusion.hip as torch calls: every ctypes call into that file is made here, once, for the sampler
(model/gdp.py) and the trainer (model/gdp_train.py) alike.  Exact fp32, no atomics.

  group_norm_act / silu / avg_pool2x2 / qkv_attention   autograd Functions: differentiable when grad is enabled and an input requires it,
                     a plain launch of the same forward kernel otherwise (no graph, nothing kept).
  group_norm_fwd_raw / group_norm_bwd_raw / avg_pool2x2_bwd / attention_fwd_lse / attention_bwd_raw   the launches alone.
  randn_rows / sampler_step / q_sample_rows / quantize_u8   the sampler's and q_sample's row kernels; no gradient passes through them."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _hip, ops
from ..ops import _p, _stream

GROUPS = 32


def _rows(t, what):
    """(t, row stride) of a float32 device tensor [..., rows, C] whose channels are adjacent and whose rows lie `ld >= C` apart (a channel
    slice of a wider row buffer, or a dense one)."""
    ops._require_gpu(t, what)
    if t.dim() < 2 or t.stride(-1) != 1:
        raise ValueError('%s: channels must be the innermost, adjacent dimension, got strides %s' % (what, t.stride()))
    ld = t.stride(-2) if t.shape[-2] > 1 else max(t.stride(-2), t.shape[-1])
    step = ld
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] > 1 and t.stride(d) != step:
            raise ValueError('%s: rows must lie one row stride apart, got shape %s strides %s' % (what, tuple(t.shape), t.stride()))
        step *= t.shape[d]
    if ld < t.shape[-1]:
        raise ValueError('%s: row stride %d < %d channels' % (what, ld, t.shape[-1]))
    return t, ld


# ------------------------------------------------------------------------------------------------------------------------------ #
# GroupNorm(32) + scale-shift + SiLU
# ------------------------------------------------------------------------------------------------------------------------------ #
def group_norm_fwd_raw(x, weight, bias, mod, silu, eps=1e-5):
    """(y dense [n, p, C], statistics [n, 32, 2] = mean | 1 / sigma as the forward kernel leaves them in its workspace) of x [n, p, C]
    (row stride >= C) with mod [n, 2 C] = scale | shift or None."""
    x, ldx = _rows(x, 'group_norm_act')
    if x.dim() != 3:
        raise ValueError('group_norm_act: x must be [n, p, C], got %s' % (tuple(x.shape),))
    n, p, c = x.shape
    scale = shift = None
    if mod is not None:
        if tuple(mod.shape) != (n, 2 * c) or not mod.is_contiguous():
            raise ValueError('group_norm_act: scale | shift must be a dense [n, 2 C] = %s, got %s' % ((n, 2 * c), tuple(mod.shape)))
        scale, shift = mod[:, :c], mod[:, c:]
    y = torch.empty(n, p, c, device=x.device, dtype=torch.float32)
    lib = _hip.lib()
    ws = torch.empty(max(1, lib.srhip_diff_gn_workspace(n, p) // 4), device=x.device, dtype=torch.float32)
    _hip.check(lib.srhip_diff_gn_fwd(_p(x), ldx, _p(weight), _p(bias), _p(scale), _p(shift), 2 * c, _p(y), c, _p(ws), ws.numel() * 4,
                                     n, p, c, float(eps), int(bool(silu)), _stream()), 'diff_gn_fwd')
    off = lib.srhip_diff_gn_stats_offset(n, p) // 4
    return y, ws[off:off + n * GROUPS * 2].view(n, GROUPS, 2)


def group_norm_bwd_raw(dy, x, stats, weight, bias, mod, silu, out=None):
    """(dx [n, p, C], dgamma, dbeta, dmod [n, 2 C] or None) from dy [n, p, C] and the forward's x and statistics.  dy may be a channel
    slice of a wider row buffer (any other layout is copied dense); dx is dense, or `out` ([n, p, C], row stride >= C)."""
    x, ldx = _rows(x, 'group_norm_act backward')
    n, p, c = x.shape
    try:
        dy, lddy = _rows(dy, 'group_norm_act backward')
    except ValueError:                                   # e.g. an NCHW-dense gradient seen through the token view
        dy, lddy = dy.contiguous(), c
    if tuple(dy.shape) != (n, p, c):
        raise ValueError('group_norm_act backward: dy %s does not match x %s' % (tuple(dy.shape), (n, p, c)))
    if out is None:
        dx, lddx = torch.empty(n, p, c, device=x.device, dtype=torch.float32), c
    else:
        dx, lddx = _rows(out, 'group_norm_act backward')
        if tuple(dx.shape) != (n, p, c):
            raise ValueError('group_norm_act backward: out %s does not match x %s' % (tuple(dx.shape), (n, p, c)))
    dgamma, dbeta = torch.empty_like(weight), torch.empty_like(bias)
    scale = shift = dmod = dscale = dshift = None
    if mod is not None:
        scale, shift = mod[:, :c], mod[:, c:]
        dmod = torch.empty_like(mod)
        dscale, dshift = dmod[:, :c], dmod[:, c:]
    lib = _hip.lib()
    ws = torch.empty(max(1, lib.srhip_diff_gn_bwd_workspace(n, p, c) // 4), device=x.device, dtype=torch.float32)
    _hip.check(lib.srhip_diff_gn_bwd(_p(dy), lddy, _p(x), ldx, _p(stats), _p(weight), _p(bias), _p(scale), _p(shift), 2 * c, _p(dx), lddx,
                                     _p(dgamma), _p(dbeta), _p(dscale), _p(dshift), 2 * c, _p(ws), ws.numel() * 4, n, p, c,
                                     int(bool(silu)), _stream()), 'diff_gn_bwd')
    return dx, dgamma, dbeta, dmod


class _GroupNormAct(Function):
    """x [n, p, C] (row stride >= C), mod [n, 2 C] = scale | shift or None -> dense [n, p, C]."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, silu, eps):
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        mod = mod.contiguous() if mod is not None else None
        y, stats = group_norm_fwd_raw(x, weight, bias, mod, silu, eps)
        ctx.save_for_backward(x, weight, bias, mod, stats)
        ctx.silu = bool(silu)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, bias, mod, stats = ctx.saved_tensors
        return group_norm_bwd_raw(dy, x, stats, weight, bias, mod, ctx.silu) + (None, None)


def _one_row(scale, shift):
    """The [n, 2 C] tensor whose halves `scale` and `shift` are (the same memory, no copy), or None when they are not the two halves of
    one dense row.  Halves that carry a gradient are left to torch.cat: autograd has to see both of them."""
    n, c = scale.shape
    if torch.is_grad_enabled() and (scale.requires_grad or shift.requires_grad):
        return None
    halves = scale.dtype == shift.dtype and scale.untyped_storage().data_ptr() == shift.untyped_storage().data_ptr() \
        and shift.data_ptr() == scale.data_ptr() + c * scale.element_size()
    if not halves or any(t.stride(1) != 1 or (n > 1 and t.stride(0) != 2 * c) for t in (scale, shift)):
        return None
    return scale.as_strided((n, 2 * c), (2 * c, 1))


def group_norm_act(x, weight, bias, scale=None, shift=None, silu=False, eps=1e-5, mod=None):
    """nn.GroupNorm(32, C) over x [n, p, C] (rows may be a channel slice: row stride >= C), then y * (1 + scale) + shift, then SiLU if
    asked; a dense [n, p, C] tensor, differentiable in x, weight, bias and the modulation.  The modulation is `mod` [n, 2 C] =
    scale | shift (the emb_layers row as it stands) or `scale` and `shift` [n, C]: the two halves of one such row reach the kernel
    as they lie, anything else is concatenated first."""
    if (scale is None) != (shift is None):
        raise ValueError('group_norm_act: scale and shift come together')
    if scale is not None:
        if scale.dim() != 2 or tuple(shift.shape) != tuple(scale.shape):
            raise ValueError('group_norm_act: scale and shift must both be [n, C], got %s and %s' % (tuple(scale.shape), tuple(shift.shape)))
        mod = _one_row(scale, shift)
        if mod is None:
            mod = torch.cat([scale, shift], dim=1)
    return _GroupNormAct.apply(x, weight, bias, mod, silu, eps)


# ------------------------------------------------------------------------------------------------------------------------------ #
# SiLU, the 2 x 2 average pool
# ------------------------------------------------------------------------------------------------------------------------------ #
class _SiLU(Function):
    @staticmethod
    def forward(ctx, x):
        ops._require_gpu(x, 'silu')
        x = x.contiguous()
        y = torch.empty_like(x)
        _hip.check(_hip.lib().srhip_diff_silu_fwd(_p(x), _p(y), x.numel(), _stream()), 'diff_silu_fwd')
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _hip.check(_hip.lib().srhip_diff_silu_bwd(_p(dy), _p(x), _p(dx), x.numel(), _stream()), 'diff_silu_bwd')
        return dx


def silu(x):
    return _SiLU.apply(x)


class _AvgPool2x2(Function):
    @staticmethod
    def forward(ctx, x):
        ops._require_gpu(x, 'avg_pool2x2')
        x = ops.nhwc(x)
        n, c, h, w = x.shape
        y = ops.empty_nhwc(n, c, h // 2, w // 2, x)
        _hip.check(_hip.lib().srhip_diff_avgpool2x2_fwd(_p(x), _p(y), n, h, w, c, _stream()), 'diff_avgpool2x2_fwd')
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return avg_pool2x2_bwd(dy, ctx.shape)


def avg_pool2x2(x):
    """nn.AvgPool2d(2) of a logical [n, C, h, w] tensor (NHWC memory); h and w must be even."""
    return _AvgPool2x2.apply(x)


def avg_pool2x2_bwd(dy, shape):
    """The pool's backward alone: dy [n, C, h / 2, w / 2] -> dx of `shape` = [n, C, h, w] (NHWC memory)."""
    ops._require_gpu(dy, 'avg_pool2x2_bwd')
    n, c, h, w = shape
    dy = ops.nhwc(dy)
    if tuple(dy.shape) != (n, c, h // 2, w // 2):
        raise ValueError('avg_pool2x2_bwd: dy %s does not belong to an input of %s' % (tuple(dy.shape), tuple(shape)))
    dx = ops.empty_nhwc(n, c, h, w, dy)
    _hip.check(_hip.lib().srhip_diff_avgpool2x2_bwd(_p(dy), _p(dx), n, h, w, c, _stream()), 'diff_avgpool2x2_bwd')
    return dx


# ------------------------------------------------------------------------------------------------------------------------------ #
# QKVAttentionLegacy
# ------------------------------------------------------------------------------------------------------------------------------ #
def attention_fwd_lse(qkv, heads, want_lse=True):
    """(qkv dense, out [n, t, heads * ch], lse [n, heads, t]) on the qkv rows [n, t, heads * 3 * ch] (each head's q | k | v adjacent),
    ch in {32, 64}.  want_lse=False launches the kernel without its lse store (`out` has the same bits) and returns None for it."""
    ops._require_gpu(qkv, 'qkv_attention')
    if qkv.dim() != 3 or qkv.shape[2] % (3 * heads):
        raise ValueError('qkv_attention: expected [n, t, heads * 3 * ch], got %s for %d heads' % (tuple(qkv.shape), heads))
    qkv = qkv.contiguous()
    n, t, width = qkv.shape
    ch = width // (3 * heads)
    out = torch.empty(n, t, heads * ch, device=qkv.device, dtype=torch.float32)
    if not want_lse:
        _hip.check(_hip.lib().srhip_diff_attn_fwd(_p(qkv), _p(out), n, t, heads, ch, _stream()), 'diff_attn_fwd')
        return qkv, out, None
    lse = torch.empty(n, heads, t, device=qkv.device, dtype=torch.float32)
    _hip.check(_hip.lib().srhip_diff_attn_fwd_lse(_p(qkv), _p(out), _p(lse), n, t, heads, ch, _stream()), 'diff_attn_fwd_lse')
    return qkv, out, lse


def attention_bwd_raw(qkv, out, lse, dout, heads):
    """dqkv [n, t, heads * 3 * ch] from what attention_fwd_lse returned and dout [n, t, heads * ch]."""
    n, t, width = qkv.shape
    dout = dout.contiguous()
    if dout.data_ptr() % 16:
        dout = dout.clone()
    dqkv = torch.empty_like(qkv)
    lib = _hip.lib()
    ws = torch.empty(max(1, lib.srhip_diff_attn_bwd_workspace(n, t, heads) // 4), device=qkv.device, dtype=torch.float32)
    _hip.check(lib.srhip_diff_attn_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), _p(ws), ws.numel() * 4, n, t, heads,
                                       width // (3 * heads), _stream()), 'diff_attn_bwd')
    return dqkv


class _QKVAttention(Function):
    @staticmethod
    def forward(ctx, qkv, heads):
        need = ctx.needs_input_grad[0]
        qkv, out, lse = attention_fwd_lse(qkv, heads, need)
        if need:
            ctx.save_for_backward(qkv, out, lse)
            ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return attention_bwd_raw(qkv, out, lse, dout, ctx.heads), None


def qkv_attention(qkv, heads):
    """QKVAttentionLegacy on the qkv rows [n, t, heads * 3 * ch] -> [n, t, heads * ch]."""
    return _QKVAttention.apply(qkv, heads)


# ------------------------------------------------------------------------------------------------------------------------------ #
# row kernels of the sampler and of q_sample
# ------------------------------------------------------------------------------------------------------------------------------ #
def randn_rows(out, seed, step):
    """Fill out [..., rows, C] (row stride >= C) with the Philox normals of (seed, step); element index = row * C + channel."""
    out, ld = _rows(out, 'randn_rows')
    rows = out.numel() // out.shape[-1]
    _hip.check(_hip.lib().srhip_diff_randn(_p(out), ld, rows, out.shape[-1], int(seed), int(step), _stream()), 'diff_randn')
    return out


def sampler_step(x0, xt, out, c1, c2, logvar, t_nonzero, noise=None, seed=0, step=0):
    """out = c1 * clamp(x0, -1, 1) + c2 * xt + (t_nonzero ? exp(0.5 * logvar) * noise : 0) over rows [..., rows, C], every tensor with its
    own row stride; out may be xt.  noise=None draws randn_rows(seed, step)'s values in the kernel."""
    x0, l0 = _rows(x0, 'sampler_step')
    xt, lt = _rows(xt, 'sampler_step')
    out, lo = _rows(out, 'sampler_step')
    ln = 0
    if noise is not None:
        noise, ln = _rows(noise, 'sampler_step')
    ch = x0.shape[-1]
    rows = x0.numel() // ch
    for t in (xt, out) + ((noise,) if noise is not None else ()):
        if tuple(t.shape) != tuple(x0.shape):
            raise ValueError('sampler_step: shapes differ: %s vs %s' % (tuple(t.shape), tuple(x0.shape)))
    _hip.check(_hip.lib().srhip_diff_sampler_step(_p(x0), l0, _p(xt), lt, _p(noise), ln, _p(out), lo, rows, ch, float(c1), float(c2),
                                                  float(logvar), int(bool(t_nonzero)), int(seed), int(step), _stream()),
               'diff_sampler_step')
    return out


def q_sample_rows(x0, t, sqrt_ac, sqrt_1mac, out, noise=None, seed=0, step=0):
    """out = sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * eps over rows [B, ..., C] (each tensor with its own row stride; `out` may be a channel
    slice of the U-Net input).  t: int64 [B] on the device.  eps = noise, or randn_rows(seed, step)'s draws taken in the kernel."""
    x0, l0 = _rows(x0, 'q_sample')
    out, lo = _rows(out, 'q_sample')
    ln = 0
    if noise is not None:
        noise, ln = _rows(noise, 'q_sample')
    for other in (out,) + ((noise,) if noise is not None else ()):
        if tuple(other.shape) != tuple(x0.shape):
            raise ValueError('q_sample: shapes differ: %s vs %s' % (tuple(other.shape), tuple(x0.shape)))
    b, ch = x0.shape[0], x0.shape[-1]
    if not t.is_cuda or t.dtype != torch.int64 or tuple(t.shape) != (b,):
        raise TypeError('q_sample: t must be an int64 device tensor of shape (%d,), got %s %s on %s' % (b, t.dtype, tuple(t.shape), t.device))
    t = t.contiguous()
    _hip.check(_hip.lib().srhip_diff_q_sample(_p(x0), l0, _p(noise), ln, _p(out), lo, _p(t), _p(sqrt_ac), _p(sqrt_1mac), sqrt_ac.numel(), b,
                                              x0.numel() // (b * ch), ch, int(seed), int(step), _stream()), 'diff_q_sample')
    return out


def quantize_u8(x, min_max=(-1.0, 1.0)):
    """core/metrics.py tensor2img on the device: x [..., rows, C] float32 -> uint8 of the same shape, clamp to min_max, map to [0, 1],
    x 255, round half to even."""
    x, ld = _rows(x, 'quantize_u8')
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    rows = x.numel() // x.shape[-1]
    _hip.check(_hip.lib().srhip_diff_quant_u8(_p(x), ld, _p(out), rows, x.shape[-1], float(min_max[0]), float(min_max[1]), _stream()),
               'diff_quant_u8')
    return out
