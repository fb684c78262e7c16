"""GDP diffusion super-resolution, training: the reference's `GDP_x0/model/model.py` (DDPM) and the training half of
`gdp_modules/diffusion.py` (set_loss, q_sample, p_losses) on the HIP kernels.  model/gdp.py stays the sampler: its classes keep their
parameters frozen and refuse to train; the classes here derive from them, share their module tree and state-dict keys, and add the
backward pass.

  group_norm_act / silu / avg_pool2x2 / qkv_attention   autograd Functions over csrc/diffusion.hip: the forward kernels of gdp.py (the
                     attention one in its lse-emitting form, same bits) and srhip_diff_*_bwd.  Exact fp32, no atomics.
  TrainableUNet      gdp.UNet with parameters that require grad.  With grad enabled the forward runs the same kernels through
                     ops.conv2d / ops.linear (residual epilogues for the skip adds), ops.cat_channels and ops.upsample_nearest, so its
                     output has the bits of gdp.UNet.forward_embedded; without grad it IS that forward.  Conv arithmetic `half` is
                     replaced by `bf16x3` for forward and backward alike (_HoldConvMath).
  TrainableDiffusion set_loss, q_sample (srhip_diff_q_sample writes x_t into channels 0..2 of the U-Net input, gathering the schedule
                     coefficients by the device tensor t) and p_losses (sum-reduced, as the reference's reduction='sum').
  DDPM               the reference's model surface: feed_data, optimize_parameters (dp.ParamArena + srhip_adam_step, no host sync in
                     the step), test / sample, save_network / load_network in the reference's file layout.
  training_batch     uint8 HR tiles -> {'HR', 'SR', 'LR'} as prepare_data.py + LRHR_dataset.py make them.

Not built: dropout != 0, finetune_norm, EMA, nn.DataParallel, hipGraph capture."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _hip, data as sdata, dp, ops
from . import gdp
from .gdp import _image, _p, _rows, _stream, _tokens

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


# ------------------------------------------------------------------------------------------------------------------------------ #
# differentiable kernels (csrc/diffusion.hip)
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
    return y, ws[off:off + n * gdp.GROUPS * 2].view(n, gdp.GROUPS, 2)


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


def group_norm_act(x, weight, bias, scale=None, shift=None, silu=False, eps=1e-5, mod=None):
    """gdp.group_norm_act, differentiable in x, weight, bias and the modulation.  The modulation is `mod` [n, 2 C] = scale | shift (the
    emb_layers row as it stands) or `scale` and `shift` [n, C]."""
    if (scale is None) != (shift is None):
        raise ValueError('group_norm_act: scale and shift come together')
    if scale is not None:
        mod = torch.cat([scale, shift], dim=1)
    return _GroupNormAct.apply(x, weight, bias, mod, silu, eps)


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


def attention_fwd_lse(qkv, heads):
    """(out [n, t, heads * ch], lse [n, heads, t]) of gdp.qkv_attention's arithmetic; `out` has its bits."""
    ops._require_gpu(qkv, 'qkv_attention')
    if qkv.dim() != 3 or qkv.shape[2] % (3 * heads):
        raise ValueError('qkv_attention: expected [n, t, heads * 3 * ch], got %s for %d heads' % (tuple(qkv.shape), heads))
    qkv = qkv.contiguous()
    n, t, width = qkv.shape
    ch = width // (3 * heads)
    out = torch.empty(n, t, heads * ch, device=qkv.device, dtype=torch.float32)
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
        qkv, out, lse = attention_fwd_lse(qkv, heads)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return attention_bwd_raw(qkv, out, lse, dout, ctx.heads), None


def qkv_attention(qkv, heads):
    return _QKVAttention.apply(qkv, heads)


def q_sample_rows(x0, t, sqrt_ac, sqrt_1mac, out, noise=None, seed=0, step=0):
    """out = sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * eps over rows [B, ..., C] (each tensor with its own row stride; `out` may be a channel
    slice of the U-Net input).  t: int64 [B] on the device.  eps = noise, or gdp.randn_rows(seed, step)'s draws taken in the kernel."""
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


# ------------------------------------------------------------------------------------------------------------------------------ #
# the U-Net with a backward pass: gdp.py's modules, walked with differentiable ops
# ------------------------------------------------------------------------------------------------------------------------------ #
def _conv(x, conv, residual=None):
    w = conv.weight
    if w.dim() == 4:
        return ops.conv2d(x, w, conv.bias, 1, w.shape[2] // 2, None, residual)
    return ops.linear(x, w, conv.bias, residual)             # nn.Linear and the attention's nn.Conv1d(k = 1): the 1 x 1 conv route


def _norm(x, gn, mod=None, act=False):
    n, c, h, w = x.shape
    return _image(_GroupNormAct.apply(_tokens(x), gn.weight, gn.bias, mod, act, gn.eps), h, w)


def _res_forward(blk, x, emb_act):
    h = _norm(x, blk.in_layers[0], act=True)
    if blk.updown:
        if blk.h_upd.up:
            h, x = ops.upsample_nearest(h, 2), ops.upsample_nearest(x, 2)
        else:
            h, x = avg_pool2x2(h), avg_pool2x2(x)
    h = _conv(h, blk.in_layers[2])
    mod = _conv(emb_act, blk.emb_layers[1]).reshape(x.shape[0], 2 * blk.out_channel)
    h = _norm(h, blk.out_layers[0], mod, act=True)
    skip = x if isinstance(blk.skip_connection, nn.Identity) else _conv(x, blk.skip_connection)
    return _conv(h, blk.out_layers[3], residual=skip)


def _attn_forward(blk, x):
    n, c, h, w = x.shape
    qkv = _conv(_norm(x, blk.norm), blk.qkv)
    a = qkv_attention(_tokens(qkv), blk.num_heads)
    return _conv(_image(a, h, w), blk.proj_out, residual=x)


def _block_forward(block, x, emb_act):
    for layer in block:
        if isinstance(layer, gdp.ResBlock):
            x = _res_forward(layer, x, emb_act)
        elif isinstance(layer, gdp.AttentionBlock):
            x = _attn_forward(layer, x)
        else:
            x = _conv(x, layer)
    return x


def _thaw(net):
    """Parameters require grad and join the per-step batched re-pack: the static mark goes, and packed images made while the net was
    frozen (a net that was sampled from first) are dropped, so that the next use packs them again and registers them."""
    dropped = set()
    for p in net.parameters():
        p.requires_grad_(True)
        dropped.update(id(ent) for ent in getattr(p, '_srhip_packed', {}).values())
        for attr in ('_srhip_static', '_srhip_packed'):
            if hasattr(p, attr):
                delattr(p, attr)
    reg = ops._registry                                  # a net that has trained before: its images leave the batched re-pack too
    if any(id(ent) in dropped for ent in reg.entries):
        reg.entries = [ent for ent in reg.entries if id(ent) not in dropped]
        reg.dirty = True


class _HoldConvMath(Function):
    """Identity on the U-Net's output whose backward switches the conv arithmetic to `mode` for the rest of that backward pass (the
    net's data and weight gradients: everything behind its output) and puts the caller's mode back when the pass ends."""

    @staticmethod
    def forward(ctx, y, mode):
        ctx.mode = mode
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        prev = ops.set_conv_math(ctx.mode)
        torch.autograd.Variable._execution_engine.queue_callback(lambda: ops.set_conv_math(prev))
        return g, None


class TrainableUNet(gdp.UNet):
    def __init__(self, image_size, in_channel=3, model_channels=128, out_channel=3, res_blocks=2, attention_resolutions=(32, 16, 8),
                 dropout=0, **kw):
        if dropout != 0:
            raise NotImplementedError('dropout=%r: the training forward has no dropout kernel (every reference config trains with 0.0)'
                                      % (dropout,))
        super().__init__(image_size, in_channel, model_channels, out_channel, res_blocks, attention_resolutions, dropout, **kw)
        _thaw(self)
        self.train()

    @classmethod
    def adopt(cls, net):
        """Make a gdp.UNet (e.g. one loaded for sampling, and sampled from) trainable in place; returns it."""
        if not isinstance(net, gdp.UNet):
            raise TypeError('TrainableUNet.adopt expects a gdp.UNet, got %s' % type(net).__name__)
        if net.dropout != 0:
            raise NotImplementedError('dropout=%r: the training forward has no dropout kernel' % (net.dropout,))
        net.__class__ = cls
        _thaw(net)
        return net.train()

    def embed(self, emb_in):
        if not torch.is_grad_enabled():
            return super().embed(emb_in)
        n = emb_in.shape[0]
        e = _conv(emb_in.reshape(n, -1, 1, 1), self.time_embed[0])
        return silu(_conv(silu(e), self.time_embed[2]))

    def forward_embedded(self, x, emb_in):
        if not torch.is_grad_enabled():
            return super().forward_embedded(x, emb_in)
        if ops.get_conv_math() == 'half':                # as the sampler: the U-Net is outside the 16-bit contract, forward AND backward
            with ops.conv_math('bf16x3'):
                y = self.forward_embedded(x, emb_in)
            return _HoldConvMath.apply(y, 'bf16x3')
        emb_act = self.embed(emb_in)
        h, hs = x, []
        for block in self.input_blocks:
            h = _block_forward(block, h, emb_act)
            hs.append(h)
        h = _block_forward(self.middle_block, h, emb_act)
        for block in self.output_blocks:
            h = _block_forward(block, ops.cat_channels([h, hs.pop()]), emb_act)
        return _conv(_norm(h, self.out[0], act=True), self.out[2])

    def forward(self, x, timesteps, y=None):
        if not torch.is_grad_enabled():
            return super().forward(x, timesteps, y)
        if y is not None:
            raise NotImplementedError('num_classes: class conditioning is not built')
        ops._require_gpu(x, 'gdp_train.TrainableUNet')
        if x.dim() != 4 or x.shape[1] != self.in_channel:
            raise ValueError('gdp_train.TrainableUNet: input must be [N, %d, H, W], got %s' % (self.in_channel, tuple(x.shape)))
        down = 2 ** (len(self.channel_mults) - 1)
        if x.shape[2] % down or x.shape[3] % down:
            raise ValueError('gdp_train.TrainableUNet: H and W must be multiples of %d, got %d x %d' % (down, x.shape[2], x.shape[3]))
        emb_in = gdp.timestep_embedding(torch.as_tensor(timesteps), self.model_channels).to(x.device)
        return self.forward_embedded(ops.nhwc(x), emb_in)


# ------------------------------------------------------------------------------------------------------------------------------ #
# p_losses
# ------------------------------------------------------------------------------------------------------------------------------ #
class TrainableDiffusion(gdp.GaussianDiffusion):
    def set_loss(self, device):
        if self.loss_type not in ('l1', 'l2'):
            raise NotImplementedError('loss_type=%r: l1 and l2 are what the reference names' % (self.loss_type,))
        self.loss_kind = self.loss_type

    def _table(self, device):
        """Sinusoid rows of every timestep on the device: a step gathers its rows by t, nothing goes through the host."""
        if self._sinusoid is None or self._sinusoid.device != device:
            self._sinusoid = gdp.timestep_embedding(torch.arange(self.num_timesteps), self.denoise_fn.model_channels).to(device)
        return self._sinusoid

    def _check_batch(self, x, what):
        ops._require_gpu(x, what)
        if x.dim() != 4:
            raise ValueError('%s: expected [B, C, H, W], got %s' % (what, tuple(x.shape)))

    def q_sample(self, x_start, t, noise=None, *, seed=None, step=0):
        """x_t = sqrt(acp[t]) x_start + sqrt(1 - acp[t]) noise for x_start [B, C, H, W]; t int64 [B] (moved to the device if it is not
        there).  noise=None draws Philox normals of (seed, step) in the kernel."""
        self._need_schedule()
        self._check_batch(x_start, 'gdp_train.q_sample')
        b, c, h, w = x_start.shape
        out = torch.empty(b, h, w, c, device=x_start.device, dtype=torch.float32)
        self._q_rows(x_start, t, noise, seed, step, out)
        return out.permute(0, 3, 1, 2)

    def _q_rows(self, x_start, t, noise, seed, step, out):
        t = torch.as_tensor(t).to(device=x_start.device, dtype=torch.int64)
        if noise is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())               # a host tensor from torch's CPU generator: no device sync
        rows = ops.nhwc(x_start).permute(0, 2, 3, 1)
        nrows = None
        if noise is not None:
            self._check_batch(noise, 'gdp_train.q_sample (noise)')
            nrows = ops.nhwc(noise).permute(0, 2, 3, 1)
        q_sample_rows(rows, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, out, nrows, seed or 0, step)
        return t

    def p_losses(self, x_in, noise=None, *, t=None, seed=None):
        """The reference's p_losses: x_in = {'HR', 'SR'[, 'LR']} in [-1, 1] -> loss_func(denoise_fn(cat(q_sample(HR, t), SR), t), HR),
        SUM-reduced.  t: int64 [B], default torch.randint(0, T, (B,)) on the device; noise: the draw to use, default Philox normals of
        `seed` (default: drawn from torch's CPU generator)."""
        self._need_schedule()
        if not hasattr(self, 'loss_kind'):
            raise RuntimeError('TrainableDiffusion: call set_loss(device) first')
        hr = x_in['HR']
        self._check_batch(hr, 'gdp_train.p_losses')
        b, c, h, w = hr.shape
        if t is None:
            t = torch.randint(0, self.num_timesteps, (b,), device=hr.device).long()
        extra = 0
        if self.conditional:
            sr = x_in['SR']
            self._check_batch(sr, 'gdp_train.p_losses (SR)')
            extra = sr.shape[1]
        buf = torch.empty(b, h, w, c + extra, device=hr.device, dtype=torch.float32)
        if extra:
            buf[..., c:] = sr.permute(0, 2, 3, 1)
        t = self._q_rows(hr, t, noise, seed, 0, buf[..., :c])
        x_recon = self.denoise_fn.forward_embedded(buf.permute(0, 3, 1, 2), self._table(hr.device).index_select(0, t))
        mean = ops.l1_mean(x_recon, hr) if self.loss_kind == 'l1' else ops.mse_mean(x_recon, hr)
        return mean * float(hr.numel())

    def forward(self, x, *args, **kwargs):
        return self.p_losses(x, *args, **kwargs)


def define_G(opt):
    """gdp.define_G with the trainable classes."""
    m = opt['model']
    if m['which_model_G'] != 'gdp':
        raise NotImplementedError("which_model_G=%r: only 'gdp' is built (the reference ships no ddpm module)" % m['which_model_G'])
    u = m['unet']
    model = TrainableUNet(in_channel=u['in_channel'], out_channel=u['out_channel'], norm_groups=u.get('norm_groups') or 32,
                          inner_channel=u['inner_channel'], channel_mults=u['channel_multiplier'], attn_res=u['attn_res'],
                          res_blocks=u['res_blocks'], dropout=u['dropout'], image_size=m['diffusion']['image_size'])
    return TrainableDiffusion(model, image_size=m['diffusion']['image_size'], channels=m['diffusion']['channels'], loss_type='l2',
                              conditional=m['diffusion']['conditional'], schedule_opt=m['beta_schedule']['train'])


# ------------------------------------------------------------------------------------------------------------------------------ #
# the trainer (model/model.py)
# ------------------------------------------------------------------------------------------------------------------------------ #
class DDPM:
    def __init__(self, opt, device=None, netG=None):
        """opt: the reference's configuration dict.  netG: a TrainableDiffusion to train instead of define_G(opt)'s (a U-Net whose
        shape the configuration file cannot express, or one adopted from a sampler)."""
        self.opt = opt
        self.device = torch.device(device if device is not None else 'cuda:0')
        if self.device.type != 'cuda':
            raise RuntimeError('gdp_train.DDPM: runs on the MI355X HIP path only (got device %s); there is no CPU fallback' % self.device)
        if opt['model'].get('finetune_norm'):
            raise NotImplementedError("finetune_norm=True: it selects parameters named 'transformer', of which this U-Net has none")
        self.begin_step = self.begin_epoch = 0
        if netG is not None and not isinstance(netG, TrainableDiffusion):
            raise TypeError('gdp_train.DDPM: netG must be a TrainableDiffusion, got %s' % type(netG).__name__)
        self.netG = (netG if netG is not None else define_G(opt)).to(self.device)
        self.schedule_phase = None
        self.set_loss()
        self.set_new_noise_schedule(opt['model']['beta_schedule']['train'], schedule_phase='train')
        self.train_phase = opt['phase'] == 'train'
        if self.train_phase:
            self.netG.train()
            self.lr = float(opt['train']['optimizer']['lr'])
            self.arena = dp.ParamArena(self.netG)
            self.steps = 0
            self.log_dict = OrderedDict()
        self.load_network()

    def set_device(self, x):
        if isinstance(x, dict):
            return {k: (v.to(self.device) if v is not None and torch.is_tensor(v) else v) for k, v in x.items()}
        if isinstance(x, list):
            return [v.to(self.device) if v is not None else v for v in x]
        return x.to(self.device)

    def feed_data(self, data):
        self.data = self.set_device(data)

    def optimize_parameters(self, noise=None, *, t=None, seed=None):
        """One Adam step on the fed batch.  noise / t / seed reach p_losses (tests inject them); the reference passes none."""
        if not self.train_phase:
            raise RuntimeError("gdp_train.DDPM: optimize_parameters needs opt['phase'] == 'train' (no optimiser was built)")
        a = self.arena
        a.zero_grad()
        b, c, h, w = self.data['HR'].shape
        l_pix = self.netG(self.data, noise, t=t, seed=seed) / int(b * c * h * w)
        l_pix.backward()
        _hip.check(_hip.lib().srhip_adam_step(_p(a.flat_p), _p(a.flat_g), _p(a.exp_avg), _p(a.exp_avg_sq), _p(a.step_state), a.numel, self.lr,
                                              ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, 1.0, 0.0, _stream()), 'adam_step')
        ops.bump_weight_epoch()
        self.steps += 1
        self.log_dict['l_pix'] = l_pix.detach()            # a 0-d device tensor: reading it is the caller's sync, not the step's

    def test(self, continous=False, *, noise=None, seed=None):
        self.netG.eval()
        with torch.no_grad():
            self.SR = self.netG.super_resolution(self.data['SR'], continous, noise=noise, seed=seed)
        self.netG.train()

    def sample(self, batch_size=1, continous=False, *, noise=None, seed=None):
        self.netG.eval()
        with torch.no_grad():
            self.SR = self.netG.sample(batch_size, continous, noise=noise, seed=seed)
        self.netG.train()

    def set_loss(self):
        self.netG.set_loss(self.device)

    def set_new_noise_schedule(self, schedule_opt, schedule_phase='train'):
        if self.schedule_phase is None or self.schedule_phase != schedule_phase:
            self.schedule_phase = schedule_phase
            self.netG.set_new_noise_schedule(schedule_opt, self.device)

    def get_current_log(self):
        return self.log_dict

    def get_current_visuals(self, need_LR=True, sample=False):
        out = OrderedDict()
        if sample:
            out['SAM'] = self.SR.detach().float().cpu()
        else:
            out['SR'] = self.SR.detach().float().cpu()
            out['INF'] = self.data['SR'].detach().float().cpu()
            out['HR'] = self.data['HR'].detach().float().cpu()
            if 'HR_Mask' in self.data:
                out['HR_Mask'] = self.data['HR_Mask'].detach().float().cpu()
            out['LR'] = self.data['LR'].detach().float().cpu() if need_LR and 'LR' in self.data else out['INF']
        return out

    # ---- checkpoints in the reference's layout ------------------------------------------------------------------------------- #
    def optimizer_state_dict(self):
        """The arena's Adam state as torch.optim.Adam(list(netG.parameters()), lr).state_dict() would hold it (made by such an
        optimiser over host copies, so the layout is the installed torch's own)."""
        a = self.arena
        host = [nn.Parameter(torch.empty(p.shape), requires_grad=True) for p in a.params]
        opt = torch.optim.Adam(host, lr=self.lr, betas=ADAM_BETAS, eps=ADAM_EPS)
        if self.steps:
            m, v = a.exp_avg.cpu(), a.exp_avg_sq.cpu()
            for q, p, o in zip(host, a.params, a.offsets):
                opt.state[q] = {'step': torch.tensor(float(self.steps)), 'exp_avg': m[o:o + p.numel()].view(p.shape).clone(),
                                'exp_avg_sq': v[o:o + p.numel()].view(p.shape).clone()}
        return opt.state_dict()

    def load_optimizer_state_dict(self, sd):
        a = self.arena
        if len(sd['param_groups']) != 1 or len(sd['param_groups'][0]['params']) != len(a.params):
            raise ValueError('optimizer state: expected one group of %d parameters' % len(a.params))
        g = sd['param_groups'][0]
        if tuple(g.get('betas', ADAM_BETAS)) != ADAM_BETAS or g.get('eps', ADAM_EPS) != ADAM_EPS or g.get('weight_decay', 0) != 0 \
                or g.get('amsgrad', False):
            raise NotImplementedError('optimizer state: Adam with betas %s, eps %g, no weight decay, no amsgrad is what the step runs'
                                      % (ADAM_BETAS, ADAM_EPS))
        self.lr = float(g['lr'])
        steps = set()
        a.exp_avg.zero_()
        a.exp_avg_sq.zero_()
        for idx, p, o in zip(g['params'], a.params, a.offsets):
            st = sd['state'].get(idx)
            if st is None:
                steps.add(0)
                continue
            steps.add(int(st['step']))
            a.exp_avg[o:o + p.numel()].view(p.shape).copy_(st['exp_avg'])
            a.exp_avg_sq[o:o + p.numel()].view(p.shape).copy_(st['exp_avg_sq'])
        if len(steps) != 1:
            raise NotImplementedError('optimizer state: parameters at different step counts %s (the arena keeps one)' % sorted(steps))
        self.steps = steps.pop()
        a.step_state.zero_()
        a.step_state[0] = float(self.steps)                 # the kernel derives its bias corrections from the count

    def save_network(self, epoch, iter_step):
        root = self.opt['path']['checkpoint']
        gen_path = os.path.join(root, 'I{}_E{}_gen.pth'.format(iter_step, epoch))
        opt_path = os.path.join(root, 'I{}_E{}_opt.pth'.format(iter_step, epoch))
        torch.save(OrderedDict((k, v.detach().cpu().clone()) for k, v in self.netG.state_dict().items()), gen_path)
        torch.save({'epoch': epoch, 'iter': iter_step, 'scheduler': None, 'optimizer': self.optimizer_state_dict()}, opt_path)
        return gen_path, opt_path

    def load_network(self):
        load_path = self.opt['path'].get('resume_state')
        if load_path is None:
            return
        state = torch.load('{}_gen.pth'.format(load_path), map_location='cpu')
        with torch.no_grad():
            self.netG.load_state_dict(state, strict=False)       # in place: the parameters stay views of the arena
        if self.train_phase:
            opt = torch.load('{}_opt.pth'.format(load_path), map_location='cpu')
            self.load_optimizer_state_dict(opt['optimizer'])
            self.begin_step, self.begin_epoch = opt['iter'], opt['epoch']
            if not self.arena.check_views():
                raise RuntimeError('gdp_train.DDPM: loading the checkpoint detached the parameters from the arena')


def training_batch(hr_u8, lr_size):
    """uint8 HR tiles [N, H, W, 3] on the device -> {'HR', 'SR', 'LR'} float32 in [-1, 1] as prepare_data.py (Pillow bicubic down to
    lr_size, then back up to H x W) and LRHR_dataset.py (to_tensor * 2 - 1) make them."""
    if not torch.is_tensor(hr_u8) or hr_u8.dtype != torch.uint8 or hr_u8.dim() != 4:
        raise TypeError('training_batch expects a [N, H, W, 3] uint8 tensor')
    if not hr_u8.is_cuda:
        raise RuntimeError('training_batch: runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback' % hr_u8.device.type)
    _, h, w, _ = hr_u8.shape
    lr = sdata.resize_u8(hr_u8, lr_size, lr_size)
    sr = sdata.resize_u8(lr, h, w)
    return {k: sdata.to_tensor(v) * 2.0 + (-1.0) for k, v in (('HR', hr_u8), ('SR', sr), ('LR', lr))}
