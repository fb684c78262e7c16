"""GDP diffusion super-resolution, sampling only: the reference's `GDP_x0/model/gdp_modules` (unet.py: UNet, diffusion.py:
GaussianDiffusion) and `networks.define_G`, run from a trained `I*_E*_gen.pth` on the HIP kernels.  There is no backward pass, no
training step and no optimiser here: the classes below keep their parameters frozen and refuse to train.  model/gdp_train.py derives
the trainable ones from them (TrainableUNet, TrainableDiffusion, DDPM).

  UNet               guided-diffusion's U-Net with the reference's signature, defaults and state-dict keys.  Activations are NHWC;
                     every conv (3x3, and the 1x1 skip / qkv / proj_out) goes through srhip_conv2d_fwd with its bias and residual
                     epilogues, so it follows the conv arithmetic mode; GroupNorm + scale-shift + SiLU, the 2x2 average pool and
                     QKVAttentionLegacy are csrc/diffusion.hip in exact fp32.
  GaussianDiffusion  the schedule (float64 on the host, the reference's nine float32 buffers plus betas / alphas_cumprod(_prev)) and
                     p_sample / p_sample_loop / super_resolution / sample.  x_t lives in channels 0..2 of the six-channel U-Net input
                     for the whole loop and the condition in channels 3..5: the sampler kernel writes x_{t-1} in place through a row
                     stride.  Noise is a caller's tensor (`noise=`, parity with torch.randn) or Philox draws in the kernel (`seed=`).
  define_G / load_gen / gdp_super_resolve   the reference's config dict -> model, its checkpoint -> weights, and sr_mfe.py's
                     validation path (uint8 LR -> bicubic -> [-1, 1] -> sampler -> tensor2img) without files in between.

The kernels of csrc/diffusion.hip are called through model/gdp_kernels.py.  The U-Net's forward is written once, over ops and those
differentiable kernels: it runs under torch.no_grad() here and with grad enabled in gdp_train.TrainableUNet."""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import data as sdata, ops
from .gdp_kernels import (GROUPS, avg_pool2x2, group_norm_act, qkv_attention, quantize_u8, randn_rows, sampler_step,  # noqa: F401
                          silu)

SCHEDULE_BUFFERS = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod',
                    'log_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_variance',
                    'posterior_log_variance_clipped', 'posterior_mean_coef1', 'posterior_mean_coef2')
_TRAINING = 'training is not built: this is the sampler (gdp_train.TrainableDiffusion and gdp_train.DDPM train)'


# ------------------------------------------------------------------------------------------------------------------------------ #
# the U-Net: parameter holders with the reference's module tree (so the state-dict keys are the reference's), forward on the kernels
# ------------------------------------------------------------------------------------------------------------------------------ #
def _zero(module):
    for p in module.parameters():
        p.detach().zero_()
    return module


def _tokens(x):
    """logical [n, C, h, w] over NHWC memory -> the same memory as [n, h * w, C]"""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c)


def _image(rows, h, w):
    n, _, c = rows.shape
    return rows.reshape(n, h, w, c).permute(0, 3, 1, 2)


def _conv(x, conv, residual=None):
    w = conv.weight
    if w.dim() == 4:
        return ops.conv2d(x, w, conv.bias, 1, w.shape[2] // 2, None, residual)
    return ops.linear(x, w, conv.bias, residual)             # nn.Linear and the attention's nn.Conv1d(k = 1): the 1 x 1 conv route


def _norm(x, gn, mod=None, act=False):
    n, c, h, w = x.shape
    return _image(group_norm_act(_tokens(x), gn.weight, gn.bias, silu=act, eps=gn.eps, mod=mod), h, w)


class _Resample(nn.Module):
    """Upsample(channels, False) / Downsample(channels, False): no parameters."""

    def __init__(self, up):
        super().__init__()
        self.up = up

    def forward(self, x):
        return ops.upsample_nearest(x, 2) if self.up else avg_pool2x2(x)


class ResBlock(nn.Module):
    def __init__(self, channels, emb_channels, dropout, out_channel=None, up=False, down=False):
        super().__init__()
        self.channels, self.out_channel = channels, out_channel or channels
        self.in_layers = nn.Sequential(nn.GroupNorm(GROUPS, channels), nn.SiLU(), nn.Conv2d(channels, self.out_channel, 3, padding=1))
        self.updown = up or down
        if self.updown:
            self.h_upd, self.x_upd = _Resample(up), _Resample(up)
        else:
            self.h_upd = self.x_upd = nn.Identity()
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * self.out_channel))
        self.out_layers = nn.Sequential(nn.GroupNorm(GROUPS, self.out_channel), nn.SiLU(), nn.Dropout(p=dropout),
                                        _zero(nn.Conv2d(self.out_channel, self.out_channel, 3, padding=1)))
        if self.out_channel == channels:
            self.skip_connection = nn.Identity()
        else:
            self.skip_connection = nn.Conv2d(channels, self.out_channel, 1)

    def forward(self, x, emb_act):
        """emb_act: SiLU(emb) as [n, E, 1, 1] (the SiLU of emb_layers is the same for every block: taken once per forward)."""
        h = _norm(x, self.in_layers[0], act=True)
        if self.updown:
            h, x = self.h_upd.forward(h), self.x_upd.forward(x)
        h = _conv(h, self.in_layers[2])
        mod = _conv(emb_act, self.emb_layers[1]).reshape(x.shape[0], 2 * self.out_channel)      # scale | shift, as the kernel reads it
        h = _norm(h, self.out_layers[0], mod, act=True)
        skip = x if isinstance(self.skip_connection, nn.Identity) else _conv(x, self.skip_connection)
        return _conv(h, self.out_layers[3], residual=skip)


class AttentionBlock(nn.Module):
    def __init__(self, channels, num_heads, num_head_channels):
        super().__init__()
        self.channels = channels
        if num_head_channels == -1:
            self.num_heads = num_heads
        else:
            if channels % num_head_channels:
                raise ValueError('q,k,v channels %d is not divisible by num_head_channels %d' % (channels, num_head_channels))
            self.num_heads = channels // num_head_channels
        if channels % self.num_heads or channels // self.num_heads not in (32, 64):
            raise NotImplementedError('num_heads / num_head_channels: the attention kernel has head widths 32 and 64, %d channels in %d '
                                      'heads is %s' % (channels, self.num_heads, channels / self.num_heads))
        self.norm = nn.GroupNorm(GROUPS, channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = _zero(nn.Conv1d(channels, channels, 1))

    def forward(self, x):
        n, c, h, w = x.shape
        qkv = _conv(_norm(x, self.norm), self.qkv)
        a = qkv_attention(_tokens(qkv), self.num_heads)
        return _conv(_image(a, h, w), self.proj_out, residual=x)


class _Block(nn.Sequential):
    """TimestepEmbedSequential.  The walk invokes the holders' `forward` directly (here, in ResBlock and in UNet._walk): they carry no
    hooks, and nn.Module's call machinery on some 75 of them per forward measured 0.3 % of a fp32 training step."""

    def forward(self, x, emb_act):
        for layer in self:
            if isinstance(layer, ResBlock):
                x = layer.forward(x, emb_act)
            elif isinstance(layer, AttentionBlock):
                x = layer.forward(x)
            else:
                x = _conv(x, layer)
        return x


def timestep_embedding(timesteps, dim, max_period=10000):
    """Sinusoid rows [N, dim] in float32, on the host: row t = (cos(t f_0) .. cos(t f_{h-1}), sin(t f_0) .. sin(t f_{h-1})) with h = dim // 2
    and f_j = max_period^(-j / h); an odd dim gets one trailing zero column.  Every product and function is taken in float32, as the
    trained weights expect."""
    h = dim // 2
    j = torch.arange(h, dtype=torch.float32)
    f = torch.exp(j * (-math.log(max_period)) / h)
    phase = timesteps.detach().cpu().to(torch.float32).reshape(-1, 1) * f.reshape(1, -1)
    rows = torch.zeros(phase.shape[0], dim, dtype=torch.float32)
    rows[:, :h] = torch.cos(phase)
    rows[:, h:2 * h] = torch.sin(phase)
    return rows


def unet_plan(model_channels, channel_mults, res_blocks, attention_resolutions):
    """The U-Net as three lists of blocks (encoder, middle, decoder), each block a list of layers ('conv', cin, cout) |
    ('res', cin, cout, None | 'down' | 'up') | ('attn', channels).  Level l has width channel_mults[l] * model_channels and runs at
    1 / 2^l of the input size; attention follows a ResBlock wherever 2^l is in attention_resolutions.  The encoder records the width
    of every block output; the decoder's ResBlocks read them back last in, first out, concatenated to their input."""
    widths = [int(m * model_channels) for m in channel_mults]
    last = len(widths) - 1
    enc, skips = [[('conv', None, widths[0])]], [widths[0]]
    ch = widths[0]
    for level, wd in enumerate(widths):
        attn = [('attn', wd)] if 2 ** level in attention_resolutions else []
        for _ in range(res_blocks):
            enc.append([('res', ch, wd, None)] + attn)
            skips.append(wd)
            ch = wd
        if level < last:
            enc.append([('res', ch, ch, 'down')])
            skips.append(ch)
    attn = [('attn', ch)]
    mid = [('res', ch, ch, None)] + attn + [('res', ch, ch, None)]
    dec = []
    for level in range(last, -1, -1):
        wd = widths[level]
        attn = [('attn', wd)] if 2 ** level in attention_resolutions else []
        for i in range(res_blocks + 1):
            block = [('res', ch + skips.pop(), wd, None)] + attn
            ch = wd
            if level > 0 and i == res_blocks:
                block.append(('res', ch, ch, 'up'))
            dec.append(block)
    return enc, mid, dec


class UNet(nn.Module):
    def __init__(self, image_size, in_channel=3, model_channels=128, out_channel=3, res_blocks=2, attention_resolutions=(32, 16, 8),
                 dropout=0, channel_mults=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False,
                 num_heads=4, num_head_channels=64, num_heads_upsample=-1, use_scale_shift_norm=True, resblock_updown=True,
                 use_new_attention_order=False, inner_channel=32, norm_groups=32, attn_res=(8), with_time_emb=True):
        super().__init__()
        for name, value, built in (('dims', dims, 2), ('num_classes', num_classes, None), ('use_fp16', use_fp16, False),
                                   ('use_scale_shift_norm', use_scale_shift_norm, True), ('resblock_updown', resblock_updown, True),
                                   ('use_new_attention_order', use_new_attention_order, False)):
            if value != built:
                raise NotImplementedError('%s=%r: the sampler is built for %s=%r only' % (name, value, name, built))
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        if model_channels % GROUPS or any(int(m * model_channels) % GROUPS for m in channel_mults):
            raise NotImplementedError('model_channels / channel_mults: every width must be a multiple of %d (GroupNorm32)' % GROUPS)
        self.image_size, self.in_channel, self.model_channels, self.out_channel = image_size, in_channel, model_channels, out_channel
        self.res_blocks, self.attention_resolutions, self.dropout, self.channel_mults = res_blocks, attention_resolutions, dropout, channel_mults
        self.conv_resample, self.num_classes, self.use_checkpoint, self.dtype = conv_resample, num_classes, use_checkpoint, torch.float32
        self.num_heads, self.num_head_channels, self.num_heads_upsample = num_heads, num_head_channels, num_heads_upsample

        emb_dim = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, emb_dim), nn.SiLU(), nn.Linear(emb_dim, emb_dim))
        enc, mid, dec = unet_plan(model_channels, channel_mults, res_blocks, attention_resolutions)

        def build(block, heads):
            layers = []
            for kind, *spec in block:
                if kind == 'conv':
                    layers.append(nn.Conv2d(in_channel, spec[1], 3, padding=1))
                elif kind == 'res':
                    layers.append(ResBlock(spec[0], emb_dim, dropout, out_channel=spec[1], up=spec[2] == 'up', down=spec[2] == 'down'))
                else:
                    layers.append(AttentionBlock(spec[0], heads, num_head_channels))
            return _Block(*layers)

        self.input_blocks = nn.ModuleList([build(b, num_heads) for b in enc])
        self.middle_block = build(mid, num_heads)
        self.output_blocks = nn.ModuleList([build(b, num_heads_upsample) for b in dec])
        width0 = int(channel_mults[0] * model_channels)
        self.out = nn.Sequential(nn.GroupNorm(GROUPS, width0), nn.SiLU(), _zero(nn.Conv2d(width0, out_channel, 3, padding=1)))
        for p in self.parameters():
            p.requires_grad_(False)
        ops.mark_static(self)
        self.eval()

    def embed(self, emb_in):
        """time_embed on sinusoid rows [n, model_channels] (device) -> SiLU(emb) as [n, 4 * model_channels, 1, 1]: every ResBlock's
        emb_layers starts with that SiLU."""
        e = _conv(emb_in.reshape(emb_in.shape[0], -1, 1, 1), self.time_embed[0])
        return silu(_conv(silu(e), self.time_embed[2]))

    def _walk(self, x, emb_in):
        """The forward on x [N, in_channel, H, W] (NHWC memory) and sinusoid rows, in the caller's grad mode and conv arithmetic."""
        emb_act = self.embed(emb_in)
        h, hs = x, []
        for block in self.input_blocks:
            h = block.forward(h, emb_act)
            hs.append(h)
        h = self.middle_block.forward(h, emb_act)
        for block in self.output_blocks:
            h = block.forward(ops.cat_channels([h, hs.pop()]), emb_act)
        return _conv(_norm(h, self.out[0], act=True), self.out[2])

    def _checked_rows(self, who, x, timesteps, y):
        """UNet.forward's input checks, with `who` in the messages -> the sinusoid rows of `timesteps` on x's device."""
        if y is not None:
            raise NotImplementedError('num_classes: class conditioning is not built')
        ops._require_gpu(x, who)
        if x.dim() != 4 or x.shape[1] != self.in_channel:
            raise ValueError('%s: input must be [N, %d, H, W], got %s' % (who, self.in_channel, tuple(x.shape)))
        down = 2 ** (len(self.channel_mults) - 1)
        if x.shape[2] % down or x.shape[3] % down:
            raise ValueError('%s: H and W must be multiples of %d, got %d x %d' % (who, down, x.shape[2], x.shape[3]))
        return timestep_embedding(torch.as_tensor(timesteps), self.model_channels).to(x.device)

    @torch.no_grad()
    def forward_embedded(self, x, emb_in):
        if ops.get_conv_math() == 'half':                # inference must not move with the training arithmetic
            with ops.conv_math('bf16x3'):
                return self._walk(x, emb_in)
        return self._walk(x, emb_in)

    @torch.no_grad()
    def forward(self, x, timesteps, y=None):
        """x [N, in_channel, H, W] float32 on the device, timesteps [N] -> [N, out_channel, H, W] (NHWC memory).  Eval mode, no grad."""
        return self.forward_embedded(ops.nhwc(x), self._checked_rows('gdp.UNet', x, timesteps, y))


# ------------------------------------------------------------------------------------------------------------------------------ #
# the schedule and the sampler
# ------------------------------------------------------------------------------------------------------------------------------ #
def _warmup_beta(start, end, n, frac):
    betas = end * np.ones(n, dtype=np.float64)
    k = int(n * frac)
    betas[:k] = np.linspace(start, end, k, dtype=np.float64)
    return betas


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """float64 betas of every schedule the reference names."""
    if schedule == 'quad':
        return np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2
    if schedule == 'linear':
        return np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64)
    if schedule == 'warmup10':
        return _warmup_beta(linear_start, linear_end, n_timestep, 0.1)
    if schedule == 'warmup50':
        return _warmup_beta(linear_start, linear_end, n_timestep, 0.5)
    if schedule == 'const':
        return linear_end * np.ones(n_timestep, dtype=np.float64)
    if schedule == 'jsd':
        return 1. / np.linspace(n_timestep, 1, n_timestep, dtype=np.float64)
    if schedule == 'cosine':
        steps = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + cosine_s
        alphas = torch.cos(steps / (1 + cosine_s) * math.pi / 2).pow(2)
        alphas = alphas / alphas[0]
        return (1 - alphas[1:] / alphas[:-1]).clamp(max=0.999).numpy()
    raise NotImplementedError(schedule)


def draw_seed():
    """A Philox seed from torch's CPU generator (a host tensor: no device sync), for callers that pass neither noise nor seed."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class GaussianDiffusion(nn.Module):
    def __init__(self, denoise_fn, image_size, channels=3, loss_type='l2', conditional=True, schedule_opt=None, scale=4):
        super().__init__()
        self.channels, self.image_size, self.denoise_fn = channels, image_size, denoise_fn
        self.conditional, self.loss_type = conditional, loss_type
        self.num_timesteps = None                       # like the reference, the schedule is set by set_new_noise_schedule, not here

    def set_loss(self, device):
        raise NotImplementedError(_TRAINING)

    def p_losses(self, x_in, noise=None):
        raise NotImplementedError(_TRAINING)

    def forward(self, x, *args, **kwargs):
        raise NotImplementedError(_TRAINING)

    def _register(self, name, value):
        if name in self._buffers:
            self._buffers[name] = value
        else:
            self.register_buffer(name, value)

    def set_new_noise_schedule(self, schedule_opt, device):
        betas = make_beta_schedule(schedule_opt['schedule'], schedule_opt['n_timestep'], schedule_opt['linear_start'],
                                   schedule_opt['linear_end'])
        alphas = 1. - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1., ac[:-1])
        pv = betas * (1. - ac_prev) / (1. - ac)
        values = {
            'betas': betas, 'alphas_cumprod': ac, 'alphas_cumprod_prev': ac_prev, 'sqrt_alphas_cumprod': np.sqrt(ac),
            'sqrt_one_minus_alphas_cumprod': np.sqrt(1. - ac), 'log_one_minus_alphas_cumprod': np.log(1. - ac),
            'sqrt_recip_alphas_cumprod': np.sqrt(1. / ac), 'sqrt_recipm1_alphas_cumprod': np.sqrt(1. / ac - 1),
            'posterior_variance': pv, 'posterior_log_variance_clipped': np.log(np.maximum(pv, 1e-20)),
            'posterior_mean_coef1': betas * np.sqrt(ac_prev) / (1. - ac),
            'posterior_mean_coef2': (1. - ac_prev) * np.sqrt(alphas) / (1. - ac)}
        for name in SCHEDULE_BUFFERS:
            self._register(name, torch.tensor(values[name], dtype=torch.float32, device=device))
        self._adopt_schedule()

    def _adopt_schedule(self):
        """Host copies of the three per-step coefficients (passed to the kernel by value) and the sinusoid rows of every timestep."""
        self.num_timesteps = int(self.betas.shape[0])
        self._c1 = self.posterior_mean_coef1.detach().cpu().tolist()
        self._c2 = self.posterior_mean_coef2.detach().cpu().tolist()
        self._logvar = self.posterior_log_variance_clipped.detach().cpu().tolist()
        self._sinusoid = None

    def _table(self, device):
        """Sinusoid rows of every timestep, [T, model_channels] on the device: the sampler reads row i, a training step gathers by t."""
        if self._sinusoid is None or self._sinusoid.device != device:
            self._sinusoid = timestep_embedding(torch.arange(self.num_timesteps), self.denoise_fn.model_channels).to(device)
        return self._sinusoid

    def _emb_rows(self, i, b, device):
        return self._table(device)[i:i + 1].expand(b, -1).contiguous()

    def _need_schedule(self):
        if self.num_timesteps is None:
            raise RuntimeError('GaussianDiffusion: call set_new_noise_schedule(schedule_opt, device) first')

    def _uniform_t(self, t):
        ts = torch.as_tensor(t).reshape(-1).tolist()
        if any(v != ts[0] for v in ts):
            raise NotImplementedError('p_sample: one timestep for the whole batch (the sampler passes its coefficients by value)')
        return int(ts[0])

    @torch.no_grad()
    def p_sample(self, x, t, clip_denoised=True, repeat_noise=False, condition_x=None, *, noise=None, seed=None, step=0):
        """x_{t-1} from x_t [B, C, H, W].  noise: the draw to use ([B, C, H, W]); otherwise Philox draws of (seed, step)."""
        self._need_schedule()
        if not clip_denoised or repeat_noise:
            raise NotImplementedError('p_sample: clip_denoised=True and repeat_noise=False are what the sampler kernel computes')
        ops._require_gpu(x, 'gdp.p_sample')
        i = self._uniform_t(t)
        b, c, h, w = x.shape
        buf = torch.empty(b, h, w, c + (condition_x.shape[1] if condition_x is not None else 0), device=x.device, dtype=torch.float32)
        buf[..., :c] = x.permute(0, 2, 3, 1)
        if condition_x is not None:
            buf[..., c:] = condition_x.permute(0, 2, 3, 1)
        if noise is None and seed is None:
            seed = draw_seed()
        self._step(buf, c, i, None if noise is None else noise.permute(0, 2, 3, 1).contiguous(), seed or 0, step)
        return buf[..., :c].permute(0, 3, 1, 2)

    def _step(self, buf, c, i, noise_rows, seed, step):
        """One reverse step in place on channels 0..c-1 of the NHWC buffer `buf` (the U-Net input: x_t, then the condition)."""
        x0 = self.denoise_fn.forward_embedded(buf.permute(0, 3, 1, 2), self._emb_rows(i, buf.shape[0], buf.device))
        xt = buf[..., :c]
        sampler_step(x0.permute(0, 2, 3, 1), xt, xt, self._c1[i], self._c2[i], self._logvar[i], i > 0, noise_rows, seed, step)

    def _loop(self, cond, shape, noise, seed, keep):
        """The reverse chain.  cond: [B, C', H, W] condition or None; returns (final [B, C, H, W], list of kept iterates)."""
        self._need_schedule()
        b, c, h, w = shape
        steps = self.num_timesteps
        device = self.betas.device
        if noise is not None:
            if tuple(noise.shape) != (steps + 1, b, c, h, w):
                raise ValueError('noise must be [num_timesteps + 1, B, C, H, W] = %s, got %s' % ((steps + 1, b, c, h, w), tuple(noise.shape)))
            ops._require_gpu(noise, 'gdp sampler (noise)')
            noise = noise.permute(0, 1, 3, 4, 2).contiguous()
        elif seed is None:
            seed = draw_seed()
        extra = cond.shape[1] if cond is not None else 0
        buf = torch.empty(b, h, w, c + extra, device=device, dtype=torch.float32)
        if cond is not None:
            buf[..., c:] = cond.permute(0, 2, 3, 1)
        if noise is not None:
            buf[..., :c] = noise[0]
        else:
            randn_rows(buf[..., :c], seed, 0)
        inter = 1 | (steps // 10)
        kept = []
        for k, i in enumerate(reversed(range(steps))):
            self._step(buf, c, i, None if noise is None else noise[k + 1], seed or 0, k + 1)
            if keep and i % inter == 0:
                kept.append(buf[..., :c].permute(0, 3, 1, 2).clone())
        return buf[..., :c].permute(0, 3, 1, 2), kept

    @torch.no_grad()
    def p_sample_loop(self, x_in, continous=False, *, noise=None, seed=None):
        """As the reference: unconditional -> the final batch; conditional -> torch.cat([x_in, iterates...], dim 0) if `continous`,
        else that stack's last entry, i.e. the LAST IMAGE of the final batch ([C, H, W]: the reference indexes the batch-concatenated
        stack with [-1]; its validation runs with batch size 1)."""
        if not self.conditional:
            shape = tuple(x_in) if not torch.is_tensor(x_in) else tuple(x_in.shape)
            final, _ = self._loop(None, shape, noise, seed, False)
            return final
        ops._require_gpu(x_in, 'gdp.p_sample_loop')
        b, _, h, w = x_in.shape
        final, kept = self._loop(x_in, (b, self.channels, h, w), noise, seed, continous)
        if continous:
            return torch.cat([x_in] + kept, dim=0)
        return final[-1]

    @torch.no_grad()
    def sample(self, batch_size=1, continous=False, *, noise=None, seed=None):
        return self.p_sample_loop((batch_size, self.channels, self.image_size, self.image_size), continous, noise=noise, seed=seed)

    @torch.no_grad()
    def super_resolution(self, x_in, continous=False, *, noise=None, seed=None):
        return self.p_sample_loop(x_in, continous, noise=noise, seed=seed)

    @torch.no_grad()
    def super_resolution_batch(self, x_in, *, noise=None, seed=None):
        """The final iterate of every image of the batch, [B, C, H, W] (super_resolution returns one image, see p_sample_loop)."""
        ops._require_gpu(x_in, 'gdp.super_resolution_batch')
        b, _, h, w = x_in.shape
        return self._loop(x_in, (b, self.channels, h, w), noise, seed, False)[0]

    def interpolate(self, *args, **kwargs):
        raise NotImplementedError('interpolate is not built')


def build_G(opt, unet, diffusion):
    """The reference's networks.define_G for which_model_G = 'gdp', over the classes `unet` and `diffusion`: only the arguments it
    passes reach the U-Net, everything else (128 base channels, heads of 64, attention at 8x down-sampling) is UNet's default."""
    m = opt['model']
    if m['which_model_G'] != 'gdp':
        raise NotImplementedError("which_model_G=%r: only 'gdp' is built (the reference ships no ddpm module)" % m['which_model_G'])
    u = m['unet']
    model = unet(in_channel=u['in_channel'], out_channel=u['out_channel'], norm_groups=u.get('norm_groups') or 32,
                 inner_channel=u['inner_channel'], channel_mults=u['channel_multiplier'], attn_res=u['attn_res'],
                 res_blocks=u['res_blocks'], dropout=u['dropout'], image_size=m['diffusion']['image_size'])
    return diffusion(model, image_size=m['diffusion']['image_size'], channels=m['diffusion']['channels'], loss_type='l2',
                     conditional=m['diffusion']['conditional'], schedule_opt=m['beta_schedule']['train'])


def define_G(opt):
    return build_G(opt, UNet, GaussianDiffusion)


def load_gen(netG, path):
    """Load a reference `I*_E*_gen.pth` (the GaussianDiffusion state dict: `denoise_fn.*` and, when it was saved after
    set_new_noise_schedule, the schedule buffers) strictly.  `path` may be the state dict itself.  A schedule in the file is adopted
    when netG has none yet; call set_new_noise_schedule afterwards to sample on another one, as the reference's validation does."""
    state = torch.load(path, map_location='cpu') if not isinstance(path, dict) else path
    state = dict(state)
    have = [k for k in SCHEDULE_BUFFERS if k in state]
    if have and netG.num_timesteps is None:
        if len(have) != len(SCHEDULE_BUFFERS):
            raise KeyError('load_gen: the file holds only part of the schedule buffers: %s' % have)
        device = next(netG.denoise_fn.parameters()).device
        for k in SCHEDULE_BUFFERS:
            netG._register(k, torch.empty(state[k].shape, dtype=torch.float32, device=device))
    elif not have and netG.num_timesteps is not None:
        for k in SCHEDULE_BUFFERS:
            state[k] = getattr(netG, k)
    netG.load_state_dict(state, strict=True)
    if have and netG.betas.device.type != 'meta':
        netG._adopt_schedule()
    return netG


def gdp_super_resolve(netG, lr_u8, out_size, *, noise=None, seed=None):
    """sr_mfe.py's validation path on the device: uint8 LR tiles [N, h, w, 3] -> Pillow-exact bicubic to out_size x out_size (the
    dataset's `SR` image) -> to_tensor * 2 - 1 -> the sampler conditioned on it -> tensor2img(min_max=(-1, 1)): uint8 [N, H, W, 3]."""
    if not torch.is_tensor(lr_u8) or lr_u8.dtype != torch.uint8 or lr_u8.dim() != 4:
        raise TypeError('gdp_super_resolve expects a [N, h, w, 3] uint8 tensor')
    if not lr_u8.is_cuda:
        raise RuntimeError('gdp_super_resolve: runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback'
                           % lr_u8.device.type)
    cond = sdata.to_tensor(sdata.resize_u8(lr_u8, out_size, out_size)) * 2.0 + (-1.0)
    final = netG.super_resolution_batch(cond, noise=noise, seed=seed)
    return quantize_u8(final.permute(0, 2, 3, 1))
