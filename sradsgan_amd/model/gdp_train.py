"""GDP diffusion super-resolution, training: the reference's `GDP_x0/model/model.py` (DDPM) and the training half of
`gdp_modules/diffusion.py` (set_loss, q_sample, p_losses) on the HIP kernels.  model/gdp.py stays the sampler: its classes keep their
parameters frozen and refuse to train; the classes here derive from them, share their module tree and state-dict keys, and add the
backward pass.

  TrainableUNet      gdp.UNet with parameters that require grad.  With grad enabled it runs gdp.UNet's one walk (ops.conv2d /
                     ops.linear, ops.cat_channels, ops.upsample_nearest and the differentiable kernels of model/gdp_kernels.py), so
                     its output has the bits of gdp.UNet.forward_embedded; without grad it IS that forward.  Conv arithmetic `half` is
                     replaced by `bf16x3` for forward and backward alike (_HoldConvMath).
  TrainableDiffusion set_loss, q_sample (srhip_diff_q_sample writes x_t into channels 0..2 of the U-Net input, gathering the schedule
                     coefficients by the device tensor t) and p_losses (sum-reduced, as the reference's reduction='sum').
  DDPM               the reference's model surface: feed_data, optimize_parameters (dp.ParamArena.adam_step, no host sync in
                     the step), test / sample, save_network / load_network in the reference's file layout.
  training_batch     uint8 HR tiles -> {'HR', 'SR', 'LR'} as prepare_data.py + LRHR_dataset.py make them.

Not built: dropout != 0, finetune_norm, EMA, nn.DataParallel, hipGraph capture."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.autograd import Function

from .. import data as sdata, dp, ops
from . import gdp
from .gdp_kernels import (attention_bwd_raw, attention_fwd_lse, avg_pool2x2, avg_pool2x2_bwd, group_norm_act,  # noqa: F401
                          group_norm_bwd_raw, group_norm_fwd_raw, q_sample_rows, qkv_attention, silu)

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


# ------------------------------------------------------------------------------------------------------------------------------ #
# the U-Net with a backward pass: gdp.UNet's walk, run with grad enabled
# ------------------------------------------------------------------------------------------------------------------------------ #
def _thaw(net):
    """Parameters require grad and join the per-step batched re-pack (ops.mark_trainable)."""
    for p in net.parameters():
        p.requires_grad_(True)
    ops.mark_trainable(net)


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

    def forward_embedded(self, x, emb_in):
        if not torch.is_grad_enabled():
            return super().forward_embedded(x, emb_in)
        if ops.get_conv_math() == 'half':                # as the sampler: the U-Net is outside the 16-bit contract, forward AND backward
            with ops.conv_math('bf16x3'):
                y = self._walk(x, emb_in)
            return _HoldConvMath.apply(y, 'bf16x3')
        return self._walk(x, emb_in)

    def forward(self, x, timesteps, y=None):
        if not torch.is_grad_enabled():
            return super().forward(x, timesteps, y)
        return self.forward_embedded(ops.nhwc(x), self._checked_rows('gdp_train.TrainableUNet', x, timesteps, y))


# ------------------------------------------------------------------------------------------------------------------------------ #
# p_losses
# ------------------------------------------------------------------------------------------------------------------------------ #
class TrainableDiffusion(gdp.GaussianDiffusion):
    def set_loss(self, device):
        if self.loss_type not in ('l1', 'l2'):
            raise NotImplementedError('loss_type=%r: l1 and l2 are what the reference names' % (self.loss_type,))
        self.loss_kind = self.loss_type

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
            seed = gdp.draw_seed()
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
    return gdp.build_G(opt, TrainableUNet, TrainableDiffusion)


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
        a.adam_step(self.lr, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS)
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


def training_batch(hr_u8, lr_size, augment=None):
    """uint8 HR tiles [N, H, W, 3] on the device -> {'HR', 'SR', 'LR'} float32 in [-1, 1] as prepare_data.py (Pillow bicubic down to
    lr_size, then back up to H x W) and LRHR_dataset.py (to_tensor * 2 - 1) make them.  augment: a data.Augment applied to the tiles
    first (crop to its crop size, noise, rotation, flips); None = the tiles as they are."""
    if not torch.is_tensor(hr_u8) or hr_u8.dtype != torch.uint8 or hr_u8.dim() != 4:
        raise TypeError('training_batch expects a [N, H, W, 3] uint8 tensor')
    if not hr_u8.is_cuda:
        raise RuntimeError('training_batch: runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback' % hr_u8.device.type)
    if augment is not None:
        hr_u8 = augment(hr_u8)
    _, h, w, _ = hr_u8.shape
    lr = sdata.resize_u8(hr_u8, lr_size, lr_size)
    sr = sdata.resize_u8(lr, h, w)
    return {k: sdata.to_tensor(v) * 2.0 + (-1.0) for k, v in (('HR', hr_u8), ('SR', sr), ('LR', lr))}
