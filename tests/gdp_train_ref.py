"""Restatement of the GDP diffusion training step on the CPU, on top of tests/gdp_ref.py: the forward diffusion, p_losses with its
gradients by autograd (float64 = the tests' reference, float32 = their error floor), plain-formula references of the single kernels,
and the gradient score of tests/test_hat_gpu.py.  Nothing here imports the product package."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import gdp_ref as R

TRAIN_SCHEDULE = dict(schedule='linear', n_timestep=1000, linear_start=1e-4, linear_end=2e-2)      # the reference's train schedule
TRAIN_T = (3, 500)
TRAIN_SEED = 4321                      # tools/make_golden_gdp_train.py: torch.manual_seed before the reference's p_losses
DIGEST = dict(full_max=512, nsample=256)
LR_ADAM = 1e-4


def train_inputs():
    """(HR, SR) in [-1, 1], [2, 3, 12, 12] each: the condition is the small net's usual one."""
    from oracle import sradsgan_ref as O
    return O.det_fill('gdp.train.hr', (2, 3, 12, 12), 1.0), R.small_input()[:, 3:].contiguous()


def step_inputs(k):
    """(t, noise) of training step k of the trajectory tests."""
    from oracle import sradsgan_ref as O
    t = [(3, 500), (999, 0), (250, 700), (41, 42)][k]
    return torch.tensor(t, dtype=torch.long), O.det_fill('gdp.train.noise.%d' % k, (2, 3, 12, 12), 1.7)


def q_coefficients(sched):
    """float32 sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod), as the model's buffers hold them."""
    betas = R.betas64(sched['schedule'], sched['n_timestep'], sched['linear_start'], sched['linear_end'])
    ac = np.cumprod(1.0 - betas)
    return torch.from_numpy(np.sqrt(ac).astype(np.float32)), torch.from_numpy(np.sqrt(1.0 - ac).astype(np.float32))


def q_sample(x0, t, noise, sched):
    a, b = q_coefficients(sched)
    dt = x0.dtype
    return a[t].to(dt).reshape(-1, 1, 1, 1) * x0 + b[t].to(dt).reshape(-1, 1, 1, 1) * noise


def p_losses(sd, hr, sr, t, noise, cfg=R.SMALL, sched=TRAIN_SCHEDULE, loss='l2', prefix=''):
    """Sum-reduced loss of the x0-predicting U-Net on q_sample(hr, t, noise) conditioned on sr (sr=None: unconditional), in the dtype
    of hr; differentiable in the entries of sd."""
    xt = q_sample(hr, t, noise.to(hr.dtype), sched)
    x = xt if sr is None else torch.cat([xt, sr], dim=1)
    recon = R.unet_forward(sd, x, t, cfg, prefix)
    return (recon - hr).abs().sum() if loss == 'l1' else ((recon - hr) ** 2).sum()


def loss_and_grads(state, hr, sr, t, noise, dtype=torch.float64, **kw):
    """(loss / numel as float, {key: gradient of loss / numel}) with the parameters `state` cast to dtype."""
    sd = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    cast = lambda v: None if v is None else v.detach().cpu().to(dtype)
    loss = p_losses(sd, cast(hr), cast(sr), t.cpu(), cast(noise), **kw) / hr.numel()
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}


def digest_score(grads, fixture, prefix='grad.'):
    """grad_score of {key: gradient} against the digests stored in the fixture (O.digest(g, **DIGEST)): the sampled values only, the
    trailing [sum, norm] of a large tensor's digest is left out (another scale)."""
    from oracle import sradsgan_ref as O
    got, want = {}, {}
    for k, g in grads.items():
        d, w = O.digest(g, **DIGEST), np.asarray(fixture[prefix + k])
        assert d.shape == w.shape, k
        n = d.size - 2 if g.numel() > DIGEST['full_max'] else d.size
        got[k], want[k] = torch.from_numpy(d[:n].astype(np.float64)), torch.from_numpy(w[:n].astype(np.float64))
    return grad_score(got, want)


def grad_score(got, want):
    """worst |dg| over max(|g| of the parameter, 1e-2 |g| of the network) (tests/test_hat_gpu.py); got / want: {key: gradient}"""
    gnet = max(float(want[k].abs().max()) for k in want)
    worst, wk = 0.0, None
    for k, g in want.items():
        d = float((got[k].detach().cpu().double() - g.detach().cpu().double()).abs().max())
        s = d / max(float(g.abs().max()), 1e-2 * gnet)
        if s > worst:
            worst, wk = s, k
    return worst, wk


# ---- single kernels: the plain formulas, differentiated by autograd -------------------------------------------------------------- #
def gn_act(x, gamma, beta, scale, shift, act):
    """x [n, p, C] -> GroupNorm(32, C), * (1 + scale) + shift (scale / shift [n, C] or None), SiLU if act."""
    y = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1)
    if scale is not None:
        y = y * (1 + scale[:, None]) + shift[:, None]
    return F.silu(y) if act else y


def gn_act_grads(x, gamma, beta, scale, shift, act, dy, dtype):
    """(dx, dgamma, dbeta, dscale, dshift) of sum(gn_act(...) * dy) in dtype (the last two None without modulation)."""
    leaves = [None if v is None else v.detach().to(dtype).clone().requires_grad_(True) for v in (x, gamma, beta, scale, shift)]
    (gn_act(*leaves, act) * dy.to(dtype)).sum().backward()
    return [None if v is None else v.grad for v in leaves]


def attention_grad(qkv, heads, dout, dtype):
    """(out, lse [n, heads, t], dqkv) of R.attention on qkv [n, t, heads * 3 * ch] rows, cotangent dout [n, t, heads * ch]."""
    leaf = qkv.detach().to(dtype).clone().requires_grad_(True)
    out = R.attention(leaf.permute(0, 2, 1), heads).permute(0, 2, 1)
    (out * dout.to(dtype)).sum().backward()
    n, t, width = qkv.shape
    ch = width // (3 * heads)
    per_head = leaf.detach().permute(0, 2, 1).reshape(n, heads, 3, ch, t)
    logits = torch.matmul((per_head[:, :, 0] / float(ch) ** 0.25).transpose(2, 3), per_head[:, :, 1] / float(ch) ** 0.25)
    return out.detach(), torch.logsumexp(logits, dim=3), leaf.grad
