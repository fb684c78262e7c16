"""fp64 references (plain torch, no kernels) of the reductions around the convolutions -- train-mode BatchNorm + LeakyReLU with its
first- and second-order backward, column sums, the loss reductions, Adam -- the error measure and bound of their GPU tests, and the
input generators those tests use.  The metric arithmetic (MSE / PSNR / ERGAS / SSIM on uint8) is oracle/sradsgan_ref.py's numpy
restatement, re-exported here.

Every tensor that reaches a kernel is [rows][C] (NHWC with the pixels flattened), so the references are written on 2-d tensors."""
import math

import torch
import torch.nn.functional as F

from oracle.sradsgan_ref import ergas2, mse_u8, psnr_u8, ssim_u8, to_uint8_hwc  # noqa: F401  (the metric reference)

FLOOR = 32 * 2.0 ** -24      # a handful of fp32 roundings: keeps a case where torch happens to be exact from failing on a last bit
FACTOR = 8.0                 # a different but sound summation order (slabs of 64 rows against torch's cascade)


def err(got, ref):
    """max|got - ref64| / max(|ref64|.max(), tiny) of one output tensor."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def bound(torch_err):
    """The bar of one output tensor: 8 x the error of stock fp32 torch on the same inputs, never below FLOOR."""
    return max(FACTOR * torch_err, FLOOR)


# --------------------------------------------------------------------------------------------- #
# BatchNorm (+ LeakyReLU), x: [rows][C]
# --------------------------------------------------------------------------------------------- #


def _slopes(mask, slope, like):
    if slope is None:
        return torch.ones_like(like)
    return torch.where(mask, torch.ones_like(like), torch.full_like(like, float(slope)))


def bn_fwd_ref(x, gamma, beta, running_mean, running_var, eps, momentum, slope):
    """Train-mode forward in fp64: normalisation by the biased variance, running update by the unbiased one (rows = 1: the biased
    one, as the kernel documents).  Returns a dict of fp64 tensors; running_* are None when no running pair is given."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    rows = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = (x - mean) * invstd * gamma + beta
    y = pre if slope is None else torch.where(pre > 0, pre, pre * slope)
    out = dict(mean=mean, invstd=invstd, y=y, running_mean=None, running_var=None)
    if running_mean is not None:
        unb = var * (rows / (rows - 1.0)) if rows > 1 else var
        out['running_mean'] = (1 - momentum) * running_mean.double() + momentum * mean
        out['running_var'] = (1 - momentum) * running_var.double() + momentum * unb
    return out


def bn_eval_ref(x, gamma, beta, running_mean, running_var, eps, slope):
    pre = (x.double() - running_mean.double()) / torch.sqrt(running_var.double() + eps) * gamma.double() + beta.double()
    return pre if slope is None else torch.where(pre > 0, pre, pre * slope)


def bn_bwd_ref(dy, x, gamma, mask, eps, slope, addend=None):
    """First-order backward in closed form, fp64.  mask: the LeakyReLU mask (y > 0) as the caller observed it -- a pre-activation
    within fp32 rounding of zero legitimately lands on either side, and one flipped element moves dgamma / dbeta by O(1 / rows).
    Returns dx (+ addend), dgamma, dbeta."""
    dy, x, gamma = dy.double(), x.double(), gamma.double()
    rows = x.shape[0]
    mean = x.mean(0)
    invstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(0) + eps)
    xhat = (x - mean) * invstd
    dz = dy * _slopes(mask, slope, dy)
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    dx = gamma * invstd * (dz - dbeta / rows - xhat * dgamma / rows)
    if addend is not None:
        dx = dx + addend.double()
    return dx, dgamma, dbeta


def bn_bwd2_ref(u, dy, x, gamma, mask, eps, slope):
    """Second-order backward in closed form, fp64: the gradients of <u, dx(dy, x, gamma)> at dy, x and gamma, where dx is the
    first-order backward above, differentiated through the batch statistics; the mask is a constant.  With E = mean over rows,
    a = gamma invstd, ubar = E[u], w = E[u xhat], p = E[dz], q = E[dz xhat], T = E[u dz] - ubar p - w q:
        g_dy = a (u - ubar - xhat w) lrelu',   g_x = -gamma invstd^2 [q (u - ubar) + w (dz - p) + xhat (T - 2 w q)],
        g_gamma = invstd rows T."""
    u, dy, x, gamma = u.double(), dy.double(), x.double(), gamma.double()
    rows = x.shape[0]
    mean = x.mean(0)
    invstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(0) + eps)
    xhat = (x - mean) * invstd
    mk = _slopes(mask, slope, dy)
    dz = dy * mk
    ubar, w, p, q = u.mean(0), (u * xhat).mean(0), dz.mean(0), (dz * xhat).mean(0)
    T = (u * dz).mean(0) - ubar * p - w * q
    g_dy = gamma * invstd * (u - ubar - xhat * w) * mk
    g_x = -gamma * invstd * invstd * (q * (u - ubar) + w * (dz - p) + xhat * (T - 2 * w * q))
    g_gamma = invstd * rows * T
    return g_dy, g_x, g_gamma


def bn_autograd(x, gamma, beta, dy, u, eps, slope, dtype, addend=None, running_mean=None, running_var=None, momentum=0.1):
    """The same quantities from stock torch under autograd in `dtype` (the batch_norm F.batch_norm dispatches to, which also hands
    out its saved statistics, + F.leaky_relu; the first-order backward with create_graph; then the backward of <u, dx>): fp32 = the
    error yardstick of the GPU tests, fp64 = the check of the closed forms.  Returns a dict with y, mask (torch's own y > 0), mean,
    invstd, running_mean / running_var (updated copies; from zeros / ones when not given), dx (+ addend), dgamma, dbeta, g_dy, g_x,
    g_gamma."""
    c = x.shape[1]
    xx, gg, bb = x.to(dtype).requires_grad_(), gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    dyy = dy.to(dtype).requires_grad_()
    rm = torch.zeros(c, dtype=dtype) if running_mean is None else running_mean.to(dtype).clone()
    rv = torch.ones(c, dtype=dtype) if running_var is None else running_var.to(dtype).clone()
    pre, mean, invstd = torch.native_batch_norm(xx, gg, bb, rm, rv, True, momentum, eps)
    y = pre if slope is None else F.leaky_relu(pre, slope)
    dx, dgamma, dbeta = torch.autograd.grad(y, [xx, gg, bb], dyy, create_graph=True)
    g_dy, g_x, g_gamma = torch.autograd.grad((dx * u.to(dtype)).sum(), [dyy, xx, gg])
    out = dict(y=y, mask=y > 0, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma, dbeta=dbeta,
               g_dy=g_dy, g_x=g_x, g_gamma=g_gamma)
    if addend is not None:
        out['dx'] = dx + addend.to(dtype)
    return {k: v.detach() for k, v in out.items()}


BN_FAMILIES = ('normal', 'mean100', 'corner3', 'corner10', 'constant_channel', 'gamma_signs')
CONSTANT_CHANNEL = 1        # which channel 'constant_channel' freezes
GAMMA_NEGATIVE, GAMMA_ZERO = 0, 2


def bn_inputs(family, rows, c, seed=0):
    """fp32 inputs of one BatchNorm case: x, gamma, beta, dy, u (the second-order cotangent), addend, acc_gamma, acc_beta (seeds of
    the accumulating entry points), running_mean, running_var.
      normal            N(0, 1)
      mean100           mean 100, std 0.01
      corner3/corner10  row 0 = 0 (the zero-padded image corner), every other row 3 +- 0.05 / 10 +- 0.05
      constant_channel  N(0, 1) with channel CONSTANT_CHANNEL constant (zero variance)
      gamma_signs       N(0, 1), gamma[GAMMA_NEGATIVE] < 0 and gamma[GAMMA_ZERO] = 0"""
    g = torch.Generator().manual_seed(1000 * seed + rows + 7 * c + 13 * BN_FAMILIES.index(family))
    x = torch.randn(rows, c, generator=g)
    if family == 'mean100':
        x = 100.0 + 0.01 * x
    elif family in ('corner3', 'corner10'):
        x = (3.0 if family == 'corner3' else 10.0) + 0.05 * (2 * torch.rand(rows, c, generator=g) - 1)
        x[0] = 0.0
    elif family == 'constant_channel':
        x[:, CONSTANT_CHANNEL] = 0.625
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    if family == 'gamma_signs':
        gamma[GAMMA_NEGATIVE] = -0.75
        gamma[GAMMA_ZERO] = 0.0
    t = dict(x=x, gamma=gamma, beta=beta, dy=torch.randn(rows, c, generator=g), u=torch.randn(rows, c, generator=g),
             addend=torch.randn(rows, c, generator=g), acc_gamma=torch.randn(c, generator=g), acc_beta=torch.randn(c, generator=g),
             running_mean=0.5 * torch.randn(c, generator=g), running_var=0.5 + torch.rand(c, generator=g))
    return t


# --------------------------------------------------------------------------------------------- #
# column sums and loss reductions
# --------------------------------------------------------------------------------------------- #


def colsum_ref(m):
    """m: [rows][C] -> fp64 [C]."""
    return m.double().sum(0)


def l1_ref(a, b, gout):
    """Returns (loss, da, db) of gout * mean|a - b| in fp64 (sign(0) = 0 like torch)."""
    d = a.double() - b.double()
    da = torch.sign(d) * (gout / d.numel())
    return d.abs().mean(), da, -da


def mse_ref(a, b, gout):
    d = a.double() - b.double()
    da = 2 * d * (gout / d.numel())
    return (d * d).mean(), da, -da


def smooth_l1_ref(a, b, gout):
    """b: a tensor or a python scalar target (then db is None).  beta = 1: |d| < 1 ? d^2 / 2 : |d| - 1/2."""
    scalar = not torch.is_tensor(b)
    d = a.double() - (b if scalar else b.double())
    z = d.abs()
    loss = torch.where(z < 1, 0.5 * z * z, z - 0.5).mean()
    da = d.clamp(-1, 1) * (gout / d.numel())
    return loss, da, (None if scalar else -da)


def mean_ref(x, gout):
    x = x.double()
    return x.mean(), torch.full_like(x, gout / x.numel())


def gp_ref(g, gout):
    """g: [npix][C].  mean over pixels of (||g_pixel||_2 - 1)^2; its gradient is 0 at a zero-norm pixel (torch's norm backward)."""
    g = g.double()
    nrm = g.pow(2).sum(1).sqrt()
    loss = ((nrm - 1) ** 2).mean()
    f = torch.where(nrm > 0, 2 * (nrm - 1) / nrm.clamp_min(1e-300), torch.zeros_like(nrm)) * (gout / g.shape[0])
    return loss, f[:, None] * g


def loss_inputs(count, seed=0):
    """A pair of flat fp32 tensors for the two-tensor losses.  Where the count allows: an exact d = 0 entry and exact d = +1 / d = -1
    entries (the kink of SmoothL1 and of |d|), |d| both below and above 1 elsewhere."""
    g = torch.Generator().manual_seed(77 + count + 1000 * seed)
    a = 1.5 * torch.randn(count, generator=g)
    b = 1.5 * torch.randn(count, generator=g)
    if count >= 5:
        b[0] = a[0]                                   # d = 0
        a[count // 2], b[count // 2] = 0.25, -0.75    # d = +1, exactly
        a[count - 1], b[count - 1] = -0.5, 0.5        # d = -1, exactly (in the scalar tail when count % 4 != 0)
    return a, b


def scalar_target_inputs(count, target, seed=0):
    """A flat fp32 tensor for SmoothL1 against a scalar target, with exact d = 0 and |d| = 1 entries where the count allows."""
    g = torch.Generator().manual_seed(91 + count + 1000 * seed)
    a = target + 1.5 * torch.randn(count, generator=g)
    if count >= 5:
        a[0] = target
        a[count // 2] = target + 1.0
        a[count - 1] = target - 1.0
    return a


def gp_inputs(npix, c, seed=0):
    """[npix][C] gradient 'image' with norms around 1; one zero-norm pixel (the last one) when npix > 1."""
    g = torch.Generator().manual_seed(55 + npix + 10 * c + 1000 * seed)
    t = torch.randn(npix, c, generator=g) / math.sqrt(c) * (0.5 + torch.rand(npix, 1, generator=g))
    if npix > 1:
        t[npix - 1] = 0.0
    return t


# --------------------------------------------------------------------------------------------- #
# Adam
# --------------------------------------------------------------------------------------------- #


def adam_ref(p, grads, lr, b1, b2, eps, grad_scale, clip):
    """fp64 Adam recurrences in torch.optim.Adam's order of operations (single-tensor form: lerp, mul + addcmul, bias corrections,
    denom = sqrt(v) / sqrt(bc2) + eps, addcdiv), the gradient multiplied by grad_scale first, p clamped to +- clip afterwards when
    clip > 0.  Returns the state after every step: [(p, m, v, [step, lr / (1 - b1^step), sqrt(1 - b2^step)]), ...]."""
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for step, g in enumerate(grads, 1):
        g = g.double() * grad_scale
        m = m + (g - m) * (1 - b1)
        v = v * b2 + (1 - b2) * g * g
        step_size = lr / (1 - b1 ** step)
        bc2_sqrt = math.sqrt(1 - b2 ** step)
        p = p - step_size * (m / (v.sqrt() / bc2_sqrt + eps))
        if clip > 0:
            p = p.clamp(-clip, clip)
        out.append((p.clone(), m.clone(), v.clone(), [float(step), step_size, bc2_sqrt]))
    return out


# hyper-parameters that fp32 holds exactly: the entry point takes them as floats, and 1 - b2 formed from a rounded 0.999 would be a
# difference of the INPUTS (1.3e-5 of v), not of the kernel's arithmetic
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 2.0 ** -12, 0.875, 1 - 2.0 ** -8, 2.0 ** -27


def adam_stock(p0, grads, clip, dtype, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """torch.optim.Adam on the CPU in `dtype`, then p.data.clamp_(-clip, clip) when clip > 0 (sradsgan.py:891-892).  Returns
    [(p, exp_avg, exp_avg_sq) after each step]."""
    q = p0.to(dtype).clone().requires_grad_()
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    steps = []
    for g in grads:
        q.grad = g.to(dtype).clone()
        opt.step()
        if clip > 0:
            q.data.clamp_(-clip, clip)
        steps.append((q.detach().clone(), opt.state[q]['exp_avg'].clone(), opt.state[q]['exp_avg_sq'].clone()))
    return steps


ADAM_GRAD_SCALES = (1.0, 1e-3, 1e-6, 0.0, 1.0)     # per step
ADAM_FROZEN = 1000                                  # the first elements never receive a gradient: m = v = 0, denominator = eps


def adam_inputs(n, seed=0):
    """p [n] ~ N(0, 0.04) and one gradient per step of ADAM_GRAD_SCALES; the first ADAM_FROZEN gradient entries are 0 in every step."""
    g = torch.Generator().manual_seed(31 + 1000 * seed)
    p = 0.04 * torch.randn(n, generator=g)
    grads = []
    for s in ADAM_GRAD_SCALES:
        t = torch.randn(n, generator=g) * s
        t[:ADAM_FROZEN] = 0.0
        grads.append(t)
    return p, grads
