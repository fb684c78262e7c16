"""LPIPS as a loss, restated with stock torch ops over tests/lpips_ref.py's `taps`: the batch mean of the distances, differentiable by
autograd in any dtype, and the closed form of one head's gradient that csrc/lpips.hip's head backward evaluates.

The root is written so that an all-zero pixel gives 0, not NaN: sqrt has an infinite slope at 0, and autograd multiplies it with the zero
gradient of the sum of squares.  `safe_norm` feeds the root 1 where the sum is 0 and selects 0 afterwards, so that pixel's features get a
zero gradient from the normalisation -- which is also what the kernels write."""
import torch

from tests import lpips_ref as R

EPS = 1e-10


def safe_norm(f):
    """sqrt(sum_c f^2) [N,1,h,w] whose gradient at an all-zero pixel is 0."""
    s = (f * f).sum(1, keepdim=True)
    live = s > 0
    return torch.where(live, torch.sqrt(torch.where(live, s, torch.ones_like(s))), torch.zeros_like(s))


def head(f0, f1, w):
    """R.head with the safe root: [N] (mean over pixels)."""
    n0 = f0 / (safe_norm(f0) + EPS)
    n1 = f1 / (safe_norm(f1) + EPS)
    return (((n0 - n1) ** 2) * w.to(n0.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def loss(pred, target, sd, lin, dtype=torch.float64, normalize=True, conv=None):
    """Batch mean of the LPIPS distances, a 0-d tensor of `dtype`; differentiable in pred."""
    t0 = R.taps(target.to(dtype), sd, normalize, conv)
    t1 = R.taps(pred.to(dtype), sd, normalize, conv)
    vals = torch.stack([head(a, b, torch.as_tensor(w).flatten()) for a, b, w in zip(t0, t1, lin)])
    return vals.sum(0).mean()


def loss_and_grad(pred, target, sd, lin, dtype=torch.float64, normalize=True, conv=None):
    """(loss, d loss / d pred) by autograd in `dtype`."""
    p = pred.detach().to(dtype).requires_grad_(True)
    val = loss(p, target, sd, lin, dtype, normalize, conv)
    g, = torch.autograd.grad(val, p)
    return val.detach(), g


class _EmulatedConv(torch.autograd.Function):
    """A stride-1 conv whose forward and data gradient are conv_emulation's contraction in `arith` (operands rounded as the kernels round
    them, exact accumulation), returned in x's dtype.  The data gradient of a stride-1 conv is a forward conv of dy with the weights
    flipped and transposed, pad k - 1 - pad, so conv_fwd serves both ways."""

    @staticmethod
    def forward(ctx, x, w, b, pad, arith):
        from tests import conv_emulation as E
        ctx.w, ctx.pad, ctx.arith = w, pad, arith
        y = E.conv_fwd(x.detach(), w, 1, pad, arith=arith, with_abs=False)[0] + b.double().view(1, -1, 1, 1)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        from tests import conv_emulation as E
        wt = ctx.w.flip(2, 3).transpose(0, 1).contiguous()
        dx = E.conv_fwd(dy, wt, 1, ctx.w.shape[2] - 1 - ctx.pad, arith=ctx.arith, with_abs=False)[0]
        return dx.to(dy.dtype), None, None, None, None


def emulated_conv(arith):
    """conv(x, w, b, stride, pad) for R.taps' convs 2-5 (all stride 1), differentiable in x."""
    def conv(x, w, b, stride, pad):
        assert stride == 1
        return _EmulatedConv.apply(x, w, b, pad, arith)
    return conv


def head_grad_autograd(f, t, w, s):
    """d (s * sum over pixels and channels of w (f/D - t/D_t)^2) / d f by autograd in f's dtype, through a ReLU in front of f: the
    gradient is 0 where f <= 0."""
    pre = f.detach().clone().requires_grad_(True)
    fr = torch.relu(pre)
    e = fr / (safe_norm(fr) + EPS) - t / (safe_norm(t) + EPS)
    val = s * ((e * e) * w.to(f.dtype).view(1, -1, 1, 1)).sum()
    g, = torch.autograd.grad(val, pre)
    return g


def head_grad_closed_form(f, t, w, s):
    """The kernel's formula: n = sqrt(sum f^2), D = n + eps, e_c = f_c / D - t_c / D_t, q_c = 2 w_c e_c s, S = sum_c q_c f_c,
    df_c = q_c / D - f_c S / (D^2 n); 0 where f_c <= 0 and at pixels with n == 0 (no 0 / 0 is formed)."""
    n = torch.sqrt((f * f).sum(1, keepdim=True))
    d = n + EPS
    dt = torch.sqrt((t * t).sum(1, keepdim=True)) + EPS
    q = 2 * w.to(f.dtype).view(1, -1, 1, 1) * (f / d - t / dt) * s
    big_s = (q * f).sum(1, keepdim=True)
    live = n > 0
    n1 = torch.where(live, n, torch.ones_like(n))
    df = q / d - f * big_s / (d * d * n1)
    return torch.where(live & (f > 0), df, torch.zeros_like(df))
