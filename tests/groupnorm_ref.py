"""fp64 references (plain torch, no kernels) of the per-sample normalisations of gn.hip -- instance norm and the reference's own
GroupNorm (base_networks.py:12-31), each followed by LeakyReLU -- with their first- and second-order backward, and the same
quantities from stock torch autograd in a chosen dtype (fp32: the error yardstick of the GPU test; fp64: the check of the closed
forms).  Mirrors bn_*_ref / bn_autograd of tests/reduction_ref.py, whose error measure, bound and input families are used as they are.

Tensors are x[n][p][c] (NHWC with the pixels flattened).  `groups` groups of cpg = c / groups adjacent channels; one statistic is
taken over the m = p * cpg elements of one (sample, group).  k = m / (m - 1) for the unbiased variance, 1 for the biased one."""
import torch
import torch.nn.functional as F

from tests import reduction_ref as R

GN_SHAPES = [(1, 2, 4, 4, 0),            # one float4, m = 2
             (3, 1, 64, 32, 1),          # p = 1, m = 2: the smallest unbiased case
             (2, 65, 64, 64, 0), (2, 65, 64, 32, 1),
             (3, 197, 192, 32, 1),       # cpg = 6: groups straddle float4s; 197 = 14^2 + 1: slabs cannot divide a sample
             (2, 4, 512, 32, 1), (2, 4, 512, 512, 0),      # block 8 at a 32 x 32 input
             (2, 5, 1024, 32, 1),        # one row lane per block
             (64, 4, 128, 32, 1),        # many samples, tiny extents
             (2, 2053, 64, 32, 1),       # several slabs per sample, a ragged last one
             (1, 11664, 64, 64, 0)]      # one real 108 x 108 layer of one sample
GN_ALL_FAMILIES = [(2, 65, 64, 32, 1), (3, 197, 192, 32, 1), (2, 2053, 64, 64, 0)]
GN_CASES = [('normal',) + s for s in GN_SHAPES if s not in GN_ALL_FAMILIES] + [(f,) + s for s in GN_ALL_FAMILIES for f in R.BN_FAMILIES]


def gn_inputs(family, n, p, c):
    """reduction_ref.bn_inputs(family, n * p, c) with the [rows][C] tensors reshaped to [n][p][C]."""
    t = R.bn_inputs(family, n * p, c)
    return {k: (v.reshape(n, p, c) if v.dim() == 2 else v) for k, v in t.items()}


def _k(p, c, groups, unbiased):
    m = p * (c // groups)
    return m / (m - 1.0) if unbiased else 1.0


def _E(t, groups):
    """mean over one (sample, group), broadcast back to [n][p][c]."""
    n, p, c = t.shape
    e = t.reshape(n, p, groups, c // groups).mean((1, 3), keepdim=True)
    return e.expand(n, p, groups, c // groups).reshape(n, p, c)


def _affine(x, gamma, beta):
    c = x.shape[2]
    gamma = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double().reshape(c)
    beta = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double().reshape(c)
    return gamma, beta


def _stats(x, groups, unbiased, eps):
    n, p, c = x.shape
    mean = _E(x, groups)
    var = _k(p, c, groups, unbiased) * _E((x - mean) ** 2, groups)
    return mean, 1.0 / torch.sqrt(var + eps)


def _slopes(mask, slope, like):
    if slope is None:
        return torch.ones_like(like)
    return torch.where(mask, torch.ones_like(like), torch.full_like(like, float(slope)))


def gn_fwd_ref(x, gamma, beta, groups, unbiased, eps, slope):
    """Forward in fp64.  mean / invstd are [n][groups]."""
    x = x.double()
    gamma, beta = _affine(x, gamma, beta)
    n, p, c = x.shape
    mean, invstd = _stats(x, groups, unbiased, eps)
    pre = (x - mean) * invstd * gamma + beta
    y = pre if slope is None else torch.where(pre > 0, pre, pre * slope)
    cpg = c // groups
    return dict(mean=mean[:, 0, ::cpg].contiguous(), invstd=invstd[:, 0, ::cpg].contiguous(), pre=pre, y=y)


def gn_bwd_ref(dy, x, gamma, mask, groups, unbiased, eps, slope, addend=None):
    """First-order backward in closed form, fp64, under the LeakyReLU mask the caller observed.  Returns dx (+ addend), dgamma, dbeta."""
    dy, x = dy.double(), x.double()
    gamma, _ = _affine(x, gamma, None)
    n, p, c = x.shape
    k = _k(p, c, groups, unbiased)
    mean, invstd = _stats(x, groups, unbiased, eps)
    xhat = (x - mean) * invstd
    dz = dy * _slopes(mask, slope, dy)
    a = dz * gamma
    dx = invstd * (a - _E(a, groups) - k * xhat * _E(a * xhat, groups))
    if addend is not None:
        dx = dx + addend.double()
    return dx, (dz * xhat).sum((0, 1)), dz.sum((0, 1))


def gn_bwd2_ref(u, dy, x, gamma, mask, groups, unbiased, eps, slope):
    """Second-order backward in closed form, fp64: the gradients of <u, dx(dy, x, gamma)> at dy, x and gamma with the mask constant.
    With a = dz gamma, ubar = E[u], w = E[u xhat], pa = E[a], q = E[a xhat], T = E[u a] - ubar pa - k w q:
        g_dy = gamma invstd (u - ubar - k xhat w) lrelu',   g_x = -k invstd^2 [q (u - ubar) + w (a - pa) + xhat (T - 2 k w q)],
        g_gamma = sum_{n,p} dz invstd (u - ubar - k xhat w)."""
    u, dy, x = u.double(), dy.double(), x.double()
    gamma, _ = _affine(x, gamma, None)
    n, p, c = x.shape
    k = _k(p, c, groups, unbiased)
    mean, invstd = _stats(x, groups, unbiased, eps)
    xhat = (x - mean) * invstd
    mk = _slopes(mask, slope, dy)
    dz = dy * mk
    a = dz * gamma
    ubar, w, pa, q = _E(u, groups), _E(u * xhat, groups), _E(a, groups), _E(a * xhat, groups)
    T = _E(u * a, groups) - ubar * pa - k * w * q
    core = invstd * (u - ubar - k * xhat * w)
    g_dy = gamma * core * mk
    g_x = -k * invstd * invstd * (q * (u - ubar) + w * (a - pa) + xhat * (T - 2 * k * w * q))
    return g_dy, g_x, (dz * core).sum((0, 1))


def gn_autograd(x, gamma, beta, dy, u, groups, unbiased, eps, slope, dtype, addend=None):
    """The same quantities from stock torch under autograd in `dtype`, in the reference's formulation: F.instance_norm for the
    instance kind (biased variance, groups = c; F.group_norm for another biased grouping), the view(N, G, -1) mean / var form of
    base_networks.GroupNorm for the unbiased kind; then F.leaky_relu, the first-order backward with create_graph, and the backward
    of <u, dx>.  Returns a dict with y, mask (torch's own y > 0), mean, invstd ([n][groups]), dx (+ addend), dgamma, dbeta, g_dy,
    g_x, g_gamma; the parameter entries are None when gamma is None."""
    n, p, c = x.shape
    affine = gamma is not None
    x4 = x.to(dtype).permute(0, 2, 1).reshape(n, c, p, 1).contiguous().requires_grad_()            # NCHW, H = p, W = 1
    dy4 = dy.to(dtype).permute(0, 2, 1).reshape(n, c, p, 1).contiguous().requires_grad_()
    gg = gamma.to(dtype).reshape(c).clone().requires_grad_() if affine else None
    bb = beta.to(dtype).reshape(c).clone().requires_grad_() if affine else None
    xg = x4.view(n, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    if unbiased:
        var = xg.var(-1, keepdim=True)
        pre = ((xg - mean) / (var + eps).sqrt()).view(n, c, p, 1)
        if affine:
            pre = pre * gg.view(1, c, 1, 1) + bb.view(1, c, 1, 1)
    else:
        var = xg.var(-1, unbiased=False, keepdim=True)
        pre = F.instance_norm(x4, weight=gg, bias=bb, eps=eps) if groups == c else F.group_norm(x4, groups, gg, bb, eps)
    y = pre if slope is None else F.leaky_relu(pre, slope)
    ins = [x4] + ([gg, bb] if affine else [])
    first = torch.autograd.grad(y, ins, dy4, create_graph=True)
    second = torch.autograd.grad((first[0] * u.to(dtype).permute(0, 2, 1).reshape(n, c, p, 1)).sum(), [dy4, x4] + ([gg] if affine else []))
    back = lambda t: t.detach().reshape(n, c, p).permute(0, 2, 1).contiguous()                     # noqa: E731
    out = dict(y=back(y), mean=mean.detach().reshape(n, groups), invstd=(1.0 / (var + eps).sqrt()).detach().reshape(n, groups),
               dx=back(first[0]), dgamma=first[1].detach() if affine else None, dbeta=first[2].detach() if affine else None,
               g_dy=back(second[0]), g_x=back(second[1]), g_gamma=second[2].detach() if affine else None)
    out['mask'] = out['y'] > 0
    if addend is not None:
        out['dx'] = out['dx'] + addend.to(dtype)
    return out
