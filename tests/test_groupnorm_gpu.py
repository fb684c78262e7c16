"""gn.hip -- the per-sample normalisations (instance norm, the reference's GroupNorm) + LeakyReLU with their first- and second-order
backward -- through the C entry points (ctypes) and through ops.group_norm_act on the same data, against the fp64 closed forms of
tests/groupnorm_ref.py.

Protocol (that of tests/test_reductions_gpu.py for bn.hip): err = max|got - ref64| / max|ref64| per output tensor; the bar is
reduction_ref.bound(err of stock fp32 torch autograd on the CPU) = max(8 x torch, 32 * 2^-24).  The fp64 reference is taken under
the LeakyReLU mask the DEVICE produced, torch is measured under its own mask, and the share of elements whose device mask differs
from the fp64 mask is capped (1e-4 for the well-conditioned families, 1 % for mean100 / corner3 / corner10).  Every figure is
printed before the test asserts.  Bit-identity is asserted where the kernels claim it: the accumulating slots, the addend (in and
out of place), ops.group_norm_act against the entry points, and every sample of a batch against the same sample computed alone."""
import pytest
import torch

from tests import groupnorm_ref as G
from tests import reduction_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS = 1e-5
MASK_CAP = {'normal': 1e-4, 'constant_channel': 1e-4, 'gamma_signs': 1e-4, 'mean100': 1e-2, 'corner3': 1e-2, 'corner10': 1e-2}

# every case with per-channel gamma / beta; the biased ones (the instance kind) also without, as nn.InstanceNorm2d(C) runs them
CASES = [c + (True,) for c in G.GN_CASES] + [c + (False,) for c in G.GN_CASES if c[5] == 0]


def _lib():
    from sradsgan_amd import _hip
    return _hip.lib()


def _ok(rc, what):
    from sradsgan_amd import _hip
    _hip.check(rc, what)


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Table:
    """Collects `err <= bound` checks of one test: prints every figure, asserts at the end."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def check(self, name, got, ref, torch_got=None, torch_ref=None):
        e = R.err(got, ref)
        te = 0.0 if torch_got is None else R.err(torch_got, ref if torch_ref is None else torch_ref)
        b = R.bound(te)
        print('%-44s %-26s err %.3e  torch-fp32 %.3e  bound %.3e%s' % (self.case, name, e, te, b, '' if e <= b else '   <-- FAIL'))
        if not e <= b:
            self.bad.append((name, e, te, b))

    def same_bits(self, name, a, b):
        same = a.shape == b.shape and torch.equal(a, b)
        print('%-44s %-26s bit-identical: %s' % (self.case, name, same))
        if not same:
            self.bad.append((name, 'bits differ'))

    def at_most(self, name, value, cap):
        print('%-44s %-26s %.3e (cap %.1e)%s' % (self.case, name, value, cap, '' if value <= cap else '   <-- FAIL'))
        if not value <= cap:
            self.bad.append((name, value, cap))

    def done(self):
        assert not self.bad, (self.case, self.bad)


class _GnDevice:
    """The C entry points of gn.hip on [n][p][C] device tensors."""

    def __init__(self, t, groups, unbiased, slope, affine):
        self.lib = _lib()
        self.t = {k: v.to(DEV) for k, v in t.items()}
        self.n, self.p, self.c = t['x'].shape
        self.gamma, self.beta = (self.t['gamma'], self.t['beta']) if affine else (None, None)
        self.affine = affine
        ws = self.lib.srhip_gn_workspace(self.n, self.p, self.c)
        self.ws = torch.full((ws // 4,), float('nan'), device=DEV)
        self.dims = (_p(self.ws), ws, self.n, self.p, self.c, groups, unbiased)
        self.end = (float(slope or 0.0), int(slope is not None), _stream())
        self.groups = groups

    def new(self, like='x'):
        return torch.full_like(self.t[like], float('nan'))

    def fwd(self):
        y = self.new()
        mean, invstd = torch.full((self.n * self.groups,), float('nan'), device=DEV), torch.full((self.n * self.groups,), float('nan'), device=DEV)
        _ok(self.lib.srhip_gn_fwd(_p(self.t['x']), _p(self.gamma), _p(self.beta), _p(y), _p(mean), _p(invstd), *self.dims, EPS, *self.end), 'gn_fwd')
        return dict(y=y, mean=mean, invstd=invstd)

    def bwd(self, f, acc=False, addend=None):
        """addend: None | 'out' | 'in' (dx starts as the addend).  Returns dx, dgamma, dbeta, acc_gamma, acc_beta."""
        t = self.t
        dx = t['addend'].clone() if addend == 'in' else self.new()
        ad = None if addend is None else (dx if addend == 'in' else t['addend'])
        dgamma, dbeta = (self.new('gamma'), self.new('gamma')) if self.affine else (None, None)
        ag, ab = (t['acc_gamma'].clone(), t['acc_beta'].clone()) if acc else (None, None)
        _ok(self.lib.srhip_gn_bwd(_p(t['dy']), _p(t['x']), _p(self.gamma), _p(self.beta), _p(f['mean']), _p(f['invstd']), _p(ad), _p(dx),
                                  _p(dgamma), _p(dbeta), _p(ag), _p(ab), *self.dims, *self.end), 'gn_bwd')
        return dx, dgamma, dbeta, ag, ab

    def bwd2(self, f, acc=False):
        t = self.t
        g_dy, g_x = self.new(), self.new()
        g_gamma = self.new('gamma') if self.affine else None
        ag = t['acc_gamma'].clone() if acc else None
        _ok(self.lib.srhip_gn_bwd_bwd(_p(t['u']), _p(t['dy']), _p(t['x']), _p(self.gamma), _p(self.beta), _p(f['mean']), _p(f['invstd']),
                                      _p(g_dy), _p(g_x), _p(g_gamma), _p(ag), *self.dims, *self.end), 'gn_bwd_bwd')
        return g_dy, g_x, g_gamma, ag


def _through_ops(dev, groups, unbiased, slope):
    """The same data through ops.group_norm_act and autograd: y, (dx, dgamma, dbeta), (g_dy, g_x, g_gamma), as [n][p][C] / [C]."""
    from sradsgan_amd import ops
    n, p, c = dev.n, dev.p, dev.c
    as4 = lambda v: v.view(n, p, 1, c).permute(0, 3, 1, 2)                      # noqa: E731  logical NCHW, NHWC memory
    back = lambda v: v.permute(0, 2, 3, 1).reshape(n, p, c)                     # noqa: E731
    x4, dy4 = as4(dev.t['x']).requires_grad_(), as4(dev.t['dy']).requires_grad_()
    w = dev.gamma.view(1, c, 1, 1).clone().requires_grad_() if dev.affine else None
    b = dev.beta.view(1, c, 1, 1).clone().requires_grad_() if dev.affine else None
    y = ops.group_norm_act(x4, groups, w, b, EPS, bool(unbiased), slope)
    first = torch.autograd.grad(y, [x4] + ([w, b] if dev.affine else []), dy4, create_graph=True)
    second = torch.autograd.grad(first[0], [dy4, x4] + ([w] if dev.affine else []), as4(dev.t['u']))
    flat = lambda v: v.reshape(-1)                                              # noqa: E731
    return (back(y.detach()), (back(first[0].detach()),) + tuple(flat(v.detach()) for v in first[1:]),
            (back(second[0]), back(second[1])) + tuple(flat(v) for v in second[2:]))


@pytest.mark.parametrize('slope', [0.2, None], ids=['lrelu', 'linear'])
@pytest.mark.parametrize('family,n,p,c,groups,unbiased,affine', CASES,
                         ids=['%s-%dx%dx%d-g%d-u%d-%s' % (k[:6] + ('affine' if k[6] else 'plain',)) for k in CASES])
def test_group_norm_entry_points_against_fp64(family, n, p, c, groups, unbiased, affine, slope):
    t = G.gn_inputs(family, n, p, c)
    gamma, beta = (t['gamma'], t['beta']) if affine else (None, None)
    tab = _Table('gn %s %dx%dx%d g%d u%d %s %s' % (family, n, p, c, groups, unbiased, 'affine' if affine else 'plain', 'lrelu' if slope else 'linear'))
    dev = _GnDevice(t, groups, unbiased, slope, affine)
    T32 = G.gn_autograd(t['x'], gamma, beta, t['dy'], t['u'], groups, unbiased, EPS, slope, torch.float32)

    # ---- forward
    ref = G.gn_fwd_ref(t['x'], gamma, beta, groups, unbiased, EPS, slope)
    f = dev.fwd()
    tab.check('fwd y', f['y'], ref['y'], T32['y'])
    for k in ('mean', 'invstd'):
        tab.check('fwd ' + k, f[k].view(n, groups), ref[k], T32[k])
    mask = (f['y'] > 0).cpu()
    if slope is not None:
        tab.at_most('mask share off fp64', float((mask != (ref['pre'] > 0)).double().mean()), MASK_CAP[family])

    # ---- first-order backward
    names = ('dx', 'dgamma', 'dbeta') if affine else ('dx',)
    ref1 = dict(zip(names, G.gn_bwd_ref(t['dy'], t['x'], gamma, mask, groups, unbiased, EPS, slope)))
    tref1 = dict(zip(names, G.gn_bwd_ref(t['dy'], t['x'], gamma, T32['mask'], groups, unbiased, EPS, slope)))
    b = dev.bwd(f)
    for k, got in zip(names, b):
        tab.check('bwd ' + k, got, ref1[k], T32[k], tref1[k])
    out = dev.bwd(f, addend='out')
    tab.same_bits('bwd addend: plain + addend', out[0], b[0] + dev.t['addend'])
    tab.check('bwd dx + addend', out[0], ref1['dx'] + t['addend'].double(), T32['dx'] + t['addend'], tref1['dx'] + t['addend'].double())
    inp = dev.bwd(f, addend='in')
    tab.same_bits('bwd addend in place', inp[0], out[0])
    if affine:
        acc = dev.bwd(f, acc=True, addend='in')
        for k, got, plain in zip(names, acc, inp):
            tab.same_bits('bwd acc ' + k, got, plain)
        tab.same_bits('bwd acc_gamma = seed + dgamma', acc[3], dev.t['acc_gamma'] + b[1])       # one fp32 add per channel, exactly
        tab.same_bits('bwd acc_beta = seed + dbeta', acc[4], dev.t['acc_beta'] + b[2])
        for k, got in zip(names[1:], out[1:3]):
            tab.same_bits('bwd addend ' + k, got, b[names.index(k)])

    # ---- second-order backward
    names2 = ('g_dy', 'g_x', 'g_gamma') if affine else ('g_dy', 'g_x')
    ref2 = dict(zip(names2, G.gn_bwd2_ref(t['u'], t['dy'], t['x'], gamma, mask, groups, unbiased, EPS, slope)))
    tref2 = dict(zip(names2, G.gn_bwd2_ref(t['u'], t['dy'], t['x'], gamma, T32['mask'], groups, unbiased, EPS, slope)))
    s = dev.bwd2(f)
    for k, got in zip(names2, s):
        tab.check('bwd_bwd ' + k, got, ref2[k], T32[k], tref2[k])
    if affine:
        sa = dev.bwd2(f, acc=True)
        for k, got, plain in zip(names2, sa, s):
            tab.same_bits('bwd_bwd acc ' + k, got, plain)
        tab.same_bits('bwd_bwd acc_gamma = seed + g_gamma', sa[3], dev.t['acc_gamma'] + s[2])

    # ---- the host wrapper on the same data
    y4, first, second = _through_ops(dev, groups, unbiased, slope)
    tab.same_bits('ops.group_norm_act y', y4, f['y'])
    for k, got, want in zip(names, first, b):
        tab.same_bits('ops ' + k, got, want)
    for k, got, want in zip(names2, second, s):
        tab.same_bits('ops ' + k, got, want)
    torch.cuda.synchronize()
    tab.done()


@pytest.mark.parametrize('n,p,c,groups,unbiased', [(3, 197, 192, 32, 1), (2, 2053, 64, 32, 1)], ids=['3x197x192', '2x2053x64'])
def test_a_sample_does_not_depend_on_its_batch(n, p, c, groups, unbiased):
    """What the per-sample norms are for: y, dx, g_dy and g_x of each sample computed alone are bit-identical to its rows in the batch."""
    t = G.gn_inputs('normal', n, p, c)
    tab = _Table('gn alone-vs-batch %dx%dx%d' % (n, p, c))
    dev = _GnDevice(t, groups, unbiased, 0.2, True)
    f = dev.fwd()
    dx, g = dev.bwd(f)[0], dev.bwd2(f)
    for i in range(n):
        one = {k: (v[i:i + 1].contiguous() if v.dim() == 3 else v) for k, v in t.items()}
        d1 = _GnDevice(one, groups, unbiased, 0.2, True)
        f1 = d1.fwd()
        g1 = d1.bwd2(f1)
        tab.same_bits('sample %d y' % i, f1['y'][0], f['y'][i])
        tab.same_bits('sample %d mean' % i, f1['mean'], f['mean'][i * groups:(i + 1) * groups])
        tab.same_bits('sample %d dx' % i, d1.bwd(f1)[0][0], dx[i])
        tab.same_bits('sample %d g_dy' % i, g1[0][0], g[0][i])
        tab.same_bits('sample %d g_x' % i, g1[1][0], g[1][i])
    torch.cuda.synchronize()
    tab.done()


@pytest.mark.parametrize('n,p,c,groups', [(2, 1, 64, 64), (2, 8, 6, 2), (2, 8, 64, 24), (2, 8, 1028, 4)], ids=['m1', 'c6', 'c-not-groups', 'c1028'])
def test_unsupported_shapes_are_refused_and_write_nothing(n, p, c, groups):
    lib = _lib()
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)                    # noqa: E731
    x, par = torch.randn(n, p, c, device=DEV), torch.ones(c, device=DEV)
    outs = [nan(n, p, c), nan(n, p, c), nan(n * groups), nan(n * groups), nan(c), nan(c)]
    ws = nan(1 << 20)
    dims = (_p(ws), ws.numel() * 4, n, p, c, groups, 0)
    rcs = [lib.srhip_gn_fwd(_p(x), _p(par), _p(par), _p(outs[0]), _p(outs[2]), _p(outs[3]), *dims, EPS, 0.2, 1, _stream()),
           lib.srhip_gn_bwd(_p(x), _p(x), _p(par), _p(par), _p(par), _p(par), None, _p(outs[0]), _p(outs[4]), _p(outs[5]), None, None, *dims,
                            0.2, 1, _stream()),
           lib.srhip_gn_bwd_bwd(_p(x), _p(x), _p(x), _p(par), _p(par), _p(par), _p(par), _p(outs[0]), _p(outs[1]), _p(outs[4]), None, *dims,
                                0.2, 1, _stream())]
    torch.cuda.synchronize()
    assert rcs == [-1, -1, -1] and lib.srhip_last_error()
    assert all(bool(torch.isnan(o).all()) for o in outs)


@pytest.mark.parametrize('n,p,c,groups,unbiased,affine', [(2, 65, 64, 32, 1, True), (2, 65, 64, 64, 0, False)], ids=['group', 'instance'])
def test_other_second_order_cotangents_go_through_the_differentiable_restatement(n, p, c, groups, unbiased, affine):
    """A double backward that itself records a graph (or carries cotangents on dgamma / dbeta) leaves the fused second-order pass for
    ops._gn_reference_bwd.  Same fp32 arithmetic in another order on well-conditioned inputs ('normal': both sit at ~1e-6 of fp64 in
    the table above); a wrong term would be O(1), so 1e-4 of each tensor's scale separates the two."""
    from sradsgan_amd import ops
    t = G.gn_inputs('normal', n, p, c)
    as4 = lambda v: v.to(DEV).view(n, p, 1, c).permute(0, 3, 1, 2)              # noqa: E731
    x4, dy4, u4 = as4(t['x']).requires_grad_(), as4(t['dy']).requires_grad_(), as4(t['u'])
    w = t['gamma'].to(DEV).view(1, c, 1, 1).requires_grad_() if affine else None
    b = t['beta'].to(DEV).view(1, c, 1, 1).requires_grad_() if affine else None
    ins = [dy4, x4] + ([w] if affine else [])
    y = ops.group_norm_act(x4, groups, w, b, EPS, bool(unbiased), 0.2)
    first = torch.autograd.grad(y, [x4] + ([w, b] if affine else []), dy4, create_graph=True)
    fast = torch.autograd.grad(first[0], ins, u4, retain_graph=True)
    slow = torch.autograd.grad(first[0], ins, u4, create_graph=True, retain_graph=True)
    for name, a, f in zip(('g_dy', 'g_x', 'g_gamma'), slow, fast):
        e = R.err(a, f)
        print('restatement vs fused %-8s %.3e' % (name, e))
        assert e <= 1e-4, (name, e)
    if affine:                                       # cotangents on all three outputs of the first-order backward
        outs = [first[0], first[1], first[2]]
        cots = [u4, torch.ones_like(first[1]), torch.ones_like(first[2])]
        got = torch.autograd.grad(outs, ins, cots)
        back = lambda v: v.permute(0, 2, 3, 1).reshape(n, p, c)                 # noqa: E731
        mask = (back(y.detach()) > 0).cpu()          # the device's own mask
        # fp64 autograd of the same three-cotangent expression through the first-order closed form
        x64, dy64, g64 = t['x'].double().requires_grad_(), t['dy'].double().requires_grad_(), t['gamma'].double().requires_grad_()
        dx_, dg_, db_ = G.gn_bwd_ref(dy64, x64, g64, mask, groups, unbiased, EPS, 0.2)
        want = torch.autograd.grad((dx_ * t['u'].double()).sum() + dg_.sum() + db_.sum(), [dy64, x64, g64])
        for name, a, r in zip(('g_dy', 'g_x', 'g_gamma'), (back(got[0]), back(got[1]), got[2].reshape(-1)), want):
            e = R.err(a, r)
            print('three cotangents     %-8s %.3e' % (name, e))
            assert e <= 1e-4, (name, e)
