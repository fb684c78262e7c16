"""The kernels around the convolutions -- bn.hip, colsum (elementwise.hip), losses.hip, optim.hip, metrics.hip -- against the fp64
references of tests/reduction_ref.py, at the shapes where their launch geometry changes: slab counts and caps, second trips of the
stage-2 loops, grid-stride trips, scalar tails, channel counts that do not fill a block, and inputs at the kinks of the arithmetic.

The measure per output tensor is err = max|got - ref64| / max|ref64|, the bar max(8 x err of stock fp32 torch on the CPU, 32 * 2^-24)
(reduction_ref.err / bound): the code under test never sets its own bar.  Every check prints `err torch-fp32-err bound` before the test
asserts.  The metrics keep the project's own 1e-9 against the oracle's numpy arithmetic; bit-identity is asserted where the kernels
claim it.  C entry points are called through ctypes where ops cannot express the case (ld, an offset pointer, one specific entry)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import reduction_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EPS, MOMENTUM = 1e-5, 0.1


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
        """got vs ref (fp64); the bar from torch_got (stock fp32 torch) vs torch_ref (ref unless the yardstick has a reference of
        its own, e.g. under torch's own LeakyReLU mask).  torch_got None: no stock counterpart, the bar is the floor."""
        e = R.err(got, ref)
        te = 0.0 if torch_got is None else R.err(torch_got, ref if torch_ref is None else torch_ref)
        b = R.bound(te)
        print('%-46s %-22s err %.3e  torch-fp32 %.3e  bound %.3e%s' % (self.case, name, e, te, b, '' if e <= b else '   <-- FAIL'))
        if not e <= b:
            self.bad.append((name, e, te, b))

    def same_bits(self, name, a, b):
        same = torch.equal(a, b)
        print('%-46s %-22s bit-identical: %s' % (self.case, name, same))
        if not same:
            self.bad.append((name, 'bits differ', float((a.double() - b.double()).abs().max())))

    def done(self):
        assert not self.bad, (self.case, self.bad)


# --------------------------------------------------------------------------------------------- #
# BatchNorm + LeakyReLU: every entry point of bn.hip
# --------------------------------------------------------------------------------------------- #

# rows = N * H * W of a real 4-d tensor (ops.batch_norm_act takes that form)
BN_NHW = {1: (1, 1, 1), 2: (2, 1, 1), 63: (1, 7, 9), 64: (1, 8, 8), 65: (1, 5, 13), 4097: (1, 17, 241), 65600: (2, 160, 205),
          130: (2, 5, 13), 75: (3, 5, 5)}
BN_GRID = [(1, 4), (2, 4), (63, 12), (64, 64), (65, 192),
           (4097, 64),       # 65 slabs: the second trip of the stage-2 loops
           (65600, 4),       # the 1024-slab cap, rows_per_block = 65
           (130, 1024),      # one row lane per block
           (75, 512)]
BN_CASES = [('normal', r, c) for r, c in BN_GRID] + [(f, r, c) for f in R.BN_FAMILIES[1:] for r, c in ((4097, 64), (65, 192))]


class _BnDevice:
    """The C entry points of bn.hip on [rows][C] device tensors."""

    def __init__(self, t, slope):
        self.lib = _lib()
        self.t = {k: v.to(DEV) for k, v in t.items()}
        self.rows, self.c = t['x'].shape
        self.slope, self.act = float(slope or 0.0), int(slope is not None)
        self.ws = torch.empty(max(self.lib.srhip_bn_workspace(self.rows, self.c), self.lib.srhip_bn_bwd2_workspace(self.rows, self.c)) // 4 + 2,
                              device=DEV)
        self.tail = (_p(self.ws), self.ws.numel() * 4, self.rows, self.c)

    def new(self, like='x'):
        return torch.full_like(self.t[like], float('nan'))

    def fwd(self, running):
        t = self.t
        y, mean, invstd = self.new(), self.new('gamma'), self.new('gamma')
        rm, rv = (t['running_mean'].clone(), t['running_var'].clone()) if running else (None, None)
        _ok(self.lib.srhip_bn_train_fwd(_p(t['x']), _p(t['gamma']), _p(t['beta']), _p(rm), _p(rv), _p(y), _p(mean), _p(invstd), *self.tail,
                                        EPS, MOMENTUM, self.slope, self.act, _stream()), 'bn_train_fwd')
        return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)

    def eval_fwd(self):
        t = self.t
        y = self.new()
        _ok(self.lib.srhip_bn_eval_fwd(_p(t['x']), _p(t['gamma']), _p(t['beta']), _p(t['running_mean']), _p(t['running_var']), _p(y),
                                       self.rows, self.c, EPS, self.slope, self.act, _stream()), 'bn_eval_fwd')
        return y

    def bwd(self, entry, f, inplace=False):
        """entry: 'bwd' | 'acc' | 'acc_x' | 'acc_xa'.  Returns dx, dgamma, dbeta, acc_gamma, acc_beta (the last two None for 'bwd')."""
        t, lib = self.t, self.lib
        dx = t['addend'].clone() if inplace else self.new()
        dgamma, dbeta = self.new('gamma'), self.new('gamma')
        ag, ab = (None, None) if entry == 'bwd' else (t['acc_gamma'].clone(), t['acc_beta'].clone())
        stats = (_p(f['mean']), _p(f['invstd']))
        end = self.tail + (self.slope, self.act, _stream())
        if entry == 'bwd':
            rc = lib.srhip_bn_train_bwd(_p(t['dy']), _p(t['x']), _p(f['y']), _p(t['gamma']), *stats, _p(dx), _p(dgamma), _p(dbeta), *end)
        elif entry == 'acc':
            rc = lib.srhip_bn_train_bwd_acc(_p(t['dy']), _p(t['x']), _p(f['y']), _p(t['gamma']), *stats, _p(dx), _p(dgamma), _p(dbeta),
                                            _p(ag), _p(ab), *end)
        elif entry == 'acc_x':
            rc = lib.srhip_bn_train_bwd_acc_x(_p(t['dy']), _p(t['x']), _p(t['gamma']), _p(t['beta']), *stats, _p(dx), _p(dgamma),
                                              _p(dbeta), _p(ag), _p(ab), *end)
        else:
            rc = lib.srhip_bn_train_bwd_acc_xa(_p(t['dy']), _p(t['x']), _p(t['gamma']), _p(t['beta']), *stats,
                                               _p(dx if inplace else t['addend']), _p(dx), _p(dgamma), _p(dbeta), _p(ag), _p(ab), *end)
        _ok(rc, 'bn_train_' + entry)
        return dx, dgamma, dbeta, ag, ab

    def bwd2(self, entry, f):
        """entry: 'bwd_bwd' | 'acc' | 'acc_x'.  Returns g_dy, g_x, g_gamma, acc_gamma."""
        t, lib = self.t, self.lib
        g_dy, g_x, g_gamma = self.new(), self.new(), self.new('gamma')
        ag = None if entry == 'bwd_bwd' else t['acc_gamma'].clone()
        stats = (_p(f['mean']), _p(f['invstd']))
        end = self.tail + (self.slope, self.act, _stream())
        if entry == 'bwd_bwd':
            rc = lib.srhip_bn_train_bwd_bwd(_p(t['u']), _p(t['dy']), _p(t['x']), _p(f['y']), _p(t['gamma']), *stats, _p(g_dy), _p(g_x),
                                            _p(g_gamma), *end)
        elif entry == 'acc':
            rc = lib.srhip_bn_train_bwd_bwd_acc(_p(t['u']), _p(t['dy']), _p(t['x']), _p(f['y']), _p(t['gamma']), *stats, _p(g_dy), _p(g_x),
                                                _p(g_gamma), _p(ag), *end)
        else:
            rc = lib.srhip_bn_train_bwd_bwd_acc_x(_p(t['u']), _p(t['dy']), _p(t['x']), _p(t['gamma']), _p(t['beta']), *stats, _p(g_dy),
                                                  _p(g_x), _p(g_gamma), _p(ag), *end)
        _ok(rc, 'bn_train_bwd_' + entry)
        return g_dy, g_x, g_gamma, ag


@pytest.mark.parametrize('slope', [0.2, None], ids=['lrelu', 'linear'])
@pytest.mark.parametrize('family,rows,c', BN_CASES, ids=['%s-%dx%d' % k for k in BN_CASES])
def test_batch_norm_entry_points_against_fp64(family, rows, c, slope):
    """Every entry point of bn.hip on one input against the fp64 closed forms.  The backward references take the LeakyReLU mask the
    DEVICE produced (y > 0): an element within rounding of zero may land on either side; stock fp32 torch, the yardstick, is measured
    the same way under its own mask.  The `_x` twins, the accumulating variants and the in-place addend must reproduce their plain
    forms bit for bit."""
    t = R.bn_inputs(family, rows, c)
    tab = _Table('bn %s %dx%d %s' % (family, rows, c, 'lrelu' if slope else 'linear'))
    dev = _BnDevice(t, slope)
    # stock fp32 torch on the CPU (rows = 1: torch has no answer -- its unbiased variance is 0/0 -- so the bar there is the floor)
    T32 = R.bn_autograd(t['x'], t['gamma'], t['beta'], t['dy'], t['u'], EPS, slope, torch.float32, running_mean=t['running_mean'],
                        running_var=t['running_var'], momentum=MOMENTUM) if rows > 1 else None
    tq = (lambda k: T32[k]) if T32 is not None else (lambda k: None)

    # ---- forward
    ref = R.bn_fwd_ref(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], EPS, MOMENTUM, slope)
    f = dev.fwd(running=True)
    for k in ('y', 'mean', 'invstd', 'running_mean', 'running_var'):
        tab.check('fwd ' + k, f[k], ref[k], tq(k))
    f0 = dev.fwd(running=False)
    for k in ('y', 'mean', 'invstd'):
        tab.same_bits('fwd(no running) ' + k, f0[k], f[k])
    # the same through the host wrapper on a 4-d NHWC tensor
    from sradsgan_amd import ops
    n, h, w = BN_NHW[rows]
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(t['gamma']), bn.bias.copy_(t['beta']), bn.running_mean.copy_(t['running_mean']), bn.running_var.copy_(t['running_var'])
        y4 = ops.batch_norm_act(dev.t['x'].view(n, h, w, c).permute(0, 3, 1, 2), bn, slope)
    tab.same_bits('ops.batch_norm_act y', y4.permute(0, 2, 3, 1).reshape(rows, c), f['y'])
    tab.same_bits('ops running_mean', bn.running_mean, f['running_mean'])
    tab.same_bits('ops running_var', bn.running_var, f['running_var'])
    # eval mode: the running statistics as given
    T_eval = F.batch_norm(t['x'], t['running_mean'], t['running_var'], t['gamma'], t['beta'], False, 0.0, EPS)
    T_eval = T_eval if slope is None else F.leaky_relu(T_eval, slope)
    tab.check('eval y', dev.eval_fwd(), R.bn_eval_ref(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], EPS, slope), T_eval)

    # ---- first-order backward
    mask = (f['y'] > 0).cpu()
    names = ('dx', 'dgamma', 'dbeta')
    ref1 = dict(zip(names, R.bn_bwd_ref(t['dy'], t['x'], t['gamma'], mask, EPS, slope)))
    tref1 = dict(zip(names, R.bn_bwd_ref(t['dy'], t['x'], t['gamma'], T32['mask'], EPS, slope))) if T32 else {}
    b = dev.bwd('bwd', f)
    for k, got in zip(names, b):
        tab.check('bwd ' + k, got, ref1[k], tq(k), tref1.get(k))
    acc = dev.bwd('acc', f)
    for k, got, plain in zip(names, acc, b):
        tab.same_bits('bwd_acc ' + k, got, plain)
    for k, got, seed, plain in (('dgamma', acc[3], t['acc_gamma'], b[1]), ('dbeta', acc[4], t['acc_beta'], b[2])):
        tab.same_bits('bwd_acc acc += ' + k, got, seed.to(DEV) + plain)                 # one fp32 add per channel, exactly
        tab.check('bwd_acc acc_' + k[1:], got, seed.double() + ref1[k], None if T32 is None else seed + T32[k],
                  None if T32 is None else seed.double() + tref1[k])
    accx = dev.bwd('acc_x', f)
    for k, got, twin in zip(names + ('acc_gamma', 'acc_beta'), accx, acc):
        tab.same_bits('bwd_acc_x ' + k, got, twin)
    xa = dev.bwd('acc_xa', f)
    tab.check('bwd_acc_xa dx+addend', xa[0], ref1['dx'] + t['addend'].double(), None if T32 is None else T32['dx'] + t['addend'],
              None if T32 is None else tref1['dx'] + t['addend'].double())
    tab.same_bits('bwd_acc_xa dx+addend (one fp32 add)', xa[0], accx[0] + dev.t['addend'])
    for k, got, twin in zip(names[1:] + ('acc_gamma', 'acc_beta'), xa[1:], accx[1:]):
        tab.same_bits('bwd_acc_xa ' + k, got, twin)
    xi = dev.bwd('acc_xa', f, inplace=True)
    for k, got, twin in zip(names + ('acc_gamma', 'acc_beta'), xi, xa):
        tab.same_bits('bwd_acc_xa in place ' + k, got, twin)

    # ---- second-order backward
    names2 = ('g_dy', 'g_x', 'g_gamma')
    ref2 = dict(zip(names2, R.bn_bwd2_ref(t['u'], t['dy'], t['x'], t['gamma'], mask, EPS, slope)))
    tref2 = dict(zip(names2, R.bn_bwd2_ref(t['u'], t['dy'], t['x'], t['gamma'], T32['mask'], EPS, slope))) if T32 else {}
    s = dev.bwd2('bwd_bwd', f)
    for k, got in zip(names2, s):
        tab.check('bwd_bwd ' + k, got, ref2[k], tq(k), tref2.get(k))
    sa = dev.bwd2('acc', f)
    for k, got, plain in zip(names2, sa, s):
        tab.same_bits('bwd_bwd_acc ' + k, got, plain)
    tab.same_bits('bwd_bwd_acc acc += g_gamma', sa[3], dev.t['acc_gamma'] + s[2])
    sx = dev.bwd2('acc_x', f)
    for k, got, twin in zip(names2 + ('acc_gamma',), sx, sa):
        tab.same_bits('bwd_bwd_acc_x ' + k, got, twin)
    torch.cuda.synchronize()
    tab.done()


# --------------------------------------------------------------------------------------------- #
# column sums
# --------------------------------------------------------------------------------------------- #

COLSUM_ROWS = [1, 63, 65, 1025, 16385]          # 1025: 17 slabs = the second stage-2 trip; 16385: the 256-slab cap
COLSUM_C = [3, 64, 252, 255, 256, 512, 1024]
SENTINEL = -12345.0


def _colsum(m_dev_flat, off, rows, c, ld, poison=True):
    """srhip_colsum on the [rows][ld] matrix that starts `off` floats into m_dev_flat.  Returns (rc, out); out starts as SENTINEL and
    the workspace as NaN (a slab nobody wrote must not pass for a sum)."""
    lib = _lib()
    out = torch.full((c,), SENTINEL, device=DEV)
    ws = torch.full((max(lib.srhip_colsum_workspace(rows, c) // 4, 1),), float('nan') if poison else 0.0, device=DEV)
    rc = lib.srhip_colsum(m_dev_flat.data_ptr() + 4 * off, _p(out), _p(ws), ws.numel() * 4, rows, c, ld, _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize('c', COLSUM_C)
@pytest.mark.parametrize('rows', COLSUM_ROWS)
def test_colsum_every_row_stride_and_alignment(rows, c):
    """srhip_colsum at ld = C, C + 4, C + 1 and from a base pointer one float into an allocation: every combination inside the
    documented limits (C <= 1024 in multiples of 4, else C <= 256) is SERVED -- 16-byte loads where ld and the address allow, the
    scalar form otherwise, which walks the column groups of a C > 256 matrix -- and equals the fp64 column sums.  (Before the fix
    C = 512 with ld = 513 returned SRHIP_OK with columns 0..255 = 0 and the rest unwritten.)"""
    from sradsgan_amd import ops
    g = torch.Generator().manual_seed(rows * 31 + c)
    m = torch.randn(rows, c, generator=g) + 0.25
    ref, t32 = R.colsum_ref(m), m.sum(0)
    tab = _Table('colsum %dx%d' % (rows, c))
    for ld, off in ((c, 0), (c + 4, 0), (c + 1, 0), (c, 1), (c + 1, 1)):
        flat = torch.full((rows * ld + off + 8,), float('nan'), device=DEV)              # padding columns are NaN: never to be read
        flat[off:off + rows * ld].view(rows, ld)[:, :c] = m.to(DEV)
        rc, out = _colsum(flat, off, rows, c, ld)
        assert rc == 0, (ld, off, _lib().srhip_last_error())
        assert not bool((out == SENTINEL).any()), ('SRHIP_OK with unwritten columns', ld, off)
        tab.check('ld=C+%d offset=%d' % (ld - c, off), out, ref, t32)
    tab.same_bits('ops.colsum_raw', ops.colsum_raw(m.to(DEV).view(1, 1, rows, c).permute(0, 3, 1, 2)),
                  _colsum(m.to(DEV).reshape(-1), 0, rows, c, c)[1])
    tab.done()


@pytest.mark.parametrize('c,ld', [(257, 257), (1028, 1028), (64, 60)])
def test_colsum_refusals_leave_the_output_untouched(c, ld):
    flat = torch.zeros(100 * max(ld, c) + 8, device=DEV)
    rc, out = _colsum(flat, 0, 100, c, ld)
    assert rc != 0 and b'colsum' in _lib().srhip_last_error()
    assert bool((out == SENTINEL).all())


# --------------------------------------------------------------------------------------------- #
# loss reductions
# --------------------------------------------------------------------------------------------- #

LOSS_COUNTS = [1, 3, 4, 5, 1023, 1024 * 256 * 4 + 5]        # the last: the grid-stride trip, all 1024 partials, and the scalar tail
GOUT = 0.37                                                 # the upstream gradient of every backward here


def _run_loss(fn, tensors, device):
    """fn(*leaves) -> scalar; backward under the upstream gradient GOUT.  Returns (value, [grads])."""
    leaves = [x.clone().to(device).requires_grad_() for x in tensors]
    out = fn(*leaves)
    (out * GOUT).backward()
    return out.detach(), [x.grad for x in leaves]


@pytest.mark.parametrize('count', LOSS_COUNTS)
def test_loss_reductions_forward_and_backward_against_fp64(count):
    """l1_mean, mse_mean, smooth_l1_mean (tensor and scalar target) and mean: the value and the gradients at BOTH tensor inputs under
    an upstream gradient != 1, against fp64; the yardstick is the nn.*Loss module on the CPU in fp32."""
    from sradsgan_amd import ops
    a, b = R.loss_inputs(count)
    tab = _Table('loss n=%d' % count)
    for name, op, stock, ref in (('l1_mean', ops.l1_mean, torch.nn.L1Loss(), R.l1_ref), ('mse_mean', ops.mse_mean, torch.nn.MSELoss(), R.mse_ref),
                                 ('smooth_l1_mean', ops.smooth_l1_mean, torch.nn.SmoothL1Loss(), R.smooth_l1_ref)):
        want = ref(a, b, GOUT)
        got, (da, db) = _run_loss(op, (a, b), DEV)
        tv, (tda, tdb) = _run_loss(stock, (a, b), 'cpu')
        tab.check(name, got, want[0], tv)
        tab.check(name + ' da', da, want[1], tda)
        tab.check(name + ' db', db, want[2], tdb)
    for target in (1.0, 0.0):                                    # NDSRGAN's valid / fake patch targets
        s = R.scalar_target_inputs(count, target)
        want = R.smooth_l1_ref(s, target, GOUT)
        got, (da,) = _run_loss(lambda x: ops.smooth_l1_mean(x, target), (s,), DEV)
        tv, (tda,) = _run_loss(lambda x: torch.nn.SmoothL1Loss()(x, torch.full_like(x, target)), (s,), 'cpu')
        tab.check('smooth_l1_mean(target %g)' % target, got, want[0], tv)
        tab.check('smooth_l1_mean(target %g) da' % target, da, want[1], tda)
    want = R.mean_ref(a, GOUT)
    got, (da,) = _run_loss(ops.mean, (a,), DEV)
    tv, (tda,) = _run_loss(torch.mean, (a,), 'cpu')
    tab.check('mean', got, want[0], tv)
    tab.check('mean dx', da, want[1], tda)
    tab.done()


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('npix', [1, 255, 262147])          # 262147 = 1024 * 256 + 3: one grid-stride trip more for three pixels
def test_gradient_penalty_norm_against_fp64(npix, c):
    from sradsgan_amd import ops
    g = R.gp_inputs(npix, c)
    as4 = lambda x: x.view(1, 1, npix, c).permute(0, 3, 1, 2)   # [1, C, 1, npix] over NHWC memory
    want = R.gp_ref(g, GOUT)
    got, (dg,) = _run_loss(lambda x: ops.gp_penalty(as4(x)), (g,), DEV)
    tv, (tdg,) = _run_loss(lambda x: ((as4(x).norm(2, 1) - 1) ** 2).mean(), (g,), 'cpu')
    tab = _Table('gp npix=%d C=%d' % (npix, c))
    tab.check('gp_penalty', got, want[0], tv)
    tab.check('gp_penalty dg', dg, want[1], tdg)
    if npix > 1:
        assert float(dg[npix - 1].abs().max()) == 0.0            # the zero-norm pixel: gradient 0, not NaN
    tab.done()


def test_loss_wrappers_copy_views_the_kernels_would_refuse():
    """What ops does with a non-contiguous view and with a view whose storage offset breaks the 16-byte alignment the float4
    reductions require: it HANDLES both (a dense aligned copy, ops._dense16), so the result and the gradients are those of the dense
    tensor bit for bit; the kernel's own `must be 16-byte aligned` refusal is never reached.  mean and gp_penalty load scalars and
    take any address."""
    from sradsgan_amd import ops
    n = 1023
    a, b = R.loss_inputs(n)
    base = [torch.zeros(2 * n + 8, device=DEV) for _ in range(4)]
    views = {'storage offset 1': (base[0][1:1 + n], base[1][1:1 + n]), 'stride 2': (base[2][0:2 * n:2], base[3][2:2 * n + 2:2])}
    for va, vb in views.values():
        va.copy_(a), vb.copy_(b)
    assert views['storage offset 1'][0].data_ptr() % 16 == 4 and not views['stride 2'][0].is_contiguous()
    for name, op in (('l1_mean', ops.l1_mean), ('mse_mean', ops.mse_mean), ('smooth_l1_mean', ops.smooth_l1_mean)):
        want, (wa, wb) = _run_loss(op, (a, b), DEV)
        for kind, (va, vb) in views.items():
            la, lb = va.detach().requires_grad_(), vb.detach().requires_grad_()
            out = op(la, lb)
            (out * GOUT).backward()
            assert torch.equal(out.detach(), want) and torch.equal(la.grad, wa) and torch.equal(lb.grad, wb), (name, kind)
    for kind, (va, _) in views.items():
        want, _ = _run_loss(ops.mean, (a,), DEV)
        assert torch.equal(ops.mean(va), want), kind
        assert torch.equal(ops.smooth_l1_mean(va, 1.0), ops.smooth_l1_mean(a.to(DEV), 1.0)), kind
    g = R.gp_inputs(255, 3)
    base = torch.zeros(255 * 3 + 8, device=DEV)
    base[1:1 + 255 * 3].copy_(g.reshape(-1))
    as4 = lambda x: x.view(1, 1, 255, 3).permute(0, 3, 1, 2)
    assert torch.equal(ops.gp_penalty(as4(base[1:1 + 255 * 3])), ops.gp_penalty(as4(g.to(DEV))))


# --------------------------------------------------------------------------------------------- #
# Adam
# --------------------------------------------------------------------------------------------- #

ADAM_N = 4 * (2048 * 256 + 3)        # float4 items: one grid-stride trip more than the 2048-block cap covers, for three items
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS      # exact in fp32 (tests/reduction_ref.py)


@pytest.mark.parametrize('clip', [0.0, 0.05])
@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
def test_adam_arena_kernel_against_fp64_recurrences(grad_scale, clip):
    """srhip_adam_step on a flat arena of 4 * (2048 * 256 + 3) floats (p, g, m, v + the 4-float device state), five steps with
    gradients of scale 1, 1e-3, 1e-6, 0, 1 and a head that never gets a gradient (m = v = 0: the update is 0 / eps): p, m, v and
    state[0..2] after every step against the fp64 recurrences; the yardstick is torch.optim.Adam + clamp_ in fp32 on the CPU."""
    lib = _lib()
    p0, grads = R.adam_inputs(ADAM_N)
    ref = R.adam_ref(p0, grads, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale, clip)
    q = p0.clone().requires_grad_()
    opt = torch.optim.Adam([q], lr=ADAM_LR, betas=(ADAM_B1, ADAM_B2), eps=ADAM_EPS)
    p, m, v, state = p0.to(DEV), torch.zeros(ADAM_N, device=DEV), torch.zeros(ADAM_N, device=DEV), torch.zeros(4, device=DEV)
    tab = _Table('adam scale=%g clip=%g' % (grad_scale, clip))
    for it, g in enumerate(grads):
        q.grad = g * grad_scale                                 # a power of two: exact
        opt.step()
        if clip > 0:
            with torch.no_grad():
                q.clamp_(-clip, clip)
        gd = g.to(DEV)
        _ok(lib.srhip_adam_step(_p(p), _p(gd), _p(m), _p(v), _p(state), ADAM_N, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale, clip,
                                _stream()), 'adam_step')
        rp, rm, rv, rs = ref[it]
        tab.check('step %d p' % (it + 1), p, rp, q.detach())
        tab.check('step %d m' % (it + 1), m, rm, opt.state[q]['exp_avg'])
        tab.check('step %d v' % (it + 1), v, rv, opt.state[q]['exp_avg_sq'])
        for j, nm in enumerate(('step', 'lr/(1-b1^t)', 'sqrt(1-b2^t)')):
            tab.check('step %d state %s' % (it + 1, nm), state[j:j + 1], torch.tensor([rs[j]], dtype=torch.float64))
    frozen = p0[:R.ADAM_FROZEN].clamp(-clip, clip) if clip > 0 else p0[:R.ADAM_FROZEN]
    assert torch.equal(p[:R.ADAM_FROZEN].cpu(), frozen) and float(m[:R.ADAM_FROZEN].abs().max()) == 0.0
    tab.done()


# --------------------------------------------------------------------------------------------- #
# validation metrics
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('c', [1, 3, 4, 5])                 # C = 5: the per-pixel SSIM kernel; C <= 4: the tiled one
@pytest.mark.parametrize('h,w', [(7, 7),                    # one interior pixel
                                 (7, 23), (38, 16),         # tiles straddle the 16-pixel grid in one axis only
                                 (22, 22), (23, 39)])       # exactly one tile; one pixel past the grid in both axes
def test_validation_metrics_at_tile_edges(h, w, c):
    """quantized_metrics (MSE, PSNR, ERGAS, SSIM of the uint8-quantised images) against the oracle's numpy arithmetic at the
    project's bound of 1e-9; values in [-0.1, 1.1] exercise the wrap; the third image is an identical pair: MSE 0, PSNR inf, SSIM 1."""
    from sradsgan_amd.validate import quantized_metrics
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c)
    sr = torch.rand(3, c, h, w, generator=g) * 1.2 - 0.1
    hr = torch.rand(3, c, h, w, generator=g) * 1.2 - 0.1
    hr[2] = sr[2]
    got = {k: v.cpu() for k, v in quantized_metrics(sr.to(DEV), hr.to(DEV), 4).items()}
    for b in range(3):
        a_img, t_img = R.to_uint8_hwc(sr[b]), R.to_uint8_hwc(hr[b])
        want = dict(mse=R.mse_u8(t_img, a_img), psnr=R.psnr_u8(t_img, a_img), ergas=R.ergas2(t_img, a_img, 4), ssim=R.ssim_u8(a_img, t_img))
        for k, wv in want.items():
            gv = float(got[k][b])
            print('metrics %dx%dx%d image %d %-5s got %.12g want %.12g' % (h, w, c, b, k, gv, wv))
            assert (gv == wv) if math.isinf(wv) else abs(gv - wv) < 1e-9, (b, k, gv, wv)
    assert float(got['mse'][2]) == 0.0 and math.isinf(float(got['psnr'][2])) and abs(float(got['ssim'][2]) - 1.0) < 1e-9
