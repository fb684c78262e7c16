"""csrc/cbam.hip -- the discriminator's attention primitives, of which the WGAN-GP double backward is composed -- one primitive at a
time through the C ABI (ctypes) against the references of tests/pointwise_ref.py, at the shapes where the launch geometry changes
(P.CBAM_SHAPES) and on the input families built to make the first-index and NaN rules decisive (random, ties, nan).

Protocol of tests/test_reductions_gpu.py: outputs start as NaN (integers: -7) inside a larger allocation with a 64-element sentinel
band on both sides, which must be unchanged afterwards; where a kernel does arithmetic, err = max|got - ref64| / max|ref64| per
output tensor against the bar max(8 x err of stock fp32 torch on the CPU, 32 * 2^-24), every figure printed before the assert; where
it does none, or one rounding (arg-max indices, max values, the fixed_arg max row, scale), bit equality with the fp32 reference.
unpool computes a * inv + m, which a compiler may contract, so it is bounded against fp64 instead."""
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_ref as P
from tests import reduction_ref as R
from tests.test_reductions_gpu import _Table, _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
IDS = [P.shape_id(s) for s in P.CBAM_SHAPES]

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _input(shape, family):
    """(x, expect) of a finite family, once per module."""
    return _once(('x', shape, family), lambda: (P.cbam_random(shape), None) if family == 'random' else P.cbam_ties(shape))


def _G(*shape, dtype=torch.float32):
    return P.Guarded(shape, DEV, dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _exact(tab, name, got, ref):
    tab.same_bits(name, _bits(got), _bits(ref.to(got.dtype) if not got.dtype.is_floating_point else ref))


def _bands(tab, **outs):
    for name, g in outs.items():
        if not g.bands_intact():
            tab.bad.append((name, 'sentinel band overwritten'))


def _pool(over, x_dev, shape, fixed=None):
    """srhip_cbam_pool_hw / _c on a device tensor.  fixed: an int32 device arg table to re-pool at.  Returns guarded t and arg."""
    n, c, h, w = shape
    hw = h * w
    t = _G(n, 2, c) if over == 'hw' else _G(n, hw, 2)
    if fixed is None:
        arg = _G(n, c, dtype=torch.int32) if over == 'hw' else _G(n, hw, dtype=torch.int32)
        ap = arg.ptr()
    else:
        arg, ap = None, fixed.data_ptr()
    entry = _lib().srhip_cbam_pool_hw if over == 'hw' else _lib().srhip_cbam_pool_c
    _ok(entry(x_dev.data_ptr(), t.ptr(), ap, int(fixed is not None), n, hw, c, _stream()), 'cbam_pool_' + over)
    torch.cuda.synchronize()
    return t, arg


def _check_pool(tab, over, x, shape, nan_places=()):
    """mean under the bar, max and arg exact; columns / rows that hold a NaN: mean and max NaN, arg the first NaN."""
    ref_mean, ref_max, ref_arg = P.pool_hw_ref(x) if over == 'hw' else P.pool_c_ref(x)
    t, arg = _pool(over, x.to(DEV), shape)
    _bands(tab, **{over + ' t': t, over + ' arg': arg})
    tt = t.t.cpu()
    mean, mx = (tt[:, 0], tt[:, 1]) if over == 'hw' else (tt[..., 0], tt[..., 1])
    _exact(tab, 'pool_%s max' % over, mx, ref_max)
    _exact(tab, 'pool_%s arg' % over, arg.t, ref_arg)
    t32 = x.mean(1 if over == 'hw' else 2)
    keep = ~torch.isnan(ref_mean)
    if nan_places:
        tab.same_bits('pool_%s NaN set of the mean' % over, torch.isnan(mean), ~keep)
        want = {(b, ch) for b, p, ch in nan_places} if over == 'hw' else {(b, p) for b, p, ch in nan_places}
        tab.same_bits('pool_%s NaN set of the max' % over, torch.isnan(mx).nonzero(), torch.tensor(sorted(want)))
    if bool(keep.any()):                                                           # 1x4x1x1 has one pixel: its only channel mean is the NaN one
        tab.check('pool_%s mean' % over, mean[keep], ref_mean[keep], t32[keep])
    return arg.t.cpu()


@pytest.mark.parametrize('family', ['random', 'ties'])
@pytest.mark.parametrize('shape', P.CBAM_SHAPES, ids=IDS)
def test_pools_mean_max_and_first_argmax(shape, family):
    """srhip_cbam_pool_hw / srhip_cbam_pool_c, fixed_arg = 0.  ties: the planted pairs (different pixel lanes with the later pixel
    in the earlier lane; channels one butterfly step apart; inside one float4; constant rows) must give the index the plant names."""
    x, expect = _input(shape, family)
    tab = _Table('cbam pool %s %s' % (P.shape_id(shape), family))
    arg = _check_pool(tab, 'hw', x, shape)
    argc = _check_pool(tab, 'c', x, shape)
    if expect:
        for b, ch, pix in expect['hw']:
            if int(arg[b, ch]) != pix:
                tab.bad.append(('planted pixel tie', (b, ch), int(arg[b, ch]), pix))
        for b, pix, ch in expect['c']:
            if int(argc[b, pix]) != ch:
                tab.bad.append(('planted channel tie', (b, pix), int(argc[b, pix]), ch))
    tab.done()


@pytest.mark.parametrize('shape', P.CBAM_SHAPES, ids=IDS)
def test_pools_surface_a_nan_and_point_at_the_first_one(shape):
    """One NaN per variant (channels 0, 1, 4, 128, c-1; pixel lanes 0..3), and a variant with a second NaN in the same column and a
    third in the same row: the pooled max of exactly that channel / pixel is NaN, arg is the first NaN, everything else is untouched
    and equal to the reference."""
    for k, (x, places) in enumerate(P.cbam_nan_variants(shape)):
        tab = _Table('cbam pool %s nan #%d %s' % (P.shape_id(shape), k, places))
        _check_pool(tab, 'hw', x, shape, places)
        _check_pool(tab, 'c', x, shape, places)
        tab.done()


@pytest.mark.parametrize('family', ['random', 'ties'])
@pytest.mark.parametrize('shape', P.CBAM_SHAPES, ids=IDS)
def test_repool_at_a_given_table_unpool_and_their_adjointness(shape, family):
    """fixed_arg != 0 with a seeded table that is NOT the arg-max of x: the max row is x at the table's position, bit for bit, and the
    table is only read.  unpool_hw / unpool_c of random gate tensors against fp64.  Adjointness from device outputs in fp64:
    <repool(x; arg), g> = <x, unpool(g; arg)> with g = repool(x; arg) itself, so that the products do not cancel."""
    n, c, h, w = shape
    hw = h * w
    x, _ = _input(shape, family)
    xd = x.to(DEV)
    gen = torch.Generator().manual_seed(17 + hw + c)
    tab = _Table('cbam repool/unpool %s %s' % (P.shape_id(shape), family))
    lib = _lib()
    for over in ('hw', 'c'):
        table = P.random_arg_table(shape, over)
        td = table.to(DEV)
        t, _ = _pool(over, xd, shape, fixed=td)
        _bands(tab, t=t)
        tab.same_bits('repool_%s leaves the table alone' % over, td.cpu(), table)
        ref_mean, ref_at = (P.repool_hw_ref if over == 'hw' else P.repool_c_ref)(x, table)
        tt = t.t.cpu()
        mean, at = (tt[:, 0], tt[:, 1]) if over == 'hw' else (tt[..., 0], tt[..., 1])
        _exact(tab, 'repool_%s x at the table' % over, at, ref_at)
        tab.check('repool_%s mean' % over, mean, ref_mean, x.mean(1 if over == 'hw' else 2))
        # unpool of a random gate tensor
        gate = torch.randn(tt.shape, generator=gen)
        out = _G(n, hw, c)
        entry = lib.srhip_cbam_unpool_hw if over == 'hw' else lib.srhip_cbam_unpool_c
        _ok(entry(gate.to(DEV).data_ptr(), td.data_ptr(), out.ptr(), n, hw, c, _stream()), 'cbam_unpool_' + over)
        torch.cuda.synchronize()
        _bands(tab, out=out)
        if over == 'hw':
            ref = P.unpool_hw_ref(gate, table, hw)
            hit = torch.arange(hw).view(1, hw, 1) == table.long().unsqueeze(1)
            t32 = gate[:, 0].unsqueeze(1) / hw + hit.float() * gate[:, 1].unsqueeze(1)
        else:
            ref = P.unpool_c_ref(gate, table, c)
            hit = torch.arange(c).view(1, 1, c) == table.long().unsqueeze(2)
            t32 = gate[..., 0].unsqueeze(2) / c + hit.float() * gate[..., 1].unsqueeze(2)
        tab.check('unpool_%s' % over, out.t, ref, t32)
        # adjointness, g = the device's own re-pool
        out = _G(n, hw, c)
        _ok(entry(t.t.data_ptr(), td.data_ptr(), out.ptr(), n, hw, c, _stream()), 'cbam_unpool_' + over)
        torch.cuda.synchronize()
        lhs = (tt.double() * tt.double()).sum().view(1)
        rhs = (x.double() * out.t.cpu().double()).sum().view(1)
        rt = torch.stack([ref_mean, ref_at.double()], 1 if over == 'hw' else 2)
        exact = (rt * rt).sum().view(1)
        t32 = torch.stack([x.mean(1 if over == 'hw' else 2), ref_at], 1 if over == 'hw' else 2)
        tab.check('adjoint_%s <repool x, g>' % over, lhs, exact, (t32 * t32).sum().view(1))
        tab.check('adjoint_%s <x, unpool g>' % over, rhs, exact, (t32 * t32).sum().view(1))
        tab.check('adjoint_%s both sides' % over, lhs, rhs, (t32 * t32).sum().view(1), exact)
    tab.done()


@pytest.mark.parametrize('family', ['random', 'ties'])
@pytest.mark.parametrize('shape', P.CBAM_SHAPES, ids=IDS)
def test_scale_is_one_multiply_and_dot_meets_the_bar(shape, family):
    """srhip_cbam_scale modes 0 and 1: bit equality with the fp32 product; srhip_cbam_dot modes 0 and 1 against fp64."""
    n, c, h, w = shape
    hw = h * w
    x, _ = _input(shape, family)
    b = _once(('b', shape), lambda: P.cbam_random(shape, 2))
    xd, bd = x.to(DEV), b.to(DEV)
    gen = torch.Generator().manual_seed(23 + hw + c)
    tab = _Table('cbam scale/dot %s %s' % (P.shape_id(shape), family))
    lib = _lib()
    for mode in (0, 1):
        s = torch.rand((n, c) if mode == 0 else (n, hw), generator=gen) * 2 - 0.5
        out = _G(n, hw, c)
        _ok(lib.srhip_cbam_scale(xd.data_ptr(), s.to(DEV).data_ptr(), out.ptr(), n, hw, c, mode, _stream()), 'cbam_scale')
        torch.cuda.synchronize()
        _bands(tab, scale=out)
        _exact(tab, 'scale mode %d' % mode, out.t, P.scale_ref(x, s, mode))
        d = _G(n, c) if mode == 0 else _G(n, hw)
        _ok(lib.srhip_cbam_dot(xd.data_ptr(), bd.data_ptr(), d.ptr(), n, hw, c, mode, _stream()), 'cbam_dot')
        torch.cuda.synchronize()
        _bands(tab, dot=d)
        tab.check('dot mode %d' % mode, d.t, P.dot_ref(x, b, mode), (x * b).sum(1 if mode == 0 else 2))
    tab.done()


@pytest.mark.parametrize('pair', [0, 1])
@pytest.mark.parametrize('n,c', P.SIGMOID_CASES)
def test_sigmoid_forward_backward_and_double_backward(n, c, pair):
    """srhip_sigmoid_fwd / _bwd / _bwd_bwd.  The inputs hold 0, -0.0, +-20, +-88, +-100 and +-inf: no NaN anywhere, exactly 0 or 1
    where expf saturates.  bwd and bwd_bwd are referred to the y the forward wrote (the reference differentiates at that y);
    bwd_bwd with dg NULL, with dy NULL and with both outputs."""
    x, g, gg, placed = P.sigmoid_inputs(n, c, bool(pair))
    lib = _lib()
    cnt = n * c
    tab = _Table('sigmoid n %d c %d pair %d' % (n, c, pair))
    xd, gd, ggd = x.to(DEV), g.to(DEV), gg.to(DEV)
    y = _G(n, c)
    _ok(lib.srhip_sigmoid_fwd(xd.data_ptr(), y.ptr(), cnt, c, pair, _stream()), 'sigmoid_fwd')
    torch.cuda.synchronize()
    _bands(tab, y=y)
    yc = y.t.cpu()
    tab.check('sigmoid_fwd', yc, P.sigmoid_ref(x, bool(pair)), torch.sigmoid(x[:, 0] + x[:, 1]) if pair else torch.sigmoid(x))
    for k, v in placed:
        if v in P.SIGMOID_SATURATED and float(yc.view(-1)[k]) != P.SIGMOID_SATURATED[v]:
            tab.bad.append(('saturation', v, float(yc.view(-1)[k])))
    yd = y.t.contiguous()
    dx = _G(*x.shape)
    _ok(lib.srhip_sigmoid_bwd(gd.data_ptr(), yd.data_ptr(), dx.ptr(), cnt, c, pair, _stream()), 'sigmoid_bwd')
    torch.cuda.synchronize()
    _bands(tab, dx=dx)
    d32 = g * (yc * (1 - yc))
    tab.check('sigmoid_bwd', dx.t, P.sigmoid_bwd_ref(g, yc, bool(pair)), torch.stack([d32, d32], 1) if pair else d32)
    rdg, rdy = P.sigmoid_bwd_bwd_ref(gg, g, yc, bool(pair))
    u32 = gg[:, 0] + gg[:, 1] if pair else gg
    tdg, tdy = u32 * (yc * (1 - yc)), u32 * g * (1 - 2 * yc)
    for want_dg, want_dy in ((1, 1), (0, 1), (1, 0)):
        dg, dy = _G(n, c), _G(n, c)
        _ok(lib.srhip_sigmoid_bwd_bwd(ggd.data_ptr(), gd.data_ptr(), yd.data_ptr(), dg.ptr() if want_dg else None, dy.ptr() if want_dy else None,
                                      cnt, c, pair, _stream()), 'sigmoid_bwd_bwd')
        torch.cuda.synchronize()
        _bands(tab, dg=dg, dy=dy)
        which = 'dg %d dy %d' % (want_dg, want_dy)
        if want_dg:
            tab.check('bwd_bwd dg (%s)' % which, dg.t, rdg, tdg)
        if want_dy:
            tab.check('bwd_bwd dy (%s)' % which, dy.t, rdy, tdy)
        if (not want_dg and not dg.untouched()) or (not want_dy and not dy.untouched()):
            tab.bad.append(('bwd_bwd wrote an output it was not given', which))
    tab.done()


def test_refusals_leave_every_buffer_untouched():
    """c % 4 != 0, n / hw / c <= 0, a null tensor, a tensor the entry checks for 16-byte alignment passed 4 bytes off, a mode other
    than 0 or 1: every call returns SRHIP_ERR_ARG from the host-side checks, and nothing -- output, input or band -- is written."""
    lib = _lib()
    bufs = {k: _G(64, dtype=torch.int32 if k == 'arg' else torch.float32) for k in ('x', 't', 'arg', 'out', 's')}
    calls = P.cbam_refusals(lib, {k: g.ptr() for k, g in bufs.items()})
    bad = []
    for label, call in calls:
        rc = call()
        if rc == 0 or not lib.srhip_last_error():
            bad.append((label, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(g.untouched() for g in bufs.values()), [k for k, g in bufs.items() if not g.untouched()]


# --------------------------------------------------------------------------------------------- #
# through autograd: ops.clam -> ops.slam on the tie family
# --------------------------------------------------------------------------------------------- #


def _restated(x, fc1, fc2, w7):
    """ChannelAttention -> SpatialAttention (base_networks.py:387-403, 440-457) with both max pools routed to the REFERENCE's first
    maximum (P.first_max), so that first- and second-order gradients under ties are defined the way the kernels define them."""
    b, c, h, w = x.shape
    mlp = lambda v: F.conv2d(F.relu(F.conv2d(v, fc1)), fc2)
    flat = x.flatten(2)
    arg = P.first_max(flat.detach(), 2)[1]
    mx = flat.gather(2, arg.unsqueeze(2)).view(b, c, 1, 1)
    s = torch.sigmoid(mlp(x.mean((2, 3), keepdim=True)) + mlp(mx))
    y = s * x
    argc = P.first_max(y.detach(), 1)[1]
    pooled = torch.cat([y.mean(1, keepdim=True), y.gather(1, argc.unsqueeze(1))], 1)
    return torch.sigmoid(F.conv2d(pooled, w7, padding=3)) * y


def test_attention_pair_on_ties_first_and_second_order():
    """The srhip_cbam_* composition on the ties family at 2x68x5x7 (a ragged second channel block, hw no multiple of 4), in the shape
    of test_attention_gpu's pair test: forward, first-order gradient and the gradient-penalty pattern, against the fp64 restatement
    that uses the reference's arg-max.  The convolutions inside run in fp32 arithmetic here (srhip_set_conv_math(0)): the bar is the
    protocol's, set by stock fp32 torch, and the subject is the primitives, not the split-bf16 contraction."""
    from sradsgan_amd import ops
    shape = P.AUTOGRAD_SHAPE
    b, c, h, w = shape
    x = P.cbam_ties(shape)[0].view(b, h, w, c).permute(0, 3, 1, 2).contiguous()
    gen = torch.Generator().manual_seed(41)
    rnd = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    dy, r = rnd(b, c, h, w), rnd(b, c, h, w)
    fc1, fc2, w7 = 0.3 * rnd(c // 16, c, 1, 1), 0.3 * rnd(c, c // 16, 1, 1), 0.3 * rnd(1, 2, 7, 7)

    def run(dev, dtype):
        xs, f1, f2, k7 = (t.to(dev, dtype).requires_grad_(True) for t in (x, fc1, fc2, w7))
        out = _restated(xs, f1, f2, k7) if dev == 'cpu' else ops.slam(ops.clam(xs, f1, f2), k7)
        (gx,) = torch.autograd.grad(out, xs, dy.to(dev, dtype), create_graph=True)
        pen = (gx * r.to(dev, dtype)).sum() + 0.1 * (gx * gx).sum()
        g2 = torch.autograd.grad(pen, [xs, f1, f2, k7])
        return [out.detach(), gx.detach()] + list(g2)
    ref, t32 = run('cpu', torch.float64), run('cpu', torch.float32)
    lib = _lib()
    math = lib.srhip_get_conv_math()
    lib.srhip_set_conv_math(0)
    try:
        got = run(DEV, torch.float32)
        torch.cuda.synchronize()
    finally:
        lib.srhip_set_conv_math(math)
    tab = _Table('clam -> slam on ties ' + P.shape_id(shape))
    for name, a_, r_, t_ in zip(('out', 'dx', 'pen/dx', 'pen/dfc1', 'pen/dfc2', 'pen/dw7'), got, ref, t32):
        tab.check(name, a_, r_, t_)
    tab.done()
