"""The references of tests/pointwise_ref.py against stock torch in fp64 wherever torch defines the operation (pools and their
autograd, max_pool2d o relu, pixel_shuffle + leaky_relu for r = 2, 3, 4, sigmoid under double autograd, cat), the first-index rule on
the tie families asserted explicitly, and -- for every reduction case of test_cbam_gpu.py -- an fp32 emulation of the kernel's own
summation order held to the bar of that test: a correct kernel can pass.  The argument refusals of every entry point need the
library but no device.  No GPU call is made here."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_ref as P
from tests import reduction_ref as R

SMALL = [s for s in P.CBAM_SHAPES if s != P.CBAM_BIG]
IDS = [P.shape_id(s) for s in SMALL]


def _nchw(x, shape):
    n, c, h, w = shape
    return x.view(n, h, w, c).permute(0, 3, 1, 2)


# --------------------------------------------------------------------------------------------- #
# pools, unpools, scale / dot
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('shape', SMALL, ids=IDS)
def test_pool_references_are_torch_pools_and_their_autograd(shape):
    n, c, h, w = shape
    hw = h * w
    x = P.cbam_random(shape).double()
    x4 = _nchw(x, shape)
    mean, mx, arg = P.pool_hw_ref(x)
    assert torch.allclose(mean, F.adaptive_avg_pool2d(x4, 1).view(n, c), rtol=0, atol=1e-15)
    assert torch.equal(mx, F.adaptive_max_pool2d(x4, 1).view(n, c))
    assert torch.equal(arg, x.max(1).indices)                                  # no ties in this family
    meanc, mxc, argc = P.pool_c_ref(x)
    assert torch.allclose(meanc, x4.mean(1).reshape(n, hw), rtol=0, atol=1e-15)
    assert torch.equal(mxc, x4.max(1).values.reshape(n, hw)) and torch.equal(argc, x.max(2).indices)
    # the unpool is the pool's vector-Jacobian product
    g = torch.Generator().manual_seed(3)
    t_hw, t_c = torch.randn(n, 2, c, generator=g).double(), torch.randn(n, hw, 2, generator=g).double()
    xr = x.clone().requires_grad_()
    pooled = torch.stack([xr.mean(1), xr.max(1).values], 1)
    (vjp,) = torch.autograd.grad(pooled, xr, t_hw)
    assert torch.allclose(P.unpool_hw_ref(t_hw, arg, hw), vjp, rtol=0, atol=1e-14)
    pooled = torch.stack([xr.mean(2), xr.max(2).values], 2)
    (vjp,) = torch.autograd.grad(pooled, xr, t_c)
    assert torch.allclose(P.unpool_c_ref(t_c, argc, c), vjp, rtol=0, atol=1e-14)
    # ... and the re-pool (at ANY arg table) is the unpool's, the unpool written with stock scatter
    for over in ('hw', 'c'):
        tab = P.random_arg_table(shape, over)
        gx = torch.randn(n, hw, c, generator=g).double()
        t = (t_hw if over == 'hw' else t_c).clone().requires_grad_()
        if over == 'hw':
            out = (t[:, 0] / hw).unsqueeze(1) + torch.zeros(n, hw, c, dtype=torch.float64).scatter(1, tab.long().unsqueeze(1), t[:, 1].unsqueeze(1))
            assert torch.equal(out.detach(), P.unpool_hw_ref(t.detach(), tab, hw))
            rm, rx = P.repool_hw_ref(gx, tab)
            want = torch.stack([rm, rx], 1)
        else:
            out = (t[..., 0] / c).unsqueeze(2) + torch.zeros(n, hw, c, dtype=torch.float64).scatter(2, tab.long().unsqueeze(2), t[..., 1].unsqueeze(2))
            assert torch.equal(out.detach(), P.unpool_c_ref(t.detach(), tab, c))
            rm, rx = P.repool_c_ref(gx, tab)
            want = torch.stack([rm, rx], 2)
        (vjp,) = torch.autograd.grad(out, t, gx)
        assert torch.allclose(want, vjp, rtol=0, atol=1e-14)


@pytest.mark.parametrize('shape', SMALL, ids=IDS)
def test_tie_family_routes_to_the_first_index(shape):
    """The planted ties force the index the plants name; every index is the first maximal one (a plain loop over the small shapes);
    the values equal torch's, which do not depend on the index."""
    n, c, h, w = shape
    hw = h * w
    x, expect = P.cbam_ties(shape)
    _, mx, arg = P.pool_hw_ref(x)
    _, mxc, argc = P.pool_c_ref(x)
    assert torch.equal(mx, x.amax(1)) and torch.equal(mxc, x.amax(2))
    for b, ch, pix in expect['hw']:
        assert int(arg[b, ch]) == pix, ('hw', b, ch, int(arg[b, ch]), pix)
        assert int((x[b, :, ch] == mx[b, ch]).sum()) >= min(2, hw)                        # the tie is real
    for b, pix, ch in expect['c']:
        assert int(argc[b, pix]) == ch, ('c', b, pix, int(argc[b, pix]), ch)
        assert int((x[b, pix, :] == mxc[b, pix]).sum()) >= 2
    if n * hw * c <= 20000:
        xs = x.tolist()
        for b in range(n):
            for ch in range(c):
                col = [xs[b][p][ch] for p in range(hw)]
                assert int(arg[b, ch]) == col.index(max(col))
            for p in range(hw):
                assert int(argc[b, p]) == xs[b][p].index(max(xs[b][p]))
    # planted hw pairs sit in different pixel lanes, the later pixel in the earlier lane; planted channel pairs differ in one lane bit
    for p1, p2 in P.HW_TIE_PAIRS:
        assert p1 < p2 and p1 % 4 > p2 % 4
    assert sorted((P.C_TIE_BASE ^ (1 << b)) for b in range(2, 8)) == sorted({14 ^ 4, 14 ^ 8, 14 ^ 16, 14 ^ 32, 14 ^ 64, 14 ^ 128})
    assert P.C_TIE_QUAD[0] // 4 == P.C_TIE_QUAD[1] // 4


@pytest.mark.parametrize('shape', SMALL, ids=IDS)
def test_nan_family_gives_nan_and_the_first_nan(shape):
    """The rule of csrc/common.h, computed explicitly: ATen is an oracle for the VALUE only (its indices under NaN differ between
    adaptive_max_pool2d and max(dim))."""
    n, c, h, w = shape
    base = P.cbam_random(shape)
    _, bmx, barg = P.pool_hw_ref(base)
    _, bmxc, bargc = P.pool_c_ref(base)
    for x, places in P.cbam_nan_variants(shape):
        assert int(torch.isnan(x).sum()) == len(places)
        _, mx, arg = P.pool_hw_ref(x)
        _, mxc, argc = P.pool_c_ref(x)
        tv = F.adaptive_max_pool2d(_nchw(x, shape), 1).view(n, c)
        assert torch.equal(torch.isnan(mx), torch.isnan(tv)) and torch.equal(mx[~torch.isnan(mx)], tv[~torch.isnan(tv)])
        tv = _nchw(x, shape).max(1).values.reshape(n, h * w)
        assert torch.equal(torch.isnan(mxc), torch.isnan(tv)) and torch.equal(mxc[~torch.isnan(mxc)], tv[~torch.isnan(tv)])
        cols = {(b, ch) for b, p, ch in places}
        rows = {(b, p) for b, p, ch in places}
        assert int(torch.isnan(mx).sum()) == len(cols) and int(torch.isnan(mxc).sum()) == len(rows)
        for b, ch in cols:
            assert torch.isnan(mx[b, ch]) and int(arg[b, ch]) == min(p for bb, p, cc in places if (bb, cc) == (b, ch))
        for b, p in rows:
            assert torch.isnan(mxc[b, p]) and int(argc[b, p]) == min(cc for bb, pp, cc in places if (bb, pp) == (b, p))
        keep = ~torch.isnan(mx)
        assert torch.equal(mx[keep], bmx[keep]) and torch.equal(arg[keep], barg[keep])
        keep = ~torch.isnan(mxc)
        assert torch.equal(mxc[keep], bmxc[keep]) and torch.equal(argc[keep], bargc[keep])


def test_scale_and_dot_references():
    shape = (2, 68, 1, 3)
    n, c, h, w = shape
    x, y = P.cbam_random(shape).double(), P.cbam_random(shape, 1).double()
    s0, s1 = x[:, 0, :].clone(), x[:, :, 0].clone()
    for mode, s in ((0, s0), (1, s1)):
        sr = s.clone().requires_grad_()
        out = x * (sr[:, None, :] if mode == 0 else sr[:, :, None])
        assert torch.equal(P.scale_ref(x, s, mode), out.detach())
        (ds,) = torch.autograd.grad(out, sr, y)                                  # dot is the adjoint of scale w.r.t. s
        assert torch.allclose(P.dot_ref(y, x, mode), ds, rtol=0, atol=1e-14)


# --------------------------------------------------------------------------------------------- #
# the bar of the GPU tests is reachable: fp32 emulation of the kernels' summation order
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('family', ['random', 'ties'])
@pytest.mark.parametrize('shape', P.CBAM_SHAPES, ids=[P.shape_id(s) for s in P.CBAM_SHAPES])
def test_a_correct_kernel_meets_the_bar_of_every_reduction_case(shape, family):
    """pool_hw / dot mode 0: four strided pixel lanes, then (l0 + l1) + (l2 + l3); pool_c / dot mode 1: 64 strided lanes of float4
    partials, then the xor butterfly.  Held to max(8 x stock fp32 torch, 32 * 2^-24) against fp64, like the GPU test."""
    x = P.cbam_random(shape) if family == 'random' else P.cbam_ties(shape)[0]
    b = P.cbam_random(shape, 2)
    bad = []

    def check(name, got, ref, torch32):
        e, te = R.err(got, ref), R.err(torch32, ref)
        print('%-16s %-6s %-12s err %.3e  torch-fp32 %.3e  bound %.3e' % (P.shape_id(shape), family, name, e, te, R.bound(te)))
        if not e <= R.bound(te):
            bad.append((name, e, te))
    check('pool_hw mean', P.emulate_pool_hw_mean(x), P.pool_hw_ref(x)[0], x.mean(1))
    check('pool_c mean', P.emulate_pool_c_mean(x), P.pool_c_ref(x)[0], x.mean(2))
    check('dot mode 0', P.emulate_dot_hw(x, b), P.dot_ref(x, b, 0), (x * b).sum(1))
    check('dot mode 1', P.emulate_dot_c(x, b), P.dot_ref(x, b, 1), (x * b).sum(2))
    assert not bad, bad


# --------------------------------------------------------------------------------------------- #
# sigmoid family
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('n,c', P.SIGMOID_CASES)
def test_sigmoid_references_are_torch_sigmoid_under_double_autograd(n, c, pair):
    x, g, gg, placed = P.sigmoid_inputs(n, c, pair)
    y = P.sigmoid_ref(x, pair)
    assert not torch.isnan(y).any()
    for k, v in placed:
        if v in P.SIGMOID_SATURATED:
            assert abs(float(y.view(-1)[k]) - P.SIGMOID_SATURATED[v]) < 1e-43
    finite = torch.isfinite(x).all(1) if pair else torch.isfinite(x)           # torch's own double backward meets inf * 0 at +-inf
    xr = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).double().requires_grad_()
    yr = torch.sigmoid(xr[:, 0] + xr[:, 1]) if pair else torch.sigmoid(xr)
    assert torch.allclose(yr.detach()[finite], y[finite], rtol=1e-14, atol=1e-300)
    (dx,) = torch.autograd.grad(yr, xr, g.double(), create_graph=True)
    assert torch.allclose(dx.detach(), P.sigmoid_bwd_ref(g, yr.detach(), pair), rtol=1e-13, atol=1e-300)
    # bwd_bwd: the gradients of <gg, dx(g, y)> at g and y, dx = g y (1 - y) as a function of (g, y)
    gv, yv = g.double().requires_grad_(), yr.detach().clone().requires_grad_()
    d = gv * yv * (1 - yv)
    dg, dy = torch.autograd.grad(torch.stack([d, d], 1) if pair else d, [gv, yv], gg.double())
    rdg, rdy = P.sigmoid_bwd_bwd_ref(gg, g, yr.detach(), pair)
    assert torch.allclose(dg, rdg, rtol=1e-13, atol=1e-300)
    assert torch.allclose(dy, rdy, rtol=1e-13, atol=1e-14)                       # 1 - 2 y cancels at y = 1/2: absolute there
    # and through torch's own second order: d<gg, dx>/dx_in = sigmoid_bwd(dy)
    (g2,) = torch.autograd.grad(dx, xr, gg.double())
    assert torch.allclose(g2, P.sigmoid_bwd_ref(rdy, yr.detach(), pair), rtol=1e-12, atol=1e-14)


# --------------------------------------------------------------------------------------------- #
# elementwise references
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('family', P.POOL_FAMILIES)
@pytest.mark.parametrize('shape', P.POOL_SHAPES, ids=[P.shape_id(s) for s in P.POOL_SHAPES])
def test_maxpool_references_are_max_pool2d_and_its_autograd(shape, family):
    x, dy, z = P.pool_inputs(family, shape)
    y, pos = P.maxpool2x2_ref(x)
    x4 = x.permute(0, 3, 1, 2)
    assert torch.equal(y.permute(0, 3, 1, 2), F.max_pool2d(x4, 2, 2))
    if family == 'equal':
        assert int(pos.abs().max()) == 0
    if family == 'ties':
        which = torch.arange(pos.numel()).view(pos.shape) % 6
        for k, (a, b) in enumerate(P.POOL_TIE_PAIRS):
            assert bool((pos[which == k] == a).all()) and bool((y[which == k] == 2.0).all())
        assert set(pos.unique().tolist()) == {0, 1, 2}
    if family in ('random', 'negative'):                                          # no ties: autograd's routing is unambiguous
        xr = x.double().permute(0, 3, 1, 2).requires_grad_()
        (dx,) = torch.autograd.grad(F.max_pool2d(xr, 2, 2), xr, dy.double().permute(0, 3, 1, 2))
        assert torch.equal(P.maxpool2x2_bwd_ref(dy.double(), x.double(), 0), dx.permute(0, 2, 3, 1))
    if family == 'relu':                                                          # ties only at 0, where the ReLU backward gives 0 anyway
        zr = z.double().permute(0, 3, 1, 2).requires_grad_()
        (dz,) = torch.autograd.grad(F.max_pool2d(F.relu(zr), 2, 2), zr, dy.double().permute(0, 3, 1, 2))
        assert torch.equal(P.maxpool2x2_bwd_ref(dy.double(), x.double(), 1), dz.permute(0, 2, 3, 1))
        assert bool(((x == 0) | (z == x)).all()) and int((y == 0).sum()) > 0
    dx0, dx1 = P.maxpool2x2_bwd_ref(dy, x, 0), P.maxpool2x2_bwd_ref(dy, x, 1)
    assert torch.equal(P._windows(dx0).sum(0), dy)                                # exactly one position per window takes dy
    assert torch.equal(P._windows(dx1).sum(0), torch.where(y > 0, dy, torch.zeros_like(dy)))
    if family == 'negative':
        assert int((dx1 != 0).sum()) == 0


def test_maxpool_reference_surfaces_a_nan_like_max_pool2d():
    x, _, _ = P.pool_inputs('random', (2, 4, 2, 2))
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        xn = x.clone()
        xn[1, i, j, 2] = P.NAN
        y, pos = P.maxpool2x2_ref(xn)
        ty = F.max_pool2d(xn.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(torch.isnan(y), torch.isnan(ty)) and int(torch.isnan(y).sum()) == 1 and torch.isnan(y[1, 0, 0, 2])
        assert int(pos[1, 0, 0, 2]) == k


@pytest.mark.parametrize('slope', P.SHUFFLE_ACTS)
@pytest.mark.parametrize('r', P.SHUFFLE_R)
def test_pixel_shuffle_references_are_torch_pixel_shuffle_and_leaky_relu(r, slope):
    for n, h, w in P.SHUFFLE_NHW:
        for cout in (4, 12):
            for integer in (False, True):
                x, dout = P.shuffle_inputs(n, h, w, cout, r, integer)
                xr = x.double().permute(0, 3, 1, 2).requires_grad_()
                out = F.pixel_shuffle(xr, r)
                if slope is not None:
                    out = F.leaky_relu(out, slope)
                ref = P.pixel_shuffle_ref(x.double(), r, slope)
                assert torch.equal(ref, out.detach().permute(0, 2, 3, 1))
                (din,) = torch.autograd.grad(out, xr, dout.double().permute(0, 3, 1, 2))
                assert torch.equal(P.pixel_shuffle_bwd_ref(dout.double(), ref, r, slope), din.permute(0, 2, 3, 1))
                # fp32: the references the GPU tests compare bits with
                o32 = F.pixel_shuffle(x.permute(0, 3, 1, 2), r)
                o32 = o32 if slope is None else F.leaky_relu(o32, slope)
                assert P.same_bits(P.pixel_shuffle_ref(x, r, slope), o32.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize('slope', P.LRELU_SLOPES)
def test_lrelu_backward_reference_and_mask_layout(slope):
    dy, y = P.lrelu_inputs(1023)
    ref = P.lrelu_bwd_ref(dy, y, slope)
    k = len(P.LRELU_Y_SPECIALS)
    want = [1.0 if v > 0 else slope for v in P.LRELU_Y_SPECIALS]                 # 0, -0, NaN, -inf, negative denormal: the slope
    got = (ref[:k].double() / dy[:k].double()).tolist()
    assert all(abs(a - b) < 1e-7 for a, b in zip(got, want)), (got, want)
    yr = y.clone().requires_grad_()
    (g,) = torch.autograd.grad(F.leaky_relu(yr, slope), yr, dy)
    fin = ~torch.isnan(y)
    assert P.same_bits(ref[fin], g[fin])
    # mask layout: element 4 l + e of chunk k -> bit l of 64-bit word 4 k + e
    yy = -torch.ones(2 * 256 + 8)
    yy[0], yy[1], yy[4], yy[4 * 9 + 2], yy[256 + 4 * 63 + 3], yy[512 + 5] = 1, 1, 1, 1, 1, 1
    m = P.lrelu_mask_ref(yy)
    assert m.numel() == 3 * 32
    words = [int.from_bytes(bytes(m[8 * i:8 * i + 8].tolist()), 'little') for i in range(12)]
    assert words == [0b11, 1, 1 << 9, 0, 0, 0, 0, 1 << 63, 0, 1 << 1, 0, 0]


def test_cat_and_split_references():
    for rows, chans in ((5, [4, 8, 12]), (3, [4] * 8)):
        ts = P.cat_inputs(rows, chans)
        wide = P.cat_ref(ts)
        assert torch.equal(wide, torch.cat(ts, 1))
        assert all(torch.equal(a, b) for a, b in zip(P.split_ref(wide, chans), ts))


# --------------------------------------------------------------------------------------------- #
# argument refusals: the library, no device
# --------------------------------------------------------------------------------------------- #


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


FAKE = {k: 0x10000 + 0x1000 * i for i, k in enumerate(('x', 't', 'arg', 'out', 's', 'y', 'rec', 'mask'))}   # aligned, never dereferenced


def test_every_entry_point_refuses_bad_arguments(lib):
    calls = P.cbam_refusals(lib, FAKE) + P.elementwise_refusals(lib, FAKE)
    assert len(calls) > 150
    lib.srhip_cbam_pool_hw(None, None, None, 0, 1, 1, 4, None)                  # leaves a message of another entry behind
    for label, call in calls:
        entry = label.split(':')[0].split(' ')[0]
        rc = call()
        msg = lib.srhip_last_error()
        assert rc == -1, (label, rc)
        assert msg and entry.encode() in msg, (label, msg)
    assert lib.srhip_lrelu_bwd(FAKE['y'], FAKE['x'], FAKE['out'], 0, 0.2, None) == 0        # count = 0: OK, nothing to do
    assert lib.srhip_lrelu_bwd_bits(FAKE['y'], FAKE['x'], FAKE['mask'], FAKE['out'], 0, 0.2, None) == 0
    assert [lib.srhip_lrelu_mask_bytes(v) for v in (0, 4, 252, 256, 260, 4194308)] == [0, 32, 32, 32, 64, 524320]
