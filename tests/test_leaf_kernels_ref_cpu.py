"""tests/leaf_kernels_ref.py without a GPU: every fp64 reference against torch fp64 autograd of the plain formulation (1e-12), every
fp32 order emulation against its fp64 reference under the bar the GPU tests hold (reduction_ref.bound of stock fp32 torch), the
conditions that make each input family and each case worth running (asserted on the fp64 references alone), and the refusal lists
on made-up addresses: every call returns SRHIP_ERR_ARG from the host-side checks with a message that names its entry point."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import leaf_kernels_ref as L
from tests.reduction_ref import bound, err

F64, F32 = L.F64, L.F32
TOL = 1e-12


def _close(got, want, what):
    e = err(got, want)
    assert e <= TOL, (what, e)


# --------------------------------------------------------------------------------------------- #
# the references against autograd of the plain formulations
# --------------------------------------------------------------------------------------------- #


def test_channel_attention_reference_is_the_existing_fp64_expression():
    from tests.test_drcan_gpu import ca_ref64
    n, h, w, hidden = 3, 5, 7, 5
    gen = torch.Generator().manual_seed(5)
    u, x, gout = (torch.randn(n, h * w, 64, generator=gen) for _ in range(3))
    fc1, b1 = 0.3 * torch.randn(hidden, 64, generator=gen), 0.2 * torch.randn(hidden, generator=gen)
    fc2, b2 = 0.3 * torch.randn(64, hidden, generator=gen), 0.5 * torch.randn(64, generator=gen)
    got = L.ca_chain_ref(u, x, fc1, b1, fc2, b2, gout)

    def nchw(t):
        return t.view(n, h, w, 64).permute(0, 3, 1, 2)
    out, leaves = ca_ref64(nchw(u), nchw(x), fc1.view(hidden, 64, 1, 1), b1, fc2.view(64, hidden, 1, 1), b2)
    out.backward(nchw(gout).double())
    assert float(got['s'].min()) > 0 and bool(((got['dfc1'] != 0).sum(1) > 0).any())
    _close(nchw(got['out']), out.detach(), 'out')
    _close(nchw(got['du']), leaves[0].grad, 'du')
    _close(got['dfc1'], leaves[2].grad.view(hidden, 64), 'dfc1')
    _close(got['db1'], leaves[3].grad, 'db1')
    _close(got['dfc2'], leaves[4].grad.view(64, hidden), 'dfc2')
    _close(got['db2'], leaves[5].grad, 'db2')
    # the stand-alone pieces: segment sums add up to the image sum; the fold and its backward
    _close(L.ca_partial_ref(u).sum(1), u.double().sum(1), 'segments')
    _close(L.ca_partial_ref(gout, u).sum(1), (gout.double() * u.double()).sum(1), 'product segments')
    a, b = torch.randn(3, 20, dtype=F64, generator=gen), torch.randn(20, dtype=F64, generator=gen).requires_grad_()
    g = torch.randn(3, 20, dtype=F64, generator=gen)
    o = a + 0.3 * b.unsqueeze(0).expand(3, 20)
    o.backward(g)
    _close(L.add_bcast_scaled_ref32(a, b.detach(), 0.3), o.detach(), 'add_bcast_scaled')
    _close(L.batch_sum_ref(g, 0.3), b.grad, 'batch_sum_scaled')


def test_prelu_gamma_residual_and_upsample_references_are_autograd():
    g, z = L.clean_rows(37, 12)
    for a in L.PRELU_SLOPES:
        zz, aa = z.double().requires_grad_(), torch.tensor([a], dtype=F64, requires_grad=True)
        y = F.prelu(zz, aa)
        y.backward(g.double())
        _close(L.prelu_fwd_ref32(z.double(), a), y.detach(), 'prelu y')
        _close(L.prelu_bwd_ref32(g.double(), z.double(), a), zz.grad, 'prelu dz')
        _close(L.prelu_slope_eval(g, z, F64), aa.grad, 'prelu da')
        _close(L.prelu_slope_terms(g, z).sum().reshape(1), aa.grad, 'prelu da terms')
    a, b, gg = (t.double() for t in L.gamma_inputs(100))
    bb, gamma = b.clone().requires_grad_(), torch.tensor([L.GAMMA], dtype=F64, requires_grad=True)
    out = a + gamma * bb
    out.backward(gg)
    _close(L.gamma_fwd_ref32(a, b, L.GAMMA), out.detach(), 'gamma out')
    _close(L.gamma_db_ref32(gg, L.GAMMA), bb.grad, 'gamma db')
    _close(L.gamma_sum_eval(gg, b, F64), gamma.grad, 'dgamma')
    # y = r + alpha c, z = s + beta y under <dz, z>: dc = alpha beta dz, dr = beta dz (+ kc e: a second consumer of r with gradient e)
    r, c, s, dz, e = (t.double() for t in L.rows_inputs(9, 8, 5, 0))
    rr, cc = r.clone().requires_grad_(), c.clone().requires_grad_()
    y = rr + 0.2 * cc
    zz = s + 0.3 * y
    ((zz * dz).sum() + 0.7 * (rr * e).sum()).backward()
    yr, zr = L.scaled_res_fwd_ref32(r, c, s, 0.2, 0.3)
    _close(yr, y.detach(), 'scaled_res y')
    _close(zr, zz.detach(), 'scaled_res z')
    dc, dr = L.scaled_res_bwd_ref32(dz, e, 0.2 * 0.3, 0.3, 0.7)
    _close(dc, cc.grad, 'scaled_res dc')
    _close(dr, rr.grad, 'scaled_res dr')
    assert L.scaled_res_fwd_ref32(r, None, None, 0.2, 0.3)[0] is r and L.scaled_res_fwd_ref32(r, None, None, 0.2, 0.3)[1] is None
    x = r.clone().requires_grad_()
    yl = F.leaky_relu(x, 0.2)
    yl.backward(dz)
    _close(L.lrelu_bwd_strided_ref32(dz, yl.detach(), 0.2), x.grad, 'lrelu_bwd_strided')
    for rr_ in L.UP_R:
        x = torch.randn(2, 3, 5, 8, dtype=F64).requires_grad_()
        up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=rr_, mode='nearest').permute(0, 2, 3, 1)
        dy = torch.randn(up.shape, dtype=F64)
        up.backward(dy)
        assert torch.equal(L.upsample_nearest_ref(x.detach(), rr_), up.detach())
        _close(L.upsample_nearest_bwd_ref(dy, rr_), x.grad, 'upsample bwd')


def _nl_autograd(inp):
    th, ph, g = (inp[k].double().requires_grad_() for k in ('theta', 'phi', 'g'))
    n, h, w, _ = th.shape
    y = torch.zeros(n, h, w, 8, dtype=F64)
    for r0, r1, c0, c1 in L.nl_quadrants(h, w):
        for b in range(n):
            t, k, v = (x[b, r0:r1, c0:c1].reshape(-1, 8) for x in (th, ph, g))
            y[b, r0:r1, c0:c1] = (torch.softmax(t @ k.t(), -1) @ v).view(r1 - r0, c1 - c0, 8)
    y.backward(inp['dy'].double())
    return dict(y=y.detach(), dtheta=th.grad, dphi=ph.grad, dg=g.grad)


@pytest.mark.parametrize('family', L.NL_FAMILIES)
def test_quadrant_attention_reference_is_autograd_of_the_per_quadrant_softmax(family):
    for n, h, w in ((2, 3, 2), (2, 5, 7), (1, 2, 2)):
        inp = L.nl_inputs(family, n, h, w)
        ref, auto = L.nl_eval(inp, F64), _nl_autograd(inp)
        scales = L.nl_scales(family, inp)
        for k, v in auto.items():
            assert L.scaled_err(ref[k], v, scales.get(k)) <= TOL, (family, (n, h, w), k)
        lg = torch.cat([s.reshape(-1) for s in L.nl_logits(inp)])
        assert float(ref['m'].max()) == float(lg.max()) and float(ref['l'].min()) >= 1.0


# --------------------------------------------------------------------------------------------- #
# the order emulations against their fp64 references, under the GPU tests' bar
# --------------------------------------------------------------------------------------------- #


def _under(label, got, ref, yard, scale=None, bad=None):
    e, te = L.scaled_err(got, ref, scale), L.scaled_err(yard, ref, scale)
    print('%-40s emulation %.3e  torch-fp32 %.3e  bound %.3e' % (label, e, te, bound(te)))
    if not e <= bound(te):
        bad.append((label, e, te))


def test_order_emulations_meet_the_bar_of_stock_fp32():
    bad = []
    for n, hw in [(3, hw) for hw in L.CA_HW]:
        t = L.ca_inputs(n, hw)
        for label, a, b in (('ca_pool_sum', t['u'], None), ('ca_bwd_partial', t['g'], t['u'])):
            v = a if b is None else a * b
            yard = torch.stack([v[:, p0:p1].sum(1) for p0, p1 in L.seg_bounds(hw)], 1)
            emu = L.emulate_ca_partial(a, b)
            _under('%s %dx%d' % (label, n, hw), emu, L.ca_partial_ref(a, b), yard, bad=bad)
            empty = [s for s, (p0, p1) in enumerate(L.seg_bounds(hw)) if p1 == p0]
            assert L.exact(emu[:, empty], torch.zeros(n, len(empty), 64))
    g = torch.randn(5, 1028, generator=torch.Generator().manual_seed(3)) + 0.5
    _under('batch_sum_scaled', L.emulate_batch_sum_scaled(g, 0.3), L.batch_sum_ref(g, 0.3), f32_mul(g.sum(0), 0.3), bad=bad)
    for r in L.UP_R:
        dy = torch.randn(2, 13 * r, 11 * r, 8, generator=torch.Generator().manual_seed(r))
        x = torch.zeros(2, 13, 11, 8, requires_grad=True)
        L.upsample_nearest_ref(x, r).backward(dy)
        _under('upsample_nearest_bwd r %d' % r, L.emulate_upsample_nearest_bwd(dy, r), L.upsample_nearest_bwd_ref(dy, r), x.grad, bad=bad)
    for hidden in L.CA_HIDDEN:
        inp = L.ca_mlp_bwd_inputs(3, hidden)
        ref, t32 = L.ca_mlp_bwd_eval(inp, F64), L.ca_mlp_bwd_eval(inp, F32)
        emu = L.emulate_ca_wgrad(t32['dl'], t32['dh'], inp['hid'], inp['avg'])
        for k, v in emu.items():
            _under('ca_mlp_wgrad %s hidden %d' % (k, hidden), v, ref[k], t32[k], bad=bad)
    assert not bad, bad


def f32_mul(t, s):
    return t * torch.tensor(s, dtype=F32)


def test_kernel_formulation_of_the_quadrant_attention_is_the_same_function():
    """nl_eval_online32 (the online soft-max with P recomputed, in fp32, every sum left to right) against fp64, next to stock fp32,
    for every case the GPU test runs: a correct fp32 evaluation of the kernels' own formulation is under the bar that stock torch
    sets, so the kernels can meet it."""
    bad = []
    for family in L.NL_FAMILIES:
        for n, h, w in L.NL_SHAPES:
            inp = L.nl_inputs(family, n, h, w)
            ref, t32, on = L.nl_eval(inp, F64), L.nl_eval(inp, F32), L.nl_eval_online32(inp)
            scales = L.nl_scales(family, inp)
            for k in L.NL_OUT:
                sc = scales.get(k)
                e, te = L.scaled_err(on[k], ref[k], sc), L.scaled_err(t32[k], ref[k], sc)
                print('%-10s %dx%dx%-4d %-7s online %.3e  torch-fp32 %.3e  bound %.3e' % (family, n, h, w, k, e, te, bound(te)))
                if not e <= bound(te):
                    bad.append((family, (n, h, w), k, e, te))
    assert not bad, bad


# --------------------------------------------------------------------------------------------- #
# the conditions of the input families
# --------------------------------------------------------------------------------------------- #


def test_scalar_sums_do_not_cancel():
    for items, (rows, ch) in L.ITEM_SHAPES.items():
        g, z = L.clean_rows(rows, ch)
        assert float(L.cancellation(L.prelu_slope_terms(g, z))) >= L.SUM_MIN_RATIO, items
        _, b, gg = L.gamma_inputs(4 * items)
        assert float(L.cancellation(gg.double() * b.double())) >= L.SUM_MIN_RATIO, items
    g, z = L.clean_rows(*L.ITEM_SHAPES[131076])
    print('ratios at 524,304 elements: slope %.3f gamma %.3f' % (float(L.cancellation(L.prelu_slope_terms(g, z))),
                                                              float(L.cancellation(L.gamma_inputs(524304)[2].double() * L.gamma_inputs(524304)[1].double()))))
    for nparts in L.REDUCE_NPARTS:
        assert float(L.cancellation(L.clean_rows(1, nparts, 9)[0])) >= L.SUM_MIN_RATIO
    for hidden in L.CA_HIDDEN:
        for n in L.CA_N:
            inp = L.ca_mlp_bwd_inputs(n, hidden)
            for k, terms in L.ca_wgrad_terms(inp).items():
                assert float(L.cancellation(terms, 0).min()) >= L.SUM_MIN_RATIO, (k, n, hidden)
            if n * hidden > 1:
                assert float(inp['hid'][0, 0]) == 0.0
            assert float(inp['hid'][n - 1, hidden - 1]) > 0 and float(inp['hid'].min()) >= 0


def test_mlp_families_clip_and_zero_the_units_they_are_named_for():
    for hidden in L.CA_HIDDEN:
        for nseg in L.CA_NSEG:
            for use_b1, use_b2 in L.CA_BIAS_COMBOS:
                pre = L.ca_mlp_fwd_eval(L.ca_mlp_inputs('mixed', 3, hidden, nseg), F64, use_b1, use_b2)['pre']
                assert bool((pre[:, 0::2] > 0.01).all()) and bool((pre[:, 1::2] < -0.01).all())          # active and clipped units
                for dtype in (F64, F32):
                    z = L.ca_mlp_fwd_eval(L.ca_mlp_inputs('zero_unit', 3, hidden, nseg), dtype, use_b1, use_b2)
                    assert bool((z['pre'][:, hidden - 1] == 0).all()) and bool((z['hid'][:, hidden - 1] == 0).all())
            r = L.ca_mlp_fwd_eval(L.ca_mlp_inputs('nan', 3, hidden, nseg), F64)
            assert bool(torch.isnan(r['s'][1]).all()) and bool(torch.isfinite(r['s'][[0, 2]]).all())
            assert bool(torch.isnan(r['hid'][1]).all())
    inp = L.ca_mlp_bwd_inputs(3, 4)
    ref = L.ca_mlp_bwd_eval(inp, F64)
    assert float(ref['dh'][0, 0]) == 0.0 and float(ref['dh'][2, 3]) > 0                                       # dh = 0 at the exact-zero unit


def test_special_value_rows_hold_every_special_at_both_ends():
    g, z = L.special_rows(*L.ITEM_SHAPES[257])
    flat = z.reshape(-1)
    for end in (flat[:8], flat[-8:]):
        assert int(torch.isnan(end).sum()) == 1 and int(torch.isinf(end).sum()) == 2 and int((end == 0).sum()) == 2
        assert int(torch.signbit(end[end == 0]).sum()) == 1 and int(((end != 0) & (end.abs() < 1e-38)).sum()) == 3
    assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize('shape', L.NL_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_quadrant_attention_families(shape):
    n, h, w = shape
    lg = {f: L.nl_logits(L.nl_inputs(f, n, h, w)) for f in L.NL_FAMILIES}
    rows = torch.cat([torch.softmax(s, -1).amax(-1).reshape(-1) for s in lg['sharp']])
    assert not bool(torch.isnan(rows).any()) and float((rows > 0.99).double().mean()) >= 0.25, float((rows > 0.99).double().mean())
    big = max(float(s.abs().max()) for s in lg['sharp'])
    print('%s sharp: max |logit| %.1f, share of rows above 0.99: %.2f' % (shape, big, float((rows > 0.99).double().mean())))
    if h * w >= 100:
        assert big > 60 and max(float(s.abs().max()) for s in lg['unit']) < 25
    for s in lg['ascending']:
        assert s.shape[2] == 1 or bool((s[..., 1:] - s[..., :-1] > 1e-3).all())          # far above an fp32 rounding of a logit of tens
    for s in lg['descending']:
        assert s.shape[2] == 1 or bool((s[..., :-1] - s[..., 1:] > 1e-3).all())
    for s in lg['equal']:
        assert float((s - s[..., :1]).abs().max()) == 0.0
    ref = L.nl_eval(L.nl_inputs('equal', n, h, w), F64)
    sc = L.nl_scales('equal', L.nl_inputs('equal', n, h, w))['dtheta']
    assert float(ref['dtheta'].abs().max()) <= 1e-13 * max(sc, 1e-30) or sc == 0.0


# --------------------------------------------------------------------------------------------- #
# the case tables hold the edges they are named for
# --------------------------------------------------------------------------------------------- #


def test_case_tables_contain_their_edges():
    assert len(L.CA_SHAPES) == 13 and set(L.CA_HW) == {1, 31, 32, 33, 1537, 2049} and set(L.CA_N) == {1, 3}
    assert L.seg_len(1) == 1 and L.seg_len(31) == 1 and L.seg_len(32) == 1 and L.seg_len(33) == 2 and L.seg_len(1537) == 49 and L.seg_len(2049) == 65
    assert sum(p1 > p0 for p0, p1 in L.seg_bounds(1)) == 1 and sum(p1 > p0 for p0, p1 in L.seg_bounds(31)) == 31
    b33 = L.seg_bounds(33)
    assert b33[16] == (32, 33) and all(p0 == p1 for p0, p1 in b33[17:])                     # a ragged last segment, then empty ones
    # segment length 49: lane 0 alone has p + 48 < p1 at p = p0; 2049 ends in a segment of 34 pixels
    assert [r for r in range(16) if r + 48 < 49] == [0] and L.seg_bounds(2049)[31] == (2015, 2049)
    n, hw = L.CA_BIG
    assert n * hw * 16 > L.STREAM_CAP == 4096 * 256 and n * hw * 16 - L.STREAM_CAP == 96 and L.seg_len(hw) == 1025
    assert max(n * hw for n, hw in L.CA_SHAPES[:-1]) * 16 < L.STREAM_CAP
    assert set(L.CA_HIDDEN) == {1, 4, 5, 16} and set(L.CA_NSEG) == {1, 3, 4, 5, 32, 64} and max(L.CA_NSEG) == L.CA_MAXSEG
    assert len(L.CA_BIAS_COMBOS) == 4 and len(set(L.CA_BIAS_COMBOS)) == 4
    assert [p // 4 for p in L.BCAST_PER_IMAGE] == [1, 255, 256, 257] and set(L.BCAST_N) == {1, 2, 5}
    assert L.BATCH_SUM_BIG == (2, 4194316) and L.BATCH_SUM_BIG[1] // 4 > L.STREAM_CAP
    assert L.ADD_BCAST_BIG[0] * L.ADD_BCAST_BIG[1] // 4 > L.STREAM_CAP >= L.ADD_BCAST_BIG[1] // 4
    assert {k: r * c // 4 for k, (r, c) in L.ITEM_SHAPES.items()} == {k: k for k in (1, 255, 256, 257, 131076)}
    assert L.ITEM_SHAPES[131076] == (43692, 12) and 131076 - L.PARTS_TRIP == 4
    assert all(c % 4 == 0 for _, c in L.ITEM_SHAPES.values())
    assert L.LAYOUTS['dense'] == (0, 0) and L.LAYOUTS['slice'][0] > 0 and L.LAYOUTS['slice'][1] % 4 == 0 and 0 < L.LAYOUTS['slice'][1] < L.LAYOUTS['slice'][0]
    assert L.PRELU_SLOPES == (0.25, 0.0, -0.3, 1.0) and L.LRELU_SLOPES == (0.2, 0.0, 1.0)
    assert L.REDUCE_NPARTS == (1, 255, 256, 257, 1536) and set(L.SMALL_ITEMS) == {255, 256, 257}
    assert set(L.UP_R) == {2, 3} and set(L.UP_C) == {4, 8, 64} and set(L.UP_NHW) == {(1, 1, 1), (3, 5, 7), (2, 13, 11)}
    assert set(L.NL_SHAPES) == {(1, 2, 2), (2, 3, 2), (1, 2, 515), (3, 17, 31), (1, 33, 32)}
    assert set(L.NL_FAMILIES) == {'unit', 'sharp', 'ascending', 'descending', 'equal'}
    n, h, w = L.NL_INDEPENDENCE
    assert (n, h, w) in L.NL_SHAPES and h * w == 527 and (h * w) % 256 != 0 and (n * h * w) % 256 != 0 and 2 * h * w // 256 == n * h * w // 256 - 2
    assert [(r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in L.nl_quadrants(2, 2)] == [1, 1, 1, 1]
    assert [(r1 - r0, c1 - c0) for r0, r1, c0, c1 in L.nl_quadrants(3, 2)] == [(1, 1), (1, 1), (2, 1), (2, 1)]
    assert [(r1 - r0, c1 - c0) for r0, r1, c0, c1 in L.nl_quadrants(2, 515)] == [(1, 257), (1, 258), (1, 257), (1, 258)]


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


FAKE = {k: 0x100000 + 0x10000 * i for i, k in enumerate('abcdefghijkl')}         # aligned, never dereferenced
FAKE.update(ws=0x4000000, ws_bytes=1 << 16)

REFUSED_ENTRIES = {
    'ca': {'ca_pool_sum', 'ca_mlp_fwd', 'ca_mlp_fwd_bias', 'ca_scale_res', 'ca_bwd_partial', 'ca_mlp_bwd', 'ca_mlp_bwd_bias', 'ca_bwd_du',
           'add_bcast_scaled', 'batch_sum_scaled'},
    'residual': {'prelu_fwd', 'prelu_bwd', 'prelu_slope_reduce', 'scaled_res_fwd', 'scaled_res_bwd', 'lrelu_bwd_strided',
                 'upsample_nearest_fwd', 'upsample_nearest_bwd', 'gamma_res_fwd', 'gamma_res_bwd'},
    'nl_quad': {'nl_quad_fwd', 'nl_quad_bwd'},
}


@pytest.mark.parametrize('family', sorted(REFUSED_ENTRIES))
def test_every_entry_point_refuses_bad_arguments(lib, family):
    calls = {'ca': L.ca_refusals, 'residual': L.residual_refusals, 'nl_quad': L.nl_quad_refusals}[family](lib, FAKE)
    assert {label.split(':')[0] for label, _ in calls} == REFUSED_ENTRIES[family]
    assert len({label for label, _ in calls}) == len(calls)
    bad = []
    for label, call in calls:
        lib.srhip_cbam_pool_hw(None, None, None, 0, 1, 1, 4, None)               # leaves a message of another entry behind
        rc = call()
        msg = lib.srhip_last_error()
        if rc != L.ERR_ARG or not msg or label.split(':')[0].encode() not in msg:
            bad.append((label, rc, msg))
    assert not bad, bad
