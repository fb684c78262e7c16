"""csrc/ca.hip -- the channel attention of DSSR / DRCAN and the DSSR upsampler fold -- one entry point at a time through the C ABI
(ctypes), each on inputs of its own, at the sizes where the launch geometry changes: fewer pixels than segments (empty segments hold
+0.0), one pixel, a ragged last segment, a segment of exactly 49 pixels (one lane in the 4-deep loop), one grid-stride trip past the
4096-block cap, every count of partial segments that leaves lanes of the segment walk empty, hidden widths 1 to 16, every NULL /
non-NULL combination of the biases and of their gradients.

Protocol of tests/test_cbam_gpu.py: every tensor lies in a pointwise_ref.Guarded allocation (64-element sentinel bands, outputs NaN),
partial arrays and the workspace are exactly as large as the library says, the bands and the inputs are intact after every call, and
every kernel runs twice on fresh buffers with equal bits.  The element-wise passes and the fixed-order sums are compared BIT FOR BIT
with tests/leaf_kernels_ref.py's fp32 evaluation of the documented order; the MLP outputs with err / bound of tests/reduction_ref.py
(8 x the error of fp32 torch on the CPU against fp64, never the device's own output).  Every figure is printed before its assert."""
import pytest
import torch

from tests import leaf_kernels_ref as L
from tests.test_reductions_gpu import _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32
C = L.CA_C
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _inputs(n, hw):
    return _once((n, hw), lambda: L.ca_inputs(n, hw))


def _ids(cases):
    return ['x'.join(str(v) for v in c) for c in cases]


# --------------------------------------------------------------------------------------------- #
# the two segment sums
# --------------------------------------------------------------------------------------------- #


def _run_partials(t, n, hw):
    lib, b = _lib(), L.Buffers(DEV)
    nseg = lib.srhip_ca_segments()
    pu, pg = b.put('u', t['u']), b.put('g', t['g'])
    _ok(lib.srhip_ca_pool_sum(pu, b.out('psum', nseg * n * C), n, hw, C, _stream()), 'ca_pool_sum')
    _ok(lib.srhip_ca_bwd_partial(pg, pu, b.out('part', nseg * n * C), n, hw, C, _stream()), 'ca_bwd_partial')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('n,hw', L.CA_SHAPES, ids=_ids(L.CA_SHAPES))
def test_segment_sums_are_the_documented_order_bit_for_bit(n, hw):
    """srhip_ca_pool_sum, srhip_ca_bwd_partial: lane r of 16 walks p0 + r in steps of 16, the 16 lanes summed in order.
    On the MI355X every case is bit-equal to the emulation; against fp64 the worst err / bar is 0.12 (2 x 32771: err 2.3e-7, fp32 torch
    1.6e-7, bar 1.9e-6)."""
    assert _lib().srhip_ca_segments() == L.CA_SEG
    t = _inputs(n, hw)
    tab = L.table('ca partials %dx%d' % (n, hw))
    first, second = _run_partials(t, n, hw), _run_partials(t, n, hw)
    tab.guards(first, second)
    empty = [s for s, (p0, p1) in enumerate(L.seg_bounds(hw)) if p1 == p0]
    for name, a, bb in (('psum', t['u'], None), ('part', t['g'], t['u'])):
        got = first.get(name).view(n, L.CA_SEG, C)
        tab.bits(name, got, L.emulate_ca_partial(a, bb))
        tab.true('%s: %d empty segments hold +0.0' % (name, len(empty)), L.exact(got[:, empty], torch.zeros(n, len(empty), C)))
        v = a if bb is None else a * bb
        tab.check(name + ' vs fp64', got, L.ca_partial_ref(a, bb), torch.stack([v[:, p0:p1].sum(1) for p0, p1 in L.seg_bounds(hw)], 1))
        tab.rerun(name, first.get(name), second.get(name))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# out = s * u + x, du = s * g + dmean
# --------------------------------------------------------------------------------------------- #


def _run_streams(t, n, hw):
    lib, b = _lib(), L.Buffers(DEV)
    ps = b.put('s', t['s'])
    _ok(lib.srhip_ca_scale_res(b.put('u', t['u']), ps, b.put('x', t['x']), b.out('out', n, hw, C), n, hw, C, _stream()), 'ca_scale_res')
    _ok(lib.srhip_ca_bwd_du(b.put('g', t['g']), ps, b.put('dmean', t['dmean']), b.out('du', n, hw, C), n, hw, C, _stream()), 'ca_bwd_du')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('n,hw', L.CA_SHAPES, ids=_ids(L.CA_SHAPES))
def test_scale_res_and_bwd_du_bit_for_bit_with_an_arbitrary_gate(n, hw):
    """srhip_ca_scale_res, srhip_ca_bwd_du on a gate no kernel produced; 2 x 32771 takes the second grid-stride trip."""
    t = _inputs(n, hw)
    tab = L.table('ca streams %dx%d' % (n, hw))
    first, second = _run_streams(t, n, hw), _run_streams(t, n, hw)
    tab.guards(first, second)
    tab.bits('out', first.get('out'), L.ca_scale_res_ref32(t['u'], t['s'], t['x']))
    tab.bits('du', first.get('du'), L.ca_bwd_du_ref32(t['g'], t['s'], t['dmean']))
    for k in ('out', 'du'):
        tab.rerun(k, first.get(k), second.get(k))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# the MLP forward on synthetic partial arrays
# --------------------------------------------------------------------------------------------- #

N_MLP = 3


def _run_mlp_fwd(inp, hidden, nseg, use_b1, use_b2, plain=False):
    lib, b = _lib(), L.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('psum', 'fc1', 'b1', 'fc2', 'b2')}
    outs = (b.out('avg', N_MLP, C), b.out('hid', N_MLP, hidden), b.out('s', N_MLP, C))
    if plain:
        _ok(lib.srhip_ca_mlp_fwd(p['psum'], nseg, p['fc1'], p['fc2'], *outs, N_MLP, inp['hw'], C, hidden, _stream()), 'ca_mlp_fwd')
    else:
        _ok(lib.srhip_ca_mlp_fwd_bias(p['psum'], nseg, p['fc1'], p['b1'] if use_b1 else None, p['fc2'], p['b2'] if use_b2 else None, *outs,
                                      N_MLP, inp['hw'], C, hidden, _stream()), 'ca_mlp_fwd_bias')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('nseg', L.CA_NSEG)
@pytest.mark.parametrize('hidden', L.CA_HIDDEN)
def test_mlp_forward_every_segment_count_hidden_width_and_bias_combination(hidden, nseg):
    """srhip_ca_mlp_fwd / _fwd_bias: avg, hid, s of three images against fp64.  Families: units both clipped and active; a unit whose
    pre-activation is exactly 0; a NaN in one partial of image 1, which fills that image's hid and s and reaches no other image.
    Worst err / bar on the MI355X: 0.14 (hidden 16, nseg 4, s: err 2.7e-7, fp32 torch 2.1e-7, bar 1.9e-6)."""
    tab = L.table('ca mlp fwd hidden %d nseg %d' % (hidden, nseg))
    for family in L.CA_MLP_FAMILIES:
        inp = L.ca_mlp_inputs(family, N_MLP, hidden, nseg)
        keep = [0, 2] if family == 'nan' else [0, 1, 2]
        for use_b1, use_b2 in L.CA_BIAS_COMBOS:
            ref, t32 = (L.ca_mlp_fwd_eval(inp, d, use_b1, use_b2) for d in (F64, F32))
            first, second = (_run_mlp_fwd(inp, hidden, nseg, use_b1, use_b2) for _ in range(2))
            tab.guards(first, second)
            tag = '%s b1 %d b2 %d ' % (family, use_b1, use_b2)
            for k in ('avg', 'hid', 's'):
                tab.check(tag + k, first.get(k)[keep], ref[k][keep], t32[k][keep])
                tab.rerun(tag + k, first.get(k), second.get(k))
            if family == 'zero_unit':
                tab.true(tag + 'hid of the zero unit == 0', bool((first.get('hid')[:, hidden - 1] == 0).all()))
            if family == 'nan':
                tab.true(tag + 'NaN fills hid and s of image 1 only', bool(torch.isnan(first.get('s')[1]).all()) and
                         bool(torch.isnan(first.get('hid')[1]).all()) and int(torch.isnan(first.get('avg')).sum()) == 1)
            if not (use_b1 or use_b2):
                plain = _run_mlp_fwd(inp, hidden, nseg, False, False, plain=True)
                tab.guards(plain)
                for k in ('avg', 'hid', 's'):
                    tab.rerun(tag + k + ' == bias-free entry', first.get(k), plain.get(k))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# the MLP backward and its weight-gradient pass
# --------------------------------------------------------------------------------------------- #

BWD_OUT = ('dmean', 'dfc1', 'dfc2')


def _run_mlp_bwd(inp, n, hidden, want_db1, want_db2, plain=False):
    lib, b = _lib(), L.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('part', 'avg', 'hid', 's', 'fc1', 'fc2')}
    need = lib.srhip_ca_mlp_bwd_workspace(n, hidden)
    assert need == 4 * n * (C + hidden)
    dmean, dfc1, dfc2 = b.out('dmean', n, C), b.out('dfc1', hidden, C), b.out('dfc2', C, hidden)
    db1, db2, ws = b.out('db1', hidden), b.out('db2', C), b.out('ws', need // 4)
    head = (p['part'], p['avg'], p['hid'], p['s'], p['fc1'], p['fc2'], dmean)
    tail = (ws, need, n, inp['hw'], C, hidden, _stream())
    if plain:
        _ok(lib.srhip_ca_mlp_bwd(*head, dfc1, dfc2, *tail), 'ca_mlp_bwd')
    else:
        _ok(lib.srhip_ca_mlp_bwd_bias(*head, dfc1, db1 if want_db1 else None, dfc2, db2 if want_db2 else None, *tail), 'ca_mlp_bwd_bias')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('n', L.CA_N)
@pytest.mark.parametrize('hidden', L.CA_HIDDEN)
def test_mlp_backward_every_bias_gradient_combination(hidden, n):
    """srhip_ca_mlp_bwd / _bwd_bias on inputs of their own: dmean, dl, dh (read back from the workspace), dfc1, dfc2, db1, db2 against
    fp64; the weight and bias gradients bit for bit with the images-in-order sum of the dl / dh the first kernel left; a bias
    gradient that is not asked for stays untouched; dh = 0 at the exact-zero hidden unit.
    Worst err / bar on the MI355X: 0.10 (hidden 16, n 3, dl: err 1.9e-7, fp32 torch 1.5e-7, bar 1.9e-6)."""
    inp = L.ca_mlp_bwd_inputs(n, hidden)
    ref, t32 = L.ca_mlp_bwd_eval(inp, F64), L.ca_mlp_bwd_eval(inp, F32)
    tab = L.table('ca mlp bwd hidden %d n %d' % (hidden, n))
    base = None
    for want_db1, want_db2 in L.CA_BIAS_COMBOS:
        first, second = (_run_mlp_bwd(inp, n, hidden, want_db1, want_db2) for _ in range(2))
        tab.guards(first, second)
        tag = 'db1 %d db2 %d ' % (want_db1, want_db2)
        ws = first.get('ws')
        got = {k: first.get(k) for k in BWD_OUT}
        got.update(dl=ws[:n * C].view(n, C), dh=ws[n * C:].view(n, hidden))
        wanted = [k for k, w in (('db1', want_db1), ('db2', want_db2)) if w]
        got.update({k: first.get(k) for k in wanted})
        for k, v in got.items():
            tab.check(tag + k, v, ref[k], t32[k])
        emu = L.emulate_ca_wgrad(got['dl'], got['dh'], inp['hid'], inp['avg'])
        for k in ['dfc1', 'dfc2'] + wanted:
            tab.bits(tag + k + ' images in order', got[k], emu[k])
        for k, w in (('db1', want_db1), ('db2', want_db2)):
            if not w:
                tab.true(tag + k + ' not asked for: untouched', first.all[k].untouched())
        if n * hidden > 1:
            tab.true(tag + 'dh = 0 at the zero unit', float(got['dh'][0, 0]) == 0.0)
        for k in BWD_OUT + ('ws',) + tuple(wanted):
            tab.rerun(tag + k, first.get(k), second.get(k))
        if base is None:
            base = first
            plain = _run_mlp_bwd(inp, n, hidden, False, False, plain=True)
            tab.guards(plain)
            tab.true('bias-free entry leaves db1, db2 untouched', plain.all['db1'].untouched() and plain.all['db2'].untouched())
            for k in BWD_OUT + ('ws',):
                tab.rerun(k + ' == bias-free entry', first.get(k), plain.get(k))
        for k in BWD_OUT + ('ws',):
            tab.rerun(tag + k + ' == without bias gradients', first.get(k), base.get(k))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# the whole block, chained; batch independence; NaN containment
# --------------------------------------------------------------------------------------------- #

CHAIN_HIDDEN = 5
CHAIN_OUT = ('psum', 'avg', 'hid', 's', 'out', 'part', 'dmean', 'dfc1', 'db1', 'dfc2', 'db2', 'du')


def _chain_params(hidden):
    gen = torch.Generator().manual_seed(808 + hidden)
    return dict(fc1=0.3 * torch.randn(hidden, C, generator=gen), b1=0.2 * torch.randn(hidden, generator=gen),
                fc2=0.3 * torch.randn(C, hidden, generator=gen), b2=0.5 * torch.randn(C, generator=gen))


def _run_chain(u, x, g, w, hidden):
    """pool_sum -> mlp_fwd_bias -> scale_res, then bwd_partial -> mlp_bwd_bias -> bwd_du, every buffer guarded."""
    lib, b = _lib(), L.Buffers(DEV)
    n, hw = u.shape[:2]
    nseg, st = lib.srhip_ca_segments(), _stream()
    pu, px, pg = b.put('u', u), b.put('x', x), b.put('g', g)
    p = {k: b.put(k, v) for k, v in w.items()}
    _ok(lib.srhip_ca_pool_sum(pu, b.out('psum', nseg * n * C), n, hw, C, st), 'ca_pool_sum')
    _ok(lib.srhip_ca_mlp_fwd_bias(b.ptr('psum'), nseg, p['fc1'], p['b1'], p['fc2'], p['b2'], b.out('avg', n, C), b.out('hid', n, hidden),
                                  b.out('s', n, C), n, hw, C, hidden, st), 'ca_mlp_fwd_bias')
    _ok(lib.srhip_ca_scale_res(pu, b.ptr('s'), px, b.out('out', n, hw, C), n, hw, C, st), 'ca_scale_res')
    _ok(lib.srhip_ca_bwd_partial(pg, pu, b.out('part', nseg * n * C), n, hw, C, st), 'ca_bwd_partial')
    need = lib.srhip_ca_mlp_bwd_workspace(n, hidden)
    _ok(lib.srhip_ca_mlp_bwd_bias(b.ptr('part'), b.ptr('avg'), b.ptr('hid'), b.ptr('s'), p['fc1'], p['fc2'], b.out('dmean', n, C),
                                  b.out('dfc1', hidden, C), b.out('db1', hidden), b.out('dfc2', C, hidden), b.out('db2', C),
                                  b.out('ws', need // 4), need, n, hw, C, hidden, st), 'ca_mlp_bwd_bias')
    _ok(lib.srhip_ca_bwd_du(pg, b.ptr('s'), b.ptr('dmean'), b.out('du', n, hw, C), n, hw, C, st), 'ca_bwd_du')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('hw', L.CA_INDEPENDENCE_HW)
def test_chained_block_against_fp64_each_image_alone_and_a_nan_in_one_image(hw):
    """The six kernels chained on a batch of 3 against the closed form in fp64 (the expression of tests/test_drcan_gpu.ca_ref64); every
    per-image result of image b equals, bit for bit, the same image run alone; a NaN in image 1's u turns that image's s and out
    into NaN and changes no bit of images 0 and 2.
    Worst err / bar on the MI355X: 0.08 (db2 at hw 33: err 1.5e-7, fp32 torch 1.0e-7, bar 1.9e-6)."""
    n = 3
    t, w = _inputs(n, hw), _chain_params(CHAIN_HIDDEN)
    args = (t['u'], t['x'], w['fc1'], w['b1'], w['fc2'], w['b2'], t['g'])
    ref, t32 = L.ca_chain_ref(*args, dtype=F64), L.ca_chain_ref(*args, dtype=F32)
    tab = L.table('ca chain 3x%d' % hw)
    first, second = (_run_chain(t['u'], t['x'], t['g'], w, CHAIN_HIDDEN) for _ in range(2))
    tab.guards(first, second)
    for k in ('s', 'out', 'du', 'dfc1', 'db1', 'dfc2', 'db2'):
        tab.check(k, first.get(k), ref[k], t32[k])
    for k in CHAIN_OUT:
        tab.rerun(k, first.get(k), second.get(k))
    per_image = ('psum', 'avg', 'hid', 's', 'out', 'part', 'dmean', 'du')
    for img in range(n):
        alone = _run_chain(t['u'][img:img + 1], t['x'][img:img + 1], t['g'][img:img + 1], w, CHAIN_HIDDEN)
        tab.guards(alone)
        for k in per_image:
            whole = first.get(k)
            whole = whole.view(n, -1) if k in ('psum', 'part') else whole
            tab.rerun('image %d alone: %s' % (img, k), whole[img].reshape(-1), alone.get(k).reshape(-1))
    u = t['u'].clone()
    u[1, hw // 2, 3] = L.NAN
    bad = _run_chain(u, t['x'], t['g'], w, CHAIN_HIDDEN)
    tab.guards(bad)
    tab.true('NaN: s and out of image 1 are NaN', bool(torch.isnan(bad.get('s')[1]).all()) and bool(torch.isnan(bad.get('out')[1]).all()))
    for k in ('avg', 'hid', 's', 'out', 'dmean', 'du'):
        tab.rerun('NaN: images 0 and 2 of ' + k, bad.get(k)[[0, 2]], first.get(k)[[0, 2]])
    tab.done()


# --------------------------------------------------------------------------------------------- #
# the upsampler fold
# --------------------------------------------------------------------------------------------- #

FOLD_CASES = [(n, per) for per in L.BCAST_PER_IMAGE for n in L.BCAST_N]
SCALE = 0.3


def _fold_inputs(n, per):
    gen = torch.Generator().manual_seed(n + 10 * per)
    return torch.randn(n, per, generator=gen), torch.randn(per, generator=gen), torch.randn(n, per, generator=gen) + 0.5


def _run_add_bcast(a, bc, n, per):
    b = L.Buffers(DEV)
    _ok(_lib().srhip_add_bcast_scaled(b.put('a', a), b.put('b', bc), SCALE, b.out('out', n, per), n, per, _stream()), 'add_bcast_scaled')
    torch.cuda.synchronize()
    return b


def _run_batch_sum(g, n, per):
    b = L.Buffers(DEV)
    _ok(_lib().srhip_batch_sum_scaled(b.put('g', g), SCALE, b.out('out', per), n, per, _stream()), 'batch_sum_scaled')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('n,per', FOLD_CASES + [L.ADD_BCAST_BIG], ids=_ids(FOLD_CASES + [L.ADD_BCAST_BIG]))
def test_add_bcast_scaled_bit_for_bit(n, per):
    a, bc, _ = _fold_inputs(n, per)
    tab = L.table('add_bcast_scaled %dx%d' % (n, per))
    first, second = _run_add_bcast(a, bc, n, per), _run_add_bcast(a, bc, n, per)
    tab.guards(first, second)
    tab.bits('out', first.get('out'), L.add_bcast_scaled_ref32(a, bc, SCALE))
    tab.rerun('out', first.get('out'), second.get('out'))
    tab.done()


@pytest.mark.parametrize('n,per', FOLD_CASES + [L.BATCH_SUM_BIG], ids=_ids(FOLD_CASES + [L.BATCH_SUM_BIG]))
def test_batch_sum_scaled_images_in_order_bit_for_bit(n, per):
    _, _, g = _fold_inputs(n, per)
    tab = L.table('batch_sum_scaled %dx%d' % (n, per))
    first, second = _run_batch_sum(g, n, per), _run_batch_sum(g, n, per)
    tab.guards(first, second)
    tab.bits('out', first.get('out'), L.emulate_batch_sum_scaled(g, SCALE))
    tab.check('out vs fp64', first.get('out'), L.batch_sum_ref(g, SCALE), g.sum(0) * L.f32(SCALE))
    tab.rerun('out', first.get('out'), second.get('out'))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------------------------- #


def test_refusals_leave_every_buffer_untouched():
    L.run_refusals(_lib(), DEV, L.ca_refusals)
