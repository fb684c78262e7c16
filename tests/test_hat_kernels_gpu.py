"""csrc/hat.hip -- LayerNorm, GELU, window attention (SA, shifted SA, OCA), channel attention and HAB's combine -- one entry point at a
time through the C ABI (ctypes) against the float64 references of tests/attn_kernels_ref.py, at the sizes where the launch geometry
changes: more than 64 windows (the backward's blocks walk windows g, g + 64, ... and 64 partial tables are reduced), more than 2048
LayerNorm tokens (its 512 blocks stride), more than 4,194,304 element-wise floats (the 4096-block grids stride), pixel counts around
the 8 pixel lanes of the channel sums, and every optional pointer NULL once.

Protocol of tests/test_cbam_gpu.py, as in tests/test_global_attn_kernels_gpu.py: every tensor a kernel sees lies between sentinel
bands, outputs and workspaces start as NaN, workspaces are exactly as large as the library asks; afterwards the bands are intact, no
NaN is left in an output, every tensor's err = max|got - ref64| / max|ref64| is under max(8 x err of the fp32 CPU evaluation,
32 * 2^-24) capped by the older tests' bounds (not on the x6 / ascending / descending attention families), and a second call on
fresh guarded buffers gives the same bits: the file uses no atomics.  Where a kernel does one rounding (da = kb g) the fp32 product's
bits are demanded.  Every figure is printed before its test asserts."""
import pytest
import torch

from tests import attn_kernels_ref as A
from tests.test_reductions_gpu import _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32


# --------------------------------------------------------------------------------------------- #
# window attention
# --------------------------------------------------------------------------------------------- #

ATTN_OUT = ('out', 'lse', 'dqkv', 'dtable')


def _attn_run(inp):
    lib, b = _lib(), A.Buffers(DEV)
    kind, ws, shift = inp['kind'], inp['ws'], inp['shift']
    n, h, w, _ = inp['qkv'].shape
    p = {k: b.put(k, inp[k]) for k in ('qkv', 'table', 'dout')}
    _ok(lib.srhip_hat_attn_fwd(p['qkv'], p['table'], b.out('out', n, h, w, 96), b.out('lse', n, h, w, 6), kind, n, h, w, ws, shift, _stream()),
        'hat_attn_fwd')
    torch.cuda.synchronize()
    need = lib.srhip_hat_attn_bwd_workspace(kind, n, h, w, ws)
    _ok(lib.srhip_hat_attn_bwd(p['qkv'], p['table'], b.ptr('out'), p['dout'], b.ptr('lse'), b.out('dqkv', n, h, w, 288),
                               b.out('dtable', A.hat_table_rows(kind, ws), 6), b.workspace('ws', need), need, kind, n, h, w, ws, shift, _stream()),
        'hat_attn_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('case', A.HAT_ATTN_CASES, ids=[c[0].replace(' ', '_').replace(',', '') for c in A.HAT_ATTN_CASES])
def test_window_attention_walks_more_windows_than_blocks(case):
    """srhip_hat_attn_fwd / _bwd: out, lse, dqkv and dtable at 75 windows (all of SA, shifted SA and OCA at window 8 and 9), at 64, 65
    and 128 windows, with logits of tens and with key scores that rise / fall along the forward's key loop.
    Worst err / bar on the MI355X: 0.27 over the nine random cases, 0.17 x6, 0.16 ascending, 0.16 descending."""
    inp = A.hat_attn_inputs(case)
    ref, t32 = A.hat_attn_eval(inp, F64), A.hat_attn_eval(inp, F32)
    table = A.bars(ref, t32, 'hat_attn', case[7] not in A.HAT_ATTN_UNCAPPED)
    tab = A.Table('hat attn ' + case[0])
    first, second = _attn_run(inp), _attn_run(inp)
    tab.buffers(first, ATTN_OUT)
    tab.buffers(second, ATTN_OUT)
    tab.check_all({k: first.get(k) for k in ATTN_OUT}, ref, table)
    tab.rerun(first, second, ATTN_OUT)
    tab.done()


# --------------------------------------------------------------------------------------------- #
# LayerNorm, GELU
# --------------------------------------------------------------------------------------------- #


def _ln_run(inp, tokens, dadd=False, dgamma=True, dbeta=True):
    lib, b = _lib(), A.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('x', 'gamma', 'beta', 'dy', 'dadd')}
    _ok(lib.srhip_hat_ln_fwd(p['x'], p['gamma'], p['beta'], b.out('y', tokens, 96), b.out('mean', tokens), b.out('rstd', tokens), tokens, _stream()),
        'hat_ln_fwd')
    torch.cuda.synchronize()
    b.out('dgamma', 96)
    b.out('dbeta', 96)
    _ok(lib.srhip_hat_ln_bwd(p['dy'], p['x'], p['gamma'], b.ptr('mean'), b.ptr('rstd'), p['dadd'] if dadd else None, b.out('dx', tokens, 96),
                             b.out('part', lib.srhip_hat_ln_parts(tokens), 192), b.ptr('dgamma') if dgamma else None,
                             b.ptr('dbeta') if dbeta else None, tokens, _stream()), 'hat_ln_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('family,tokens', A.LN_CASES, ids=['%s-%d' % c for c in A.LN_CASES])
def test_layer_norm_strides_past_its_block_cap(family, tokens):
    """srhip_hat_ln_fwd / _bwd: y, mean, rstd, dx, dgamma, dbeta with `part` sized by srhip_hat_ln_parts; dadd NULL and given; dgamma
    NULL once and dbeta NULL once (the other outputs keep their bits, the slot not given stays untouched).
    Worst err / bar on the MI355X: random 0.16, constant_token 0.12, mean_1000 0.10."""
    inp = A.ln_inputs(family, tokens)
    tab = A.Table('hat ln %s %d' % (family, tokens))
    outs = ('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta')
    runs = {}
    for dadd in (False, True):
        ref, t32 = A.ln_eval(inp, F64, dadd), A.ln_eval(inp, F32, dadd)
        first, second = _ln_run(inp, tokens, dadd), _ln_run(inp, tokens, dadd)
        tab.buffers(first, outs + ('part',))
        tab.buffers(second, outs)
        tab.check_all({k: first.get(k) for k in outs}, ref, A.bars(ref, t32, 'hat_ln'))
        tab.rerun(first, second, outs)
        runs[dadd] = first
    for skip in ('dgamma', 'dbeta'):
        b = _ln_run(inp, tokens, True, dgamma=skip != 'dgamma', dbeta=skip != 'dbeta')
        tab.buffers(b, [k for k in outs if k != skip])
        tab.require(b.all[skip].untouched(), '%s written though NULL was passed' % skip)
        for k in outs:
            if k != skip:
                tab.same_bits('no %s: %s' % (skip, k), b.get(k), runs[True].get(k))
    tab.done()


@pytest.mark.parametrize('count', A.GELU_COUNTS)
def test_gelu_strides_past_its_grid_cap_and_passes_a_nan(count):
    """srhip_hat_gelu_fwd / _bwd on x in [-12, 12] with 0.0, -0.0 and a NaN in the last float4 (at 4,194,308: the one float4 of the
    second grid sweep): the NaN comes back as NaN in y and dx and nowhere else.  Worst err / bar on the MI355X: 0.08."""
    lib = _lib()
    inp = A.gelu_inputs(count)
    ref, t32 = A.gelu_eval(inp, F64), A.gelu_eval(inp, F32)
    nan = torch.isnan(inp['x'])
    tab = A.Table('hat gelu %d' % count)
    runs = []
    for _ in range(2):
        b = A.Buffers(DEV)
        p = {k: b.put(k, inp[k]) for k in ('x', 'dy')}
        _ok(lib.srhip_hat_gelu_fwd(p['x'], b.out('y', count), count, _stream()), 'hat_gelu_fwd')
        _ok(lib.srhip_hat_gelu_bwd(p['dy'], p['x'], b.out('dx', count), count, _stream()), 'hat_gelu_bwd')
        torch.cuda.synchronize()
        tab.require(not b.broken_bands(), 'sentinel band overwritten: %s' % b.broken_bands())
        runs.append(b)
    got = {k: runs[0].get(k) for k in ('y', 'dx')}
    for k in got:
        tab.require(torch.equal(torch.isnan(got[k]), nan), 'NaN set of %s differs from the input\'s' % k)
        tab.require(torch.equal(torch.isnan(t32[k]), nan), 'NaN set of the fp32 evaluation of %s' % k)
    keep = ~nan
    table = A.bars({k: v[keep] for k, v in ref.items()}, {k: v[keep] for k, v in t32.items()}, 'hat_gelu')
    tab.check_all({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in ref.items()}, table)
    tab.rerun(runs[0], runs[1], ('y', 'dx'))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# channel attention and combine
# --------------------------------------------------------------------------------------------- #

PARAM_GRADS = ('dw1', 'db1', 'dw2', 'db2')


def _ca_run(inp, n, hw, c, hid, bias=True, kb=True, with_u=True, du=True, skip=None):
    """ca_fwd -> combine_fwd -> combine_bwd on the forward's own s and mz.  with_u False: the MLP form (no channel attention at all);
    du False: combine_bwd writes da only; skip: the parameter gradient passed as NULL."""
    lib, b = _lib(), A.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('x', 'a', 'u', 'g', 'w1', 'b1', 'w2', 'b2', 'kb')}
    kbp = p['kb'] if kb else None
    if with_u:
        _ok(lib.srhip_hat_ca_fwd(p['u'], p['w1'], p['b1'] if bias else None, p['w2'], p['b2'] if bias else None, b.out('s', n, c),
                                 b.out('mz', n, c + hid), n, hw, c, hid, _stream()), 'hat_ca_fwd')
        torch.cuda.synchronize()
    _ok(lib.srhip_hat_combine_fwd(p['x'], p['a'], kbp, p['u'] if with_u else None, b.ptr('s') if with_u else None, b.out('out', n, hw, c), A.CS,
                                  n, hw, c, _stream()), 'hat_combine_fwd')
    torch.cuda.synchronize()
    b.out('da', n, hw, c)
    if not (with_u and du):
        _ok(lib.srhip_hat_combine_bwd(p['g'], kbp, None, None, None, None, None, b.ptr('da'), None, None, None, None, None, None, 0, A.CS,
                                      n, hw, c, hid, _stream()), 'hat_combine_bwd')
    else:
        need = lib.srhip_hat_combine_bwd_workspace(n, c, hid)
        b.out('dw1', hid, c), b.out('db1', hid), b.out('dw2', c, hid), b.out('db2', c)
        gp = {k: (None if k == skip else b.ptr(k)) for k in PARAM_GRADS}
        _ok(lib.srhip_hat_combine_bwd(p['g'], kbp, p['u'], b.ptr('s'), b.ptr('mz'), p['w1'], p['w2'], b.ptr('da'), b.out('du', n, hw, c), gp['dw1'],
                                      gp['db1'], gp['dw2'], gp['db2'], b.workspace('ws', need), need, A.CS, n, hw, c, hid, _stream()),
            'hat_combine_bwd')
    torch.cuda.synchronize()
    return b


def _da_bits(tab, label, b, inp, kb):
    """da = kb[b] g is one fp32 multiply (kb NULL: g itself)"""
    want = inp['g'] * inp['kb'].view(-1, 1, 1) if kb else inp['g']
    tab.same_bits(label + ' da', b.get('da'), want)


def _ca_case(tab, inp, n, hw, c, hid, light=False):
    label = '%dx%dx%d/%d' % (n, hw, c, hid)
    full = ('s', 'mz', 'out', 'da', 'du') + PARAM_GRADS
    for bias, kb in ((True, True),) if light else ((True, True), (False, False)):
        ref, t32 = A.ca_eval(inp, F64, bias, kb), A.ca_eval(inp, F32, bias, kb)
        first, second = (_ca_run(inp, n, hw, c, hid, bias, kb) for _ in range(2))
        outs = full if bias else tuple(k for k in full if k not in ('db1', 'db2'))
        tab.buffers(first, full)
        tab.buffers(second, full)
        sub = A.Table('%s %s bias %d kb %d' % (tab.case, label, bias, kb))
        sub.check_all({k: first.get(k) for k in outs}, ref, A.bars(ref, t32, 'hat_combine'))
        tab.bad += sub.bad
        tab.worst = max(tab.worst, sub.worst)
        tab.rerun(first, second, full)
        _da_bits(tab, label, first, inp, kb)
        if bias:
            base = first
    if light:
        return base
    # the MLP form: out = x + kb a, nothing else read or written
    ref, t32 = A.ca_eval(inp, F64, with_u=False), A.ca_eval(inp, F32, with_u=False)
    b = _ca_run(inp, n, hw, c, hid, with_u=False)
    tab.buffers(b, ('out', 'da'))
    sub = A.Table('%s %s MLP form' % (tab.case, label))
    sub.check_all({k: b.get(k) for k in ('out', 'da')}, ref, A.bars(ref, t32, 'hat_combine'))
    tab.bad += sub.bad
    tab.worst = max(tab.worst, sub.worst)
    _da_bits(tab, label + ' MLP', b, inp, True)
    # du NULL: da only
    b = _ca_run(inp, n, hw, c, hid, du=False)
    tab.buffers(b, ('s', 'mz', 'out', 'da'))
    _da_bits(tab, label + ' no du', b, inp, True)
    # each parameter gradient NULL once: the others keep their bits, the slot not given stays untouched
    for skip in PARAM_GRADS:
        b = _ca_run(inp, n, hw, c, hid, skip=skip)
        tab.buffers(b, [k for k in full if k != skip])
        tab.require(b.all[skip].untouched(), '%s %s written though NULL was passed' % (label, skip))
        for k in ('da', 'du') + PARAM_GRADS:
            if k != skip:
                tab.same_bits('%s no %s: %s' % (label, skip, k), b.get(k), base.get(k))
    return base


@pytest.mark.parametrize('n', A.CA_N)
@pytest.mark.parametrize('c,hid', A.CA_DIMS)
def test_channel_attention_and_combine_with_every_optional_pointer(c, hid, n):
    """srhip_hat_ca_fwd, srhip_hat_combine_fwd and srhip_hat_combine_bwd at hw = 1, 7, 8, 9, 64, 729: biases given and NULL, kb with a
    zero entry and NULL, the MLP form (u NULL), du NULL, and each of dw1, db1, dw2, db2 NULL once.
    Worst err / bar on the MI355X: 0.34."""
    tab = A.Table('hat combine')
    for hw in A.CA_HW:
        _ca_case(tab, A.ca_inputs(n, hw, c, hid), n, hw, c, hid)
    tab.done()


def test_a_hidden_unit_at_exactly_zero_gets_no_gradient():
    """w1 row 0 and b1[0] zero: hidden unit 0 is exactly 0 before the ReLU, so dw1 row 0 and db1[0] are 0, as in torch.
    Worst err / bar on the MI355X: 0.13."""
    n, hw, c, hid = A.CA_ZERO_UNIT
    inp = A.ca_inputs(n, hw, c, hid, zero_unit=True)
    tab = A.Table('hat combine zero unit')
    b = _ca_case(tab, inp, n, hw, c, hid, light=True)
    tab.require(float(b.get('mz')[:, c].abs().max()) == 0.0, 'hidden unit 0 is not exactly 0')
    tab.require(float(b.get('dw1')[0].abs().max()) == 0.0 and float(b.get('db1')[0]) == 0.0, 'a gradient flows through the unit at 0')
    tab.done()


def test_combine_strides_past_its_grid_cap_across_images():
    """n = 3, hw = 11000, c = 128: 1,056,000 float4 > 4096 x 256, so the combine kernels' second sweep runs, in the third image, with a
    kb that differs per image.  Worst err / bar on the MI355X: 0.20."""
    n, hw, c, hid = A.CA_BIG
    tab = A.Table('hat combine big')
    _ca_case(tab, A.ca_inputs(n, hw, c, hid), n, hw, c, hid, light=True)
    tab.done()


# --------------------------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------------------------- #


def test_refusals_leave_every_buffer_untouched():
    """The list tests/test_attn_kernels_ref_cpu.py has passed without a device, again on real guarded buffers: every call returns its
    error code from the host-side checks, and nothing is written."""
    from tests.pointwise_ref import Guarded
    lib = _lib()
    bufs = {k: Guarded((2 * 16 * 16 * 288,), DEV) for k in 'abcdefghijkl'}
    bufs['ws'] = Guarded((1 << 21,), DEV)
    p = {k: g.ptr() for k, g in bufs.items()}
    p['ws_bytes'] = 4 << 21
    bad = []
    for label, code, call in A.hat_refusals(lib, p):
        rc = call()
        if rc != code or not lib.srhip_last_error():
            bad.append((label, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(g.untouched() for g in bufs.values()), [k for k, g in bufs.items() if not g.untouched()]
