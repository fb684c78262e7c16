"""csrc/hat_wide.hip and the wide channel attention of csrc/hat.hip -- LayerNorm at 144 / 180 channels, window attention (SA, shifted
SA, OCA) for heads of 24 / 30 channels at window 16, channel attention and the combine's backward at 144 / 180 channels -- one entry
point at a time through the C ABI against the float64 references of tests/hat_wide_ref.py.

Protocol of tests/test_hat_kernels_gpu.py: every tensor a kernel sees lies between sentinel bands, outputs and workspaces start as
NaN, workspaces are exactly as large as the library asks; afterwards the bands are intact, no NaN is left in an output, every tensor's
err = max|got - ref64| / max|ref64| is under max(8 x err of the fp32 CPU evaluation, 32 * 2^-24) capped by attn_kernels_ref.CAPS (not
on the x6 / ascending / descending attention families), and a second call on fresh guarded buffers gives the same bits.  Every
figure is printed before its test asserts."""
import pytest
import torch

from tests import attn_kernels_ref as A
from tests import hat_wide_ref as W
from tests.test_reductions_gpu import _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32

ATTN_OUT = ('out', 'lse', 'dqkv', 'dtable')


def _attn_run(inp):
    lib, b = _lib(), A.Buffers(DEV)
    kind, ws, shift, heads = inp['kind'], inp['ws'], inp['shift'], inp['heads']
    n, h, w, c3 = inp['qkv'].shape
    c = c3 // 3
    p = {k: b.put(k, inp[k]) for k in ('qkv', 'table', 'dout')}
    _ok(lib.srhip_hatw_attn_fwd(p['qkv'], p['table'], b.out('out', n, h, w, c), b.out('lse', n, h, w, heads), kind, n, h, w, c, heads, ws,
                                shift, _stream()), 'hatw_attn_fwd')
    torch.cuda.synchronize()
    need = lib.srhip_hatw_attn_bwd_workspace(kind, n, h, w, c, heads, ws)
    _ok(lib.srhip_hatw_attn_bwd(p['qkv'], p['table'], b.ptr('out'), p['dout'], b.ptr('lse'), b.out('dqkv', n, h, w, c3),
                                b.out('dtable', A.hat_table_rows(kind, ws), heads), b.workspace('ws', need), need, kind, n, h, w, c, heads,
                                ws, shift, _stream()), 'hatw_attn_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('case', W.ATTN_CASES, ids=[W.attn_id(c) for c in W.ATTN_CASES])
def test_window_attention_at_window_16(case):
    """srhip_hatw_attn_fwd / _bwd: out, lse, dqkv and dtable for one window and one head, every shift-mask region pair, both head
    widths, OCA's zero padding on every border, 75 windows (more than the dq kernel's 64 blocks per head), logits of tens, and key
    scores that rise / fall along the key tiles; each case twice, bit for bit.
    Worst err / bar on the MI355X: 0.26 over the seven random cases (OCA, 75 windows), 0.16 x6, 0.15 ascending, 0.16 descending."""
    inp = W.attn_inputs(case)
    ref, t32 = W.attn_eval(inp, F64), W.attn_eval(inp, F32)
    table = A.bars(ref, t32, 'hat_attn', case[7] not in W.ATTN_UNCAPPED)
    tab = A.Table('hatw attn ' + W.attn_id(case))
    first, second = _attn_run(inp), _attn_run(inp)
    tab.buffers(first, ATTN_OUT)
    tab.buffers(second, ATTN_OUT)
    tab.check_all({k: first.get(k) for k in ATTN_OUT}, ref, table)
    tab.rerun(first, second, ATTN_OUT)
    tab.done()


def _ln_run(inp, tokens, c, dadd=False, dgamma=True, dbeta=True):
    lib, b = _lib(), A.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('x', 'gamma', 'beta', 'dy', 'dadd')}
    _ok(lib.srhip_hatw_ln_fwd(p['x'], p['gamma'], p['beta'], b.out('y', tokens, c), b.out('mean', tokens), b.out('rstd', tokens), tokens, c,
                              _stream()), 'hatw_ln_fwd')
    torch.cuda.synchronize()
    b.out('dgamma', c)
    b.out('dbeta', c)
    _ok(lib.srhip_hatw_ln_bwd(p['dy'], p['x'], p['gamma'], b.ptr('mean'), b.ptr('rstd'), p['dadd'] if dadd else None, b.out('dx', tokens, c),
                              b.out('part', lib.srhip_hatw_ln_parts(tokens), 2 * c), b.ptr('dgamma') if dgamma else None,
                              b.ptr('dbeta') if dbeta else None, tokens, c, _stream()), 'hatw_ln_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('c,family,tokens', W.LN_CASES, ids=['%d-%s-%d' % x for x in W.LN_CASES])
def test_layer_norm_at_the_published_widths(c, family, tokens):
    """srhip_hatw_ln_fwd / _bwd at C = 144 and 180: y, mean, rstd, dx, dgamma, dbeta with `part` sized by srhip_hatw_ln_parts; dadd NULL
    and given; dgamma NULL once and dbeta NULL once (the other outputs keep their bits, the slot not given stays untouched).
    Worst err / bar on the MI355X: random 0.12, constant_token 0.12, mean_1000 0.13."""
    inp = W.ln_inputs(family, tokens, c)
    tab = A.Table('hatw ln %d %s %d' % (c, family, tokens))
    outs = ('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta')
    runs = {}
    for dadd in (False, True):
        ref, t32 = W.ln_eval(inp, F64, dadd), W.ln_eval(inp, F32, dadd)
        first, second = _ln_run(inp, tokens, c, dadd), _ln_run(inp, tokens, c, dadd)
        tab.buffers(first, outs + ('part',))
        tab.buffers(second, outs)
        tab.check_all({k: first.get(k) for k in outs}, ref, A.bars(ref, t32, 'hat_ln'))
        tab.rerun(first, second, outs)
        runs[dadd] = first
    for skip in ('dgamma', 'dbeta'):
        b = _ln_run(inp, tokens, c, True, dgamma=skip != 'dgamma', dbeta=skip != 'dbeta')
        tab.buffers(b, [k for k in outs if k != skip])
        tab.require(b.all[skip].untouched(), '%s written though NULL was passed' % skip)
        for k in outs:
            if k != skip:
                tab.same_bits('no %s: %s' % (skip, k), b.get(k), runs[True].get(k))
    tab.done()


PARAM_GRADS = ('dw1', 'db1', 'dw2', 'db2')


def _ca_run(inp, n, hw, c, hid, bias=True, kb=True, with_u=True):
    """hatw_ca_fwd -> hat_combine_fwd (any width) -> hatw_combine_bwd on the forward's own s and mz.  with_u False: the MLP form."""
    lib, b = _lib(), A.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('x', 'a', 'u', 'g', 'w1', 'b1', 'w2', 'b2', 'kb')}
    kbp = p['kb'] if kb else None
    if with_u:
        _ok(lib.srhip_hatw_ca_fwd(p['u'], p['w1'], p['b1'] if bias else None, p['w2'], p['b2'] if bias else None, b.out('s', n, c),
                                  b.out('mz', n, c + hid), n, hw, c, hid, _stream()), 'hatw_ca_fwd')
        torch.cuda.synchronize()
    _ok(lib.srhip_hat_combine_fwd(p['x'], p['a'], kbp, p['u'] if with_u else None, b.ptr('s') if with_u else None, b.out('out', n, hw, c), A.CS,
                                  n, hw, c, _stream()), 'hat_combine_fwd')
    torch.cuda.synchronize()
    b.out('da', n, hw, c)
    if not with_u:
        _ok(lib.srhip_hatw_combine_bwd(p['g'], kbp, None, None, None, None, None, b.ptr('da'), None, None, None, None, None, None, 0, A.CS,
                                       n, hw, c, hid, _stream()), 'hatw_combine_bwd')
    else:
        need = lib.srhip_hat_combine_bwd_workspace(n, c, hid)
        b.out('dw1', hid, c), b.out('db1', hid), b.out('dw2', c, hid), b.out('db2', c)
        _ok(lib.srhip_hatw_combine_bwd(p['g'], kbp, p['u'], b.ptr('s'), b.ptr('mz'), p['w1'], p['w2'], b.ptr('da'), b.out('du', n, hw, c),
                                       b.ptr('dw1'), b.ptr('db1'), b.ptr('dw2'), b.ptr('db2'), b.workspace('ws', need), need, A.CS, n, hw, c,
                                       hid, _stream()), 'hatw_combine_bwd')
    torch.cuda.synchronize()
    return b


def _ca_case(tab, inp, n, hw, c, hid):
    label = '%dx%dx%d/%d' % (n, hw, c, hid)
    full = ('s', 'mz', 'out', 'da', 'du') + PARAM_GRADS
    base = None
    for bias, kb in ((True, True), (False, False)):
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
        want = inp['g'] * inp['kb'].view(-1, 1, 1) if kb else inp['g']
        tab.same_bits(label + ' da', first.get('da'), want)                # da = kb[b] g is one fp32 multiply
        base = base or first
    ref, t32 = A.ca_eval(inp, F64, with_u=False), A.ca_eval(inp, F32, with_u=False)      # without u: out = x + kb a
    b = _ca_run(inp, n, hw, c, hid, with_u=False)
    tab.buffers(b, ('out', 'da'))
    sub = A.Table('%s %s MLP form' % (tab.case, label))
    sub.check_all({k: b.get(k) for k in ('out', 'da')}, ref, A.bars(ref, t32, 'hat_combine'))
    tab.bad += sub.bad
    tab.worst = max(tab.worst, sub.worst)
    return base


@pytest.mark.parametrize('n', W.CA_N)
@pytest.mark.parametrize('c,hid', W.CA_DIMS)
def test_channel_attention_and_combine_at_the_published_widths(c, hid, n):
    """srhip_hatw_ca_fwd, srhip_hat_combine_fwd and srhip_hatw_combine_bwd at (C, hidden) = (144, 6), (180, 6), (180, 16) and
    hw = 1, 7, 8, 9, 256: biases given and NULL, kb with a zero entry and NULL, and the form without u.
    Worst err / bar on the MI355X: 0.43."""
    tab = A.Table('hatw combine')
    for hw in W.CA_HW:
        _ca_case(tab, A.ca_inputs(n, hw, c, hid), n, hw, c, hid)
    tab.done()


def test_a_hidden_unit_at_exactly_zero_gets_no_gradient_at_180_channels():
    """w1 row 0 and b1[0] zero: hidden unit 0 is exactly 0 before the ReLU, so dw1 row 0 and db1[0] are 0, as in torch.
    Worst err / bar on the MI355X: 0.20."""
    n, hw, c, hid = W.CA_ZERO_UNIT
    inp = A.ca_inputs(n, hw, c, hid, zero_unit=True)
    tab = A.Table('hatw combine zero unit')
    b = _ca_case(tab, inp, n, hw, c, hid)
    tab.require(float(b.get('mz')[:, c].abs().max()) == 0.0, 'hidden unit 0 is not exactly 0')
    tab.require(float(b.get('dw1')[0].abs().max()) == 0.0 and float(b.get('db1')[0]) == 0.0, 'a gradient flows through the unit at 0')
    tab.done()


def test_refusals_leave_every_buffer_untouched():
    """hat_wide_ref.refusals on real guarded buffers: every call returns its error code from the host-side checks with a message, and
    nothing is written."""
    from tests.pointwise_ref import Guarded
    lib = _lib()
    bufs = {k: Guarded((2 * 16 * 16 * 540,), DEV) for k in 'abcdefghijkl'}
    bufs['ws'] = Guarded((1 << 21,), DEV)
    p = {k: g.ptr() for k, g in bufs.items()}
    p['ws_bytes'] = 4 << 21
    bad = []
    for label, code, call in W.refusals(lib, p):
        rc = call()
        if rc != code or not lib.srhip_last_error():
            bad.append((label, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(g.untouched() for g in bufs.values()), [k for k, g in bufs.items() if not g.untouched()]
