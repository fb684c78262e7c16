"""csrc/attn_variants.hip -- forward, closing kernels and backward of every ablation of the RAB / ResGroup attention tail (la_mode x
pool_mode) -- against the fp64 reference of tests/attn_variants_ref.py, through the C entry points (ctypes), at shapes with empty pooling
segments, hw < 16 and W < 7, n not a power of two and W > 64, on the input families of tests/attn_tail_ref.py.

The measure per output tensor is err = max|got - ref64| / max|ref64|, the bar max(8 x err of stock fp32 torch on the CPU, 32 * 2^-24)
(reduction_ref.err / bound).  No element is excluded: every input is shown, in the fp64 reference alone and before a kernel's output is
looked at, to keep the arg-max and ReLU decisions of all 15 forward configurations away from a flip (attn_variants_ref.assert_margins),
and the kernels' arg-max indices must then equal the reference's everywhere.  Outputs start as NaN / -7 and workspaces as NaN."""
import pytest
import torch

from tests import attn_variants_ref as V
from tests.test_reductions_gpu import _Table, _lib, _ok, _p, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
C = V.C
SAVED = ('avg', 'mx', 'arg', 's', 'pooled', 'argc', 'm')

_cache = {}


def _inputs(case):
    """The inputs of a case, once; the margin precondition is asserted before anything else happens."""
    if case not in _cache:
        t = V.case_inputs(*case)
        V.assert_margins(t, V.case_id(case))
        _cache[case] = dict(t=t)
    return _cache[case]['t']


def _refs(case, mode, pool):
    """(fp64 reference, stock fp32 torch) of one forward configuration of a case, once."""
    t, ent = _inputs(case), _cache[case]
    if (mode, pool) not in ent:
        ent[(mode, pool)] = (V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool),
                             V.variant_torch(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool))
    return ent[(mode, pool)]


def _nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def _present(mode, pool):
    """Which of SAVED a configuration has."""
    has_c, has_s = 'CA' in mode, 'SA' in mode
    return dict(avg=has_c and 'Avg' in pool, mx=has_c and 'Max' in pool, arg=has_c and 'Max' in pool, s=has_c, pooled=has_s,
                argc=has_s and 'Max' in pool, m=has_s)


def _fwd(t, mode, pool, c=C, hidden=None, check=True):
    """srhip_attn_var_fwd on device copies of a case's inputs; absent outputs are passed as NULL."""
    lib = _lib()
    n, _, h, w = t['u'].shape
    npix, np_ = n * h * w, len(V.pool_rows(pool))
    hidden = t['hidden'] if hidden is None else hidden
    ints = lambda *s: torch.full(s, -7, device=DEV, dtype=torch.int32)
    full = dict(avg=_nan(n, C), mx=_nan(n, C), arg=ints(n, C), s=_nan(n, C), pooled=_nan(npix, np_), argc=ints(npix), m=_nan(npix))
    has = _present(mode, pool)
    o = {k: (v if has[k] else None) for k, v in full.items()}
    u = _nhwc(t['u'])
    fc1, fc2, w7 = t['fc1'].contiguous().to(DEV), t['fc2'].contiguous().to(DEV), V.w7_of(t['w7'], pool).to(DEV)
    ws = _nan(lib.srhip_attn_var_workspace(n) // 4)
    rc = lib.srhip_attn_var_fwd(_p(u), _p(fc1), _p(fc2), _p(w7), *[_p(o[k]) for k in SAVED], _p(ws), ws.numel() * 4, n, h, w, c, hidden,
                                V.ORDER[mode], V.POOL_BITS[pool], _stream())
    torch.cuda.synchronize()
    if check:
        _ok(rc, 'attn_var_fwd')
    return rc, o, u


def _shaped(o, n, hw):
    """The saved tensors in the reference's shapes."""
    view = dict(pooled=lambda x: x.view(n, hw, -1), argc=lambda x: x.view(n, hw), m=lambda x: x.view(n, hw))
    return {k: (view.get(k, lambda x: x)(v) if v is not None else None) for k, v in o.items()}


CASE_IDS = [V.case_id(c) for c in V.CASES]
FWD_IDS = [V.variant_id(f) for f in V.FORWARDS]


@pytest.mark.parametrize('mode,pool', V.FORWARDS, ids=FWD_IDS)
@pytest.mark.parametrize('case', V.CASES, ids=CASE_IDS)
def test_forward_saved_tensors_against_fp64(case, mode, pool):
    """The 15 forward configurations behind the 21 variants (addconv does not reach the gates): arg / argc integer-equal to the first
    arg-max of the fp64 reference, a maximum of u itself bit-exact, everything else at the bar, every output finite (all_negative: the
    -inf a maximum starts from does not leak) and no output a variant lacks demanded."""
    t = _inputs(case)
    ref, y32 = _refs(case, mode, pool)
    n, hw = t['u'].shape[0], t['u'].shape[2] * t['u'].shape[3]
    _, o, _ = _fwd(t, mode, pool)
    got = _shaped(o, n, hw)
    tab = _Table('var fwd %s %s' % (V.case_id(case), V.variant_id((mode, pool))))
    for k in ('arg', 'argc'):
        if ref[k] is not None:
            idx = got[k].cpu().long()
            assert torch.equal(idx, ref[k]), '%s: first maximum differs at %s' % (k, (idx != ref[k]).nonzero()[:4].tolist())
        else:
            assert got[k] is None
    if ref['mx'] is not None and mode != 'SA-CA':
        tab.same_bits('mx is the exact maximum', got['mx'].cpu().double(), ref['mx'])
    for k in ('avg', 'mx', 's', 'pooled', 'm'):
        if ref[k] is not None:
            assert bool(torch.isfinite(got[k]).all()), k
            tab.check(k, got[k], ref[k], y32[k])
    tab.done()


def _close_expected(mode, u, s, m, skip):
    """The fp32 expression of srhip_attn_var_close, one rounding per product and per add (CPU tensors, NHWC [n, hw, 64])."""
    s_, m_ = (s[:, None, :] if s is not None else None), (m[:, :, None] if m is not None else None)
    if mode == 'CA-SA':
        return m_ * (s_ * u) + skip
    if mode == 'SA-CA':
        return s_ * (m_ * u) + skip
    if mode == 'CA':
        return s_ * u + skip
    if mode == 'SA':
        return m_ * u + skip
    return torch.cat([s_ * u, m_ * u], 2)


@pytest.mark.parametrize('mode', V.MODES, ids=[m.replace('|', '+') for m in V.MODES])
@pytest.mark.parametrize('shape', V.SHAPES, ids=['%dx%dx%d' % s for s in V.SHAPES])
def test_closing_kernels_equal_the_fp32_expression(shape, mode):
    """gate-and-add (CA-SA, SA-CA, CA, SA) and the gated cat (CA|SA): a product of at most three fp32 factors and one add, contraction
    off -- torch.equal to the same expression in stock fp32 torch, in the order of the la_mode."""
    n, h, w = shape
    hw = h * w
    g = torch.Generator().manual_seed(11 + hw)
    u, skip = torch.randn(n, hw, C, generator=g), torch.randn(n, hw, C, generator=g)
    s = torch.rand(n, C, generator=g) if 'CA' in mode else None
    m = torch.rand(n, hw, generator=g) if 'SA' in mode else None
    cat = mode == 'CA|SA'
    out = _nan(n, hw, 2 * C if cat else C)
    dev = lambda x: x.to(DEV) if x is not None else None
    du, ds, dm, dskip = dev(u), dev(s), dev(m), dev(skip)
    _ok(_lib().srhip_attn_var_close(_p(du), _p(ds), _p(dm), None if cat else _p(dskip), _p(out), n, hw, C, V.ORDER[mode], int(cat), _stream()),
        'attn_var_close')
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _close_expected(mode, u, s, m, skip))


@pytest.mark.parametrize('case', [c for c in V.CASES if c[0] in ('normal', 'pixel_ties', 'channel_ties')], ids=V.case_id)
def test_default_variant_matches_the_fused_tail(case):
    """CA-SA / Avg|Max through the new kernels against srhip_attn_tail_fwd: the indices exactly, the values within the bar."""
    t = _inputs(case)
    lib = _lib()
    n, _, h, w = t['u'].shape
    npix = n * h * w
    ref, y32 = _refs(case, 'CA-SA', 'Avg|Max')
    _, o, u = _fwd(t, 'CA-SA', 'Avg|Max')
    ints = lambda *s: torch.full(s, -7, device=DEV, dtype=torch.int32)
    f = dict(avg=_nan(n, C), mx=_nan(n, C), arg=ints(n, C), s=_nan(n, C), pooled=_nan(npix, 2), argc=ints(npix), m=_nan(npix))
    ws = _nan(lib.srhip_attn_tail_workspace(n) // 4)
    fc1, fc2, w7 = t['fc1'].to(DEV), t['fc2'].to(DEV), t['w7'].contiguous().to(DEV)       # (named: a temporary's memory is reused at once)
    _ok(lib.srhip_attn_tail_fwd(_p(u), _p(fc1), _p(fc2), _p(w7), *[_p(f[k]) for k in SAVED], _p(ws), ws.numel() * 4, n, h, w, C, t['hidden'], _stream()), 'attn_tail_fwd')
    torch.cuda.synchronize()
    assert torch.equal(o['arg'], f['arg']) and torch.equal(o['argc'], f['argc'])
    got, old = _shaped(o, n, h * w), _shaped(f, n, h * w)
    tab = _Table('var default ' + V.case_id(case))
    for k in ('avg', 'mx', 's', 'pooled', 'm'):
        tab.check(k, got[k], ref[k], y32[k])
        tab.check('fused tail ' + k, old[k], ref[k], y32[k])
    tab.done()


GRADS = ('du', 'dfc1', 'dfc2', 'dw7')


def _bwd(t, mode, pool, o, u, acc7=0, accfc=0, pre=None, c=C, check=True):
    """srhip_attn_var_bwd on the saved tensors `o` of _fwd.  Outputs start as NaN, or as the case's pre_* tensors when accumulating."""
    lib = _lib()
    n, _, h, w = t['u'].shape
    np_, hid = len(V.pool_rows(pool)), t['hidden']
    has_c, has_s = 'CA' in mode, 'SA' in mode
    dz = _nhwc(V.case_dz(t, mode))
    fc1, fc2, w7 = t['fc1'].contiguous().to(DEV), t['fc2'].contiguous().to(DEV), V.w7_of(t['w7'], pool).to(DEV)
    start = lambda name, *s: pre[name].reshape(*s).contiguous().to(DEV) if pre is not None else _nan(*s)
    g = dict(du=_nan(n, h, w, C), dfc1=start('pre_fc1', hid, C) if has_c else None, dfc2=start('pre_fc2', C, hid) if has_c else None,
             dw7=(V.w7_of(pre['pre_w7'], pool).to(DEV) if pre is not None else _nan(1, np_, 7, 7)) if has_s else None)
    ws = _nan(lib.srhip_attn_var_bwd_workspace(n, h, w, hid) // 4)
    rc = lib.srhip_attn_var_bwd(_p(dz), _p(u), _p(o['s']), _p(o['m']), _p(o['avg']), _p(o['mx']), _p(o['arg']), _p(o['pooled']), _p(o['argc']),
                                _p(w7), _p(fc1), _p(fc2), _p(g['du']), _p(g['dw7']), acc7, _p(g['dfc1']), _p(g['dfc2']), accfc, _p(ws),
                                ws.numel() * 4, n, h, w, c, hid, V.ORDER[mode], V.POOL_BITS[pool], _stream())
    torch.cuda.synchronize()
    if check:
        _ok(rc, 'attn_var_bwd')
    g['du'] = g['du'].permute(0, 3, 1, 2)
    if g['dw7'] is not None:
        g['dw7'] = g['dw7'].view(np_, 7, 7)
    return rc, g


@pytest.mark.parametrize('mode,pool', V.FORWARDS, ids=FWD_IDS)
@pytest.mark.parametrize('case', V.CASES, ids=CASE_IDS)
def test_backward_against_fp64(case, mode, pool):
    """du, dfc1, dfc2, dw7 of srhip_attn_var_bwd against fp64 autograd of the gather formulation at the (asserted) first arg-max
    indices; the bar from the same formulation in stock fp32 torch.  No element excluded; every output finite."""
    t = _inputs(case)
    ref, _ = _refs(case, mode, pool)
    _, o, u = _fwd(t, mode, pool)
    for k in ('arg', 'argc'):
        if ref[k] is not None:
            assert torch.equal(o[k].cpu().long().view(ref[k].shape), ref[k]), k
    dz = V.case_dz(t, mode)
    want = V.variant_grads(dz, t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool, ref['arg'], ref['argc'])
    y32 = V.variant_grads(dz, t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool, ref['arg'], ref['argc'], torch.float32)
    _, got = _bwd(t, mode, pool, o, u)
    tab = _Table('var bwd %s %s' % (V.case_id(case), V.variant_id((mode, pool))))
    for k in GRADS:
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            tab.check(k, got[k], want[k], y32[k])
    tab.done()


@pytest.mark.parametrize('mode,pool', V.FORWARDS, ids=FWD_IDS)
@pytest.mark.parametrize('shape', [(3, 10, 12), (2, 13, 70)], ids=['3x10x12', '2x13x70'])
def test_accumulate_flags_add_the_same_sum_and_runs_repeat(shape, mode, pool):
    """With the flags set the parameter gradients are `pre + sum` with the very sum the plain call writes (one fp32 add); du does
    not change; a second plain run gives the same bits."""
    t = _inputs(('normal',) + shape)
    _, o, u = _fwd(t, mode, pool)
    _, plain = _bwd(t, mode, pool, o, u)
    _, again = _bwd(t, mode, pool, o, u)
    _, acc = _bwd(t, mode, pool, o, u, acc7=1, accfc=1, pre=t)
    hid = t['hidden']
    pre = dict(dfc1=t['pre_fc1'].reshape(hid, C), dfc2=t['pre_fc2'].reshape(C, hid), dw7=V.w7_of(t['pre_w7'], pool)[0])
    for k in GRADS:
        if plain[k] is None:
            continue
        assert torch.equal(plain[k], again[k]), k
        want = plain[k] if k == 'du' else pre[k].to(DEV) + plain[k]
        assert torch.equal(acc[k], want), k


@pytest.mark.parametrize('mode,pool', [f for f in V.FORWARDS if 'CA' in f[0]], ids=[V.variant_id(f) for f in V.FORWARDS if 'CA' in f[0]])
@pytest.mark.parametrize('hidden', V.HIDDENS)
def test_other_hidden_sizes_against_fp64(hidden, mode, pool):
    """hidden in {1, 5, 16} through the forward and backward MLP kernels of every configuration with a channel gate: saved tensors,
    indices and all four gradients at the bars of the hidden = 4 tests."""
    t = V.case_inputs('normal', *V.HIDDEN_SHAPE, hidden=hidden)
    V.assert_margins(t, 'hidden %d' % hidden)
    n, hw = t['u'].shape[0], t['u'].shape[2] * t['u'].shape[3]
    ref = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)
    f32 = V.variant_torch(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)
    _, o, u = _fwd(t, mode, pool)
    got = _shaped(o, n, hw)
    tab = _Table('var hidden %d %s' % (hidden, V.variant_id((mode, pool))))
    for k in ('arg', 'argc'):
        if ref[k] is not None:
            assert torch.equal(got[k].cpu().long(), ref[k]), k
    for k in ('avg', 'mx', 's', 'pooled', 'm'):
        if ref[k] is not None:
            tab.check(k, got[k], ref[k], f32[k])
    dz = V.case_dz(t, mode)
    want = V.variant_grads(dz, t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool, ref['arg'], ref['argc'])
    y32 = V.variant_grads(dz, t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool, ref['arg'], ref['argc'], torch.float32)
    _, g = _bwd(t, mode, pool, o, u)
    for k in GRADS:
        if want[k] is not None:
            tab.check(k, g[k], want[k], y32[k])
    tab.done()


def test_backward_refuses_unsupported_sizes_before_any_launch():
    t = _inputs(('normal', 2, 3, 5))
    _, o, u = _fwd(t, 'CA-SA', 'Avg|Max')
    rc, g = _bwd(t, 'CA-SA', 'Avg|Max', o, u, c=32, check=False)
    assert rc == -1 and _lib().srhip_last_error()
    assert all(bool(torch.isnan(g[k]).all()) for k in GRADS)


@pytest.mark.parametrize('mode,pool', V.FORWARDS, ids=FWD_IDS)
def test_two_runs_give_the_same_bits(mode, pool):
    t = _inputs(('normal', 2, 13, 70))
    _, a, _ = _fwd(t, mode, pool)
    _, b, _ = _fwd(t, mode, pool)
    for k in SAVED:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


REFUSED = [('CA-SA', 'Avg|Max'), ('SA-CA', 'Max'), ('CA', 'Avg'), ('CA|SA', 'Avg')]


@pytest.mark.parametrize('mode,pool', REFUSED, ids=[V.variant_id(f) for f in REFUSED])
def test_unsupported_sizes_are_refused_before_any_launch(mode, pool):
    """C = 32 and hidden = 17 return SRHIP_ERR_ARG with a message and leave every output as it was."""
    lib = _lib()
    t = _inputs(('normal', 2, 3, 5))
    for kw in (dict(c=32), dict(hidden=17)):
        rc, o, _ = _fwd(t, mode, pool, check=False, **kw)
        assert rc == -1 and lib.srhip_last_error()
        for k in ('avg', 'mx', 's', 'pooled', 'm'):
            assert o[k] is None or bool(torch.isnan(o[k]).all()), k
        for k in ('arg', 'argc'):
            assert o[k] is None or bool((o[k] == -7).all()), k
    n, hw = 2, 15
    out = _nan(n, hw, C)
    z = torch.zeros(n, hw, C, device=DEV)
    rc = lib.srhip_attn_var_close(_p(z), _p(z), _p(z), _p(z), _p(out), n, hw, 32, V.ORDER[mode], int(mode == 'CA|SA'), _stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(out).all())
    rc = lib.srhip_attn_var_close(_p(z), _p(z), _p(z), _p(z), _p(out), n, hw, C, V.ORDER[mode], int(mode != 'CA|SA'), _stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(out).all())


@pytest.mark.parametrize('variant', V.VARIANTS, ids=V.variant_id)
def test_a_nan_activation_reaches_the_gates_and_the_output(variant):
    """One NaN in u: the channel gate of its image and the spatial gate at its pixel are NaN (a NaN beats every number in a max pool
    and poisons a mean), and so is the tail's output there -- through ops.attention_variant, the route the modules take."""
    from sradsgan_amd import ops
    mode, pool, addconv = variant
    t = _inputs(('normal', 3, 10, 12))
    n, _, h, w = t['u'].shape
    u = t['u'].clone()
    u[1, 5, 4, 7] = float('nan')
    u, skip = u.to(DEV).contiguous(memory_format=torch.channels_last), t['skip'].to(DEV)
    has_c, has_s = 'CA' in mode, 'SA' in mode
    fc1 = t['fc1'].reshape(4, C, 1, 1).to(DEV) if has_c else None
    fc2 = t['fc2'].reshape(C, 4, 1, 1).to(DEV) if has_c else None
    w7 = V.w7_of(t['w7'], pool).to(DEV) if has_s else None
    wc = bc = None
    if mode == 'CA|SA':
        wc, bc = t['wc2'].to(DEV), t['bc'].to(DEV)
    elif '-' in mode and addconv:
        wc, bc = t['wc'].to(DEV), t['bc'].to(DEV)
    with torch.no_grad():
        assert ops.attention_variant_supported(u, mode, fc1, w7)
        s, m, _ = ops.attention_variant_gates(u, mode, pool, fc1, fc2, w7)
        out = ops.attention_variant(u, skip, mode, pool, fc1, fc2, w7, wc, bc)
    torch.cuda.synchronize()
    if has_c:
        assert bool(torch.isnan(s[1]).all()) and bool(torch.isfinite(s[0]).all()) and bool(torch.isfinite(s[2]).all())
    if has_s:
        assert bool(torch.isnan(m.view(n, h, w)[1, 4, 7])) and bool(torch.isfinite(m.view(n, h, w)[0]).all())
    assert bool(torch.isnan(out[1, :, 4, 7]).any()) and bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all())


@pytest.mark.parametrize('variant', V.VARIANTS, ids=V.variant_id)
def test_variant_tail_against_fp64_end_to_end(variant):
    """tail(u) + skip of all 21 variants through ops.attention_variant (gates, then the 1x1 conv with m and s as its scales, the
    gated cat + 128 -> 64 conv, or gate-and-add) against fp64, exact-fp32 conv arithmetic: rel_err < 1e-3, the module-level bar."""
    from sradsgan_amd import ops
    from tests.parity_util import rel_err
    mode, pool, addconv = variant
    t = _inputs(('normal', 3, 10, 12))
    ref, _ = _refs(('normal', 3, 10, 12), mode, pool)
    has_c, has_s = 'CA' in mode, 'SA' in mode
    fc1 = t['fc1'].reshape(4, C, 1, 1).to(DEV) if has_c else None
    fc2 = t['fc2'].reshape(C, 4, 1, 1).to(DEV) if has_c else None
    w7 = V.w7_of(t['w7'], pool).to(DEV) if has_s else None
    wc = bc = None
    if mode != 'CA|SA' and not ('-' in mode and addconv):
        want = ref['z'] + t['skip'].double()
    else:
        wc_cpu = t['wc2'] if mode == 'CA|SA' else t['wc']
        wc, bc = wc_cpu.to(DEV), t['bc'].to(DEV)
        want = (torch.einsum('oc,bchw->bohw', wc_cpu.double().reshape(C, -1), ref['z']) + t['bc'].double().view(1, C, 1, 1)
                + t['skip'].double())
    with ops.conv_math('fp32'), torch.no_grad():
        out = ops.attention_variant(t['u'].to(DEV), t['skip'].to(DEV), mode, pool, fc1, fc2, w7, wc, bc)
    e = rel_err(out, want)
    print('variant %s: rel_err %.3e' % (V.variant_id(variant), e))
    assert e < 1e-3
