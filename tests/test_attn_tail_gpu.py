"""csrc/attn_tail.hip -- the fused CLAM -> SLAM -> 1x1 conv -> skip tail of every RAB and ResGroup -- against the independent fp64
reference of tests/attn_tail_ref.py, through the tail's own C entry points (ctypes), at the shapes where its launch geometry changes
(tests/attn_tail_ref.py SHAPES) and on inputs built to hit the arg-max edges (ties over pixels and over channels, a maximum in the
last pixel of the last pooling segment, all-negative tensors).

The measure per output tensor is err = max|got - ref64| / max|ref64|, the bar max(8 x err of stock fp32 torch on the CPU, 32 * 2^-24)
(reduction_ref.err / bound): the code under test never sets its own bar.  Every check prints `err torch-fp32-err bound` before the
test asserts; bit-identity claims use torch.equal.  No element is ever excluded: instead every input is shown -- in the fp64 reference
alone, before a kernel's output is looked at -- to keep its arg-max and ReLU decisions away from a flip (attn_tail_ref.assert_margins),
and the kernels' arg-max indices must then equal the reference's everywhere."""
import pytest
import torch

from tests import attn_tail_ref as A
from tests import conv_emulation as E
from tests import reduction_ref as R
from tests.test_reductions_gpu import _Table, _lib, _ok, _p, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
C = A.C
ROUTES = (0, 32, 16, 48)        # srhip_debug_set(7, .): 0 = the 7x7 data gradient inside the main pass (wide images fall back on their own),
#                                 32 = the earlier launch sequence, 16 = its 7x7 backward as two launches (acts wherever that sequence runs)
SAVED = ('avg', 'mx', 'arg', 's', 'pooled', 'argc', 'm')
GRADS = ('du', 'dfc1', 'dfc2', 'dw7')

_cache = {}


def _inputs(case):
    """(inputs, fp64 forward reference) of a case, once; the margin precondition is asserted before anything else happens."""
    if case not in _cache:
        t = A.case_inputs(*case)
        A.assert_margins(t, A.case_id(case))
        _cache[case] = dict(t=t, f=A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7']))
    return _cache[case]['t'], _cache[case]['f']


def _backward_refs(case, arg, argc):
    """(fp64 closed forms, stock fp32 torch) of the backward, the max pools differentiated at the indices the kernels produced --
    which the caller has asserted to be the reference's own, so one evaluation serves every test of the case."""
    ent = _cache[case]
    if 'b' not in ent:
        t = ent['t']
        ent['b'] = A.tail_bwd_parts(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], arg, argc)
        ent['y32'] = A.tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], t['dz'], torch.float32, arg, argc)
    return ent['b'], ent['y32']


def _nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


class _Tail:
    """The C entry points of attn_tail.hip on one case's device tensors.  Outputs start as NaN / -7, workspaces as NaN: whatever a
    kernel reads without having written it shows."""

    def __init__(self, t):
        self.lib = _lib()
        self.n, _, self.h, self.w = t['u'].shape
        self.npix = self.n * self.h * self.w
        self.hid = t['hidden']
        self.u, self.dz = _nhwc(t['u']), _nhwc(t['dz'])
        self.fc1, self.fc2, self.w7 = (t[k].contiguous().to(DEV) for k in ('fc1', 'fc2', 'w7'))
        self.dims = (self.n, self.h, self.w, C, self.hid)

    def new_saved(self):
        n, npix = self.n, self.npix
        ints = lambda *s: torch.full(s, -7, device=DEV, dtype=torch.int32)
        return dict(avg=_nan(n, C), mx=_nan(n, C), arg=ints(n, C), s=_nan(n, C), pooled=_nan(npix, 2), argc=ints(npix), m=_nan(npix))

    def pool(self):
        """(buffer, section bytes, segments) filled by the stand-alone pooling pass."""
        lib = self.lib
        sec = self.n * lib.srhip_clam_pool_max_segments() * C * 4
        buf = _nan(3 * sec // 4)
        _ok(lib.srhip_clam_pool_partial(_p(self.u), _p(buf), sec, self.n, self.h, self.w, C, _stream()), 'clam_pool_partial')
        return buf, sec, lib.srhip_clam_pool_segments()

    def fwd(self, pooled=False, check=True):
        lib, o = self.lib, self.new_saved()
        outs = [_p(o[k]) for k in SAVED]
        ins = (_p(self.fc1), _p(self.fc2), _p(self.w7))
        if pooled:
            buf, sec, nseg = self.pool()
            rc = lib.srhip_attn_tail_fwd_pooled(_p(self.u), _p(buf), sec, nseg, *ins, *outs, *self.dims, _stream())
        else:
            ws = _nan(lib.srhip_attn_tail_workspace(self.n) // 4)
            rc = lib.srhip_attn_tail_fwd(_p(self.u), *ins, *outs, _p(ws), ws.numel() * 4, *self.dims, _stream())
        torch.cuda.synchronize()
        if check:
            _ok(rc, 'attn_tail_fwd')
        return rc, o

    def new_grads(self, pre=None):
        k = lambda name, *s: pre[name].reshape(*s).contiguous().to(DEV) if pre is not None else _nan(*s)
        return dict(du=_nan(self.n, self.h, self.w, C), dfc1=k('pre_fc1', self.hid, C), dfc2=k('pre_fc2', C, self.hid), dw7=k('pre_w7', 98))

    def bwd(self, f, route=0, acc7=0, accfc=0, pre=None, check=True, pp_entry=True):
        """srhip_attn_tail_bwd_pp with du_pp = NULL (pp_entry False: srhip_attn_tail_bwd) under srhip_debug_set(7, route).  Returns du
        [n, 64, h, w], dfc1, dfc2, dw7 [2, 7, 7]."""
        lib, o = self.lib, self.new_grads(pre)
        ws = _nan(lib.srhip_attn_tail_bwd_fused_workspace(self.n, self.h, self.w, self.hid) // 4)
        head = (_p(self.dz), _p(self.u), _p(f['s']), _p(f['m']), _p(f['pooled']), _p(f['argc']), _p(f['avg']), _p(f['mx']), _p(f['arg']),
                _p(self.w7), _p(self.fc1), _p(self.fc2), _p(o['du']))
        rest = (_p(o['dw7']), acc7, _p(o['dfc1']), _p(o['dfc2']), accfc, _p(ws), ws.numel() * 4, *self.dims, _stream())
        lib.srhip_debug_set(7, route)
        try:
            rc = lib.srhip_attn_tail_bwd_pp(*head, None, *rest) if pp_entry else lib.srhip_attn_tail_bwd(*head, *rest)
            torch.cuda.synchronize()
        finally:
            lib.srhip_debug_set(7, 0)
        if check:
            _ok(rc, 'attn_tail_bwd_pp')
        return rc, dict(du=o['du'].permute(0, 3, 1, 2), dfc1=o['dfc1'], dfc2=o['dfc2'], dw7=o['dw7'].view(2, 7, 7))

    def standalone(self, f):
        """srhip_attn_tail_bwd_spatial -> _bwd_mlp -> _bwd_channel, chained as the header documents."""
        lib, o = self.lib, self.new_grads()
        n, h, w = self.n, self.h, self.w
        ds, davg, dmax = _nan(n, C), _nan(n, C), _nan(n, C)
        ws = _nan(lib.srhip_attn_tail_bwd_workspace(n, h, w) // 4)
        _ok(lib.srhip_attn_tail_bwd_spatial(_p(self.dz), _p(self.u), _p(f['s']), _p(f['m']), _p(f['pooled']), _p(f['argc']), _p(self.w7),
                                            _p(o['du']), _p(ds), _p(o['dw7']), 0, _p(ws), ws.numel() * 4, n, h, w, C, _stream()), 'bwd_spatial')
        ws2 = _nan(lib.srhip_attn_tail_mlp_workspace(n, self.hid) // 4)
        _ok(lib.srhip_attn_tail_bwd_mlp(_p(ds), _p(f['avg']), _p(f['mx']), _p(f['s']), _p(self.fc1), _p(self.fc2), _p(davg), _p(dmax),
                                        _p(o['dfc1']), _p(o['dfc2']), 0, _p(ws2), ws2.numel() * 4, n, C, self.hid, _stream()), 'bwd_mlp')
        _ok(lib.srhip_attn_tail_bwd_channel(_p(o['du']), _p(davg), _p(dmax), _p(f['arg']), n, h, w, C, _stream()), 'bwd_channel')
        torch.cuda.synchronize()
        return dict(du=o['du'].permute(0, 3, 1, 2), dfc1=o['dfc1'], dfc2=o['dfc2'], dw7=o['dw7'].view(2, 7, 7))


def _shaped(f, n, hw):
    """The saved tensors in the reference's shapes."""
    return dict(avg=f['avg'], mx=f['mx'], arg=f['arg'], s=f['s'], pooled=f['pooled'].view(n, hw, 2), argc=f['argc'].view(n, hw), m=f['m'].view(n, hw))


def _assert_indices(case, f, ref):
    """The kernels' arg-maxes equal the reference's EVERYWHERE: with the margins of the case there is no excuse for a difference."""
    n, hw = f['arg'].shape[0], f['argc'].numel() // f['arg'].shape[0]
    arg, argc = f['arg'].cpu().long(), f['argc'].cpu().long().view(n, hw)
    assert torch.equal(arg, ref['arg']), ('%s: first max pixel differs at (image, channel) %s' % (
        A.case_id(case), (arg != ref['arg']).nonzero()[:4].tolist()))
    assert torch.equal(argc, ref['argc']), ('%s: first max channel differs at (image, pixel) %s' % (
        A.case_id(case), (argc != ref['argc']).nonzero()[:4].tolist()))
    return arg, argc


def _forward_checked(case):
    """Runs the forward of a case and asserts its indices; returns (inputs, reference, device harness, saved tensors)."""
    t, ref = _inputs(case)
    dev = _Tail(t)
    _, f = dev.fwd()
    _assert_indices(case, f, ref)
    return t, ref, dev, f


CASE_IDS = [A.case_id(c) for c in A.ALL_CASES]


@pytest.mark.parametrize('case', A.ALL_CASES, ids=CASE_IDS)
def test_forward_saved_tensors_against_fp64(case):
    """srhip_attn_tail_fwd: mx bit-exact (a maximum is exact), arg / argc integer-equal, avg / s / pooled / m at the bar; the same call
    fed with srhip_clam_pool_partial's partials (srhip_attn_tail_fwd_pooled) saves the same bits.  hidden in {1, 5, 16} rides along
    at 3x10x12."""
    t, ref = _inputs(case)
    assert _lib().srhip_clam_pool_segments() == A.POOL_SEGMENTS
    dev = _Tail(t)
    n, hw = dev.n, dev.h * dev.w
    _, f = dev.fwd()
    _assert_indices(case, f, ref)
    got = _shaped(f, n, hw)
    tab = _Table('tail fwd ' + A.case_id(case))
    tab.same_bits('mx is the exact maximum', got['mx'].cpu().double(), ref['mx'])
    y32 = A.tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], None, torch.float32)       # torch's own maxima: a value does not depend on the index
    for k in ('avg', 's', 'pooled', 'm'):
        tab.check(k, got[k], ref[k], y32[k])
    _, fp = dev.fwd(pooled=True)
    for k in SAVED:
        tab.same_bits('fwd_pooled ' + k, fp[k], f[k])
    tab.done()


def _loser_checks(tab, t, case, got, ref_b, y32, arg, argc, route):
    """Tie families: du at the losing pixels / channels carries no arg-max contribution -- checked on exactly those elements, and the
    same elements of a reference that routes the gradient to the LOSER must miss the bar (else the check could not tell)."""
    n, _, h, w = t['u'].shape
    hw = h * w
    flat = lambda x: x.detach().cpu().double().reshape(n, C, hw)
    if t['family'] == 'pixel_ties':
        p1, p2 = A.tie_pixels(hw)
        wrong_arg = arg.clone()
        wrong_arg[:, A.TIE_C], wrong_arg[:, A.CONST_C] = p2, 1
        wrong = A.tail_bwd_parts(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], wrong_arg, argc)['du']
        subsets = [('du losing pixel of the tie', lambda x: flat(x)[:, A.TIE_C, p2]), ('du constant channel, pixels > 0', lambda x: flat(x)[:, A.CONST_C, 1:])]
    else:
        wrong_argc = argc.clone()
        for c1, c2 in A.CHANNEL_TIES:
            wrong_argc[argc == c1] = c2
        wrong = A.tail_bwd_parts(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], arg, wrong_argc)['du']
        subsets = [('du second channel of tie (%d, %d)' % (c1, c2), (lambda c: lambda x: flat(x)[:, c])(c2)) for c1, c2 in A.CHANNEL_TIES]
    for name, sub in subsets:
        tab.check('route %d %s' % (route, name), sub(got['du']), sub(ref_b['du']), sub(y32['du']))
        e_wrong, bar = R.err(sub(wrong), sub(ref_b['du'])), R.bound(R.err(sub(y32['du']), sub(ref_b['du'])))
        print('%-46s %-22s a gradient sent to the loser would be off by %.3e (bound %.3e)' % (tab.case, name, e_wrong, bar))
        assert e_wrong > 100 * bar, (name, e_wrong, bar)


@pytest.mark.parametrize('case', A.ALL_CASES, ids=CASE_IDS)
def test_backward_against_fp64(case):
    """srhip_attn_tail_bwd_pp (du_pp = NULL) on the kernels' own saved tensors and a random dz: du, dfc1, dfc2, dw7 against the closed
    forms, on the default route and under srhip_debug_set(7, 32 / 16 / 48).  1x4x430 takes the wide-image fallback without a key;
    1x4x422 is the widest image that does not (60 KB of dynamic LDS, with the static part the 64 KB a block may have)."""
    t, ref, dev, f = _forward_checked(case)
    arg, argc = _assert_indices(case, f, ref)
    ref_b, y32 = _backward_refs(case, arg, argc)
    tab = _Table('tail bwd ' + A.case_id(case))
    for route in ROUTES:
        _, got = dev.bwd(f, route)
        for k in GRADS:
            tab.check('route %d %s' % (route, k), got[k], ref_b[k], y32[k])
        if t['family'] in ('pixel_ties', 'channel_ties'):
            _loser_checks(tab, t, case, got, ref_b, y32, arg, argc, route)
    tab.done()


@pytest.mark.parametrize('shape', A.ACC_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_accumulate_flags_add_the_same_sum(shape):
    """accumulate_dw7 / accumulate_dfc: prefill + the non-accumulating result, bit for bit -- one fp32 add of the same sum, the kernels
    claim identical summation order -- and the flag that is off leaves its outputs plain."""
    case = ('normal',) + tuple(shape) + (4,)
    t, ref, dev, f = _forward_checked(case)
    pre = {k: t[k].reshape(-1).to(DEV) for k in ('pre_fc1', 'pre_fc2', 'pre_w7')}
    tab = _Table('tail bwd accumulate ' + A.case_id(case))
    for route in (0, 32, 48):
        _, plain = dev.bwd(f, route)
        for acc7, accfc in ((1, 1), (1, 0), (0, 1)):
            _, got = dev.bwd(f, route, acc7, accfc, pre=t)
            want = dict(plain)
            if acc7:
                want['dw7'] = pre['pre_w7'].view(2, 7, 7) + plain['dw7']
            if accfc:
                want['dfc1'], want['dfc2'] = pre['pre_fc1'].view(4, C) + plain['dfc1'], pre['pre_fc2'].view(C, 4) + plain['dfc2']
            for k in GRADS:
                tab.same_bits('route %d acc7=%d accfc=%d %s' % (route, acc7, accfc, k), got[k], want[k])
    tab.done()


def test_hidden_17_is_refused_before_any_launch():
    """hidden <= 16 is a limit of the kernels' LDS arrays: every entry point that takes `hidden` returns the error and leaves its
    outputs untouched."""
    from sradsgan_amd import _hip, ops
    t = A.tail_inputs('normal', 2, 3, 5, hidden=17, seed=0)
    dev = _Tail(t)
    lib = dev.lib
    untouched = lambda o: all(bool(torch.isnan(v).all()) if v.is_floating_point() else bool((v == -7).all()) for v in o.values())
    for pooled in (False, True):
        rc, o = dev.fwd(pooled, check=False)
        assert rc != 0 and b'hidden' in lib.srhip_last_error() and untouched(o), ('fwd', pooled)
    ok16 = _Tail(A.tail_inputs('normal', 2, 3, 5, hidden=16, seed=0))
    _, f = ok16.fwd()                                            # saved tensors of a legal call: only `hidden` is wrong below
    rc, o = dev.bwd(f, check=False)
    assert rc != 0 and b'hidden' in lib.srhip_last_error() and bool(torch.isnan(torch.cat([v.reshape(-1) for v in o.values()])).all())
    davg, dmax, dfc1, dfc2, ws = _nan(2, C), _nan(2, C), _nan(17, C), _nan(C, 17), _nan(lib.srhip_attn_tail_mlp_workspace(2, 17) // 4)
    rc = lib.srhip_attn_tail_bwd_mlp(_p(f['s']), _p(f['avg']), _p(f['mx']), _p(f['s']), _p(dev.fc1), _p(dev.fc2), _p(davg), _p(dmax), _p(dfc1),
                                     _p(dfc2), 0, _p(ws), ws.numel() * 4, 2, C, 17, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b'hidden' in lib.srhip_last_error()
    assert all(bool(torch.isnan(v).all()) for v in (davg, dmax, dfc1, dfc2))
    with ops.conv_math('bf16x3'), torch.no_grad(), pytest.raises(_hip.HipLibraryError, match='hidden'):
        ops._tail_forward_eval(_cl(t['u']), _cl(t['skip']), dev.fc1.view(17, C, 1, 1), dev.fc2.view(C, 17, 1, 1), dev.w7, t['wc'].to(DEV),
                               t['bc'].to(DEV))


@pytest.mark.parametrize('shape', A.STANDALONE_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_standalone_entry_points_chained(shape):
    """srhip_attn_tail_bwd_spatial + _bwd_mlp + _bwd_channel, which no Python code calls: within the bar of the reference, and
    bit-identical to the fused call under srhip_debug_set(7, 32) (`same arithmetic and summation orders`).  srhip_attn_tail_bwd, the
    entry without the plane argument, is srhip_attn_tail_bwd_pp(du_pp = NULL)."""
    case = ('normal',) + tuple(shape) + (4,)
    t, ref, dev, f = _forward_checked(case)
    arg, argc = _assert_indices(case, f, ref)
    ref_b, y32 = _backward_refs(case, arg, argc)
    got = dev.standalone(f)
    _, fused = dev.bwd(f, 32)
    _, entry = dev.bwd(f, 32, pp_entry=False)
    tab = _Table('tail bwd stand-alone ' + A.case_id(case))
    for k in GRADS:
        tab.check(k, got[k], ref_b[k], y32[k])
        tab.same_bits(k + ' == fused call, route 32', got[k], fused[k])
        tab.same_bits(k + ' srhip_attn_tail_bwd == _bwd_pp(NULL)', entry[k], fused[k])
    tab.done()


def _ops_params(t):
    hid = t['hidden']
    return [t['fc1'].reshape(hid, C, 1, 1).to(DEV), t['fc2'].reshape(C, hid, 1, 1).to(DEV), t['w7'].to(DEV), t['wc'].to(DEV), t['bc'].to(DEV)]


@pytest.mark.parametrize('shape', A.PLANE_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_du_planes_are_the_fp32_gradient(shape):
    """ops._tail_backward(du_pp=planes): tail_bwd_fix_kernel's plane output, decoded with ops.pp_to_f32, against the du of the fp32
    call on the same inputs.  hi = bf16(v) leaves |v - hi| <= 2^-9 |v|, lo = bf16(v - hi) leaves 2^-9 of that, and the decoder's one
    fp32 add 2^-24 |v|: every element within 2^-16 |du| (derived, not measured).  The pad / guard / tail rows of the buffer, zero
    before the call, are zero bits afterwards (n = 2: the image stride of the row index)."""
    from sradsgan_amd import ops
    if ops.get_conv_math() != 'bf16x3':
        pytest.skip('padded planes are the split-bf16 arithmetic')
    case = ('normal',) + tuple(shape) + (4,)
    t, _ = _inputs(case)
    n, h, w = shape
    lib = _lib()
    u, skip, g = _cl(t['u']), _cl(t['skip']), _cl(t['g'])
    par = _ops_params(t)
    guard = lib.srhip_pp_guard(w)
    b, y, x = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing='ij')
    rows = (guard + (b * (h + 1) + y) * (w + 1) + x).reshape(-1).to(DEV)
    for route in (0, 32):
        lib.srhip_debug_set(7, route)
        try:
            _, saved = ops._tail_forward(u, skip, *par)
            du32 = ops._tail_backward(g, u, *par, saved, True, skip_params=True)[0]
            pp = ops.plane_pool.get(n, C, h, w, DEV)
            assert pp.buf.shape[0] == lib.srhip_pp_plane_pixels(n, h, w)
            pad = torch.ones(pp.buf.shape[0], dtype=torch.bool, device=DEV)
            pad[rows] = False
            assert not bool(pp.buf.view(torch.int16)[pad].any()), 'a pooled plane buffer with dirty pad rows'
            none = ops._tail_backward(g, u, *par, saved, True, skip_params=True, du_pp=pp)[0]
            dec = ops.pp_to_f32(pp)
            torch.cuda.synchronize()
        finally:
            lib.srhip_debug_set(7, 0)
        assert none is None
        want = du32.double()
        ratio = float(((dec.double() - want).abs() / want.abs().clamp_min(1e-300)).max())
        print('tail du planes %dx%dx%d route %d: max |decoded - du| / |du| = %.3e  (bound 2^-16 = %.3e)' % (n, h, w, route, ratio, 2.0 ** -16))
        assert bool(((dec.double() - want).abs() <= 2.0 ** -16 * want.abs()).all()), ratio
        assert not bool(pp.buf.view(torch.int16)[pad].any()), 'the plane output wrote a pad / guard / tail row'
        ops.plane_pool.put(pp)


def _emulated(arith):
    """The three contractions of the 1x1 conv as tests/conv_emulation.py computes them for a conv arithmetic ({}: stock fp32)."""
    if arith == 'fp32':
        return {}
    fa, ga = ('bf16x3', 'bf16x3') if arith == 'bf16x3' else ('fp16', 'bf16')
    return dict(conv_fwd=lambda x, k: E.conv_fwd(x, k, arith=fa, with_abs=False)[0],
                conv_dgrad=lambda d, k: E.conv_dgrad(d, k, tuple(d.shape), arith=ga, with_abs=False)[0],
                conv_wgrad=lambda x, d: E.conv_wgrad(x, d, (C, C, 1, 1), arith=ga, with_abs=False)[0])


@pytest.mark.parametrize('mode', ['fp32', 'default', 'default-lds-dma'])
@pytest.mark.parametrize('shape', A.E2E_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_whole_tail_with_its_conv_forward_and_seven_gradients(shape, mode):
    """ops.attention_tail with the 1x1 conv and its bias: the output and the gradients at u, skip, fc1, fc2, w7, wc, bc against the
    reference composed with an fp64 1x1 conv.  Under ops.conv_math('fp32') the yardstick is stock fp32 torch; under the default
    arithmetic the yardstick's 1x1 conv is the split-bf16 emulation of tests/conv_emulation.py.  Problems this small send the 1x1
    conv to the exact-fp32 register kernel in every arithmetic; 'default-lds-dma' pins the conv and its data gradient to the LDS-DMA
    kernels the benchmark sizes take (srhip_debug_set(0, -1)), so the split products really run."""
    from sradsgan_amd import ops
    case = ('normal',) + tuple(shape) + (4,)
    t, ref = _inputs(case)
    arith = 'fp32' if mode == 'fp32' else ops.get_conv_math()
    with ops.conv_math(arith):
        _lib().srhip_debug_set(0, -1 if mode == 'default-lds-dma' else 0)
        try:
            u, skip = _cl(t['u']).requires_grad_(), _cl(t['skip']).requires_grad_()
            par = [p.requires_grad_() for p in _ops_params(t)]
            with torch.no_grad():
                _, saved = ops._tail_forward(u.detach(), skip.detach(), *[p.detach() for p in par])
            arg, argc = _assert_indices(case, dict(arg=saved[2], argc=saved[5]), ref)
            out = ops.attention_tail(u, skip, *par)
            assert type(out.grad_fn).__name__.startswith('_AttentionTail')          # the HIP path ran
            out.backward(_cl(t['g']))
            torch.cuda.synchronize()
        finally:
            _lib().srhip_debug_set(0, 0)
    got = dict(zip(A.E2E_NAMES, [out.detach(), u.grad, skip.grad] + [p.grad for p in par]))
    want = A.e2e_ref(t, arg, argc)
    y32 = A.e2e_torch32(t, arg, argc, **_emulated(arith))
    tab = _Table('tail end to end %s %s' % (A.case_id(case), arith))
    for k in A.E2E_NAMES:
        tab.check(k, got[k].reshape(want[k].shape), want[k], y32[k].reshape(want[k].shape))
    tab.done()


@pytest.mark.parametrize('shape', A.EVAL_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_eval_kernel_against_fp64(shape):
    """ops._tail_forward_eval (one fused kernel behind the pooling partials; split-bf16 only) against the fp64 reference -- so far it
    was only ever compared with the training forward.  With and without the bias, and fed with srhip_clam_pool_partial's partials."""
    from sradsgan_amd import ops
    case = ('normal',) + tuple(shape) + (4,)
    t, ref = _inputs(case)
    want = A.e2e_ref(t)['out']
    y32 = A.e2e_torch32(t, ref['arg'], ref['argc'], **_emulated('bf16x3'))['out']
    nobias = t['bc'].double().view(1, C, 1, 1)
    u, skip = _cl(t['u']), _cl(t['skip'])
    fc1, fc2, w7, wc, bc = _ops_params(t)
    tab = _Table('tail eval ' + A.case_id(case))
    with ops.conv_math('bf16x3'), torch.no_grad():
        out = ops._tail_forward_eval(u, skip, fc1, fc2, w7, wc, bc)
        out0 = ops._tail_forward_eval(u, skip, fc1, fc2, w7, wc, None)
        outp = ops._tail_forward_eval(u, skip, fc1, fc2, w7, wc, bc, pool=_Tail(t).pool())
        torch.cuda.synchronize()
    tab.check('out', out, want, y32)
    tab.check('out, no bias', out0, want - nobias, y32.double() - nobias)
    tab.same_bits('eval_pooled out', outp, out)
    tab.done()
