"""csrc/global_attn.hip -- CGAM and the flash-style SGAM, exact-fp32 and split-bf16 -- one entry point at a time through the C ABI
(ctypes) against the float64 references of tests/attn_kernels_ref.py, at the sizes where the launch geometry changes: hw below one key
tile, exactly 32 k and 128 k (no masked tail) and one off, hw = 1, more than 16384 pixels (the prep kernel's second sweep and more
than 64 dgamma partials, every image compared), soft-maxes that force or forbid the online rescale, and dgamma written, accumulated
onto a known value and not asked for.

Protocol of tests/test_cbam_gpu.py: EVERY tensor a kernel sees -- inputs, outputs, saved tensors, workspace -- lies inside a larger
allocation with a 64-element sentinel band on both sides; outputs and workspace start as NaN and the workspace is exactly the size the
library asks for.  After each call the bands are intact, no NaN is left in an output, err = max|got - ref64| / max|ref64| of every
tensor is under its bar (attn_kernels_ref: measured from the fp32 CPU evaluation and, for the split kernels, the split emulation;
capped by the older tests' bounds except on the sharp / ascending / descending families), and a second call on fresh guarded
buffers gives the same bits: the file uses no atomics.  Every figure is printed before its test asserts."""
import pytest
import torch

from tests import attn_kernels_ref as A
from tests.test_reductions_gpu import _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class _Arith:
    """exact: srhip_debug_set(4, 1), the all-fp32 kernels; else the default split-bf16 products (conv math 1)."""

    def __init__(self, exact):
        self.exact = exact

    def __enter__(self):
        lib = _lib()
        self.math = lib.srhip_get_conv_math()
        lib.srhip_set_conv_math(1)
        lib.srhip_debug_set(4, 1 if self.exact else 0)

    def __exit__(self, *exc):
        lib = _lib()
        lib.srhip_debug_set(4, 0)
        lib.srhip_set_conv_math(self.math)


# --------------------------------------------------------------------------------------------- #
# SGAM
# --------------------------------------------------------------------------------------------- #

SGAM_OUT = ('y', 'o', 'lse', 'dq', 'dk', 'dv')


def _sgam_ref(family, n, hw):
    def make():
        inp = A.sgam_inputs(family, n, hw)
        return inp, A.sgam_eval(inp, F64), A.sgam_eval(inp, F32), A.sgam_split_emulation(inp), A.sgam_scales(inp)
    return _once(('sgam', family, n, hw), make)


def _sgam_run(inp, n, hw, dgamma='write', prior=0.5):
    """forward, then backward from the forward's own saved o and lse.  dgamma: 'write' (accumulate 0 onto NaN), 'accumulate' (onto
    `prior`), 'null'."""
    lib, b = _lib(), A.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('q', 'k', 'v', 'x', 'gamma', 'dy')}
    _ok(lib.srhip_sgam_flash_fwd(p['q'], p['k'], p['v'], p['x'], p['gamma'], b.out('y', n, hw, 64), b.out('o', n, hw, 64), b.out('lse', n, hw),
                                 n, hw, 8, 64, _stream()), 'sgam_flash_fwd')
    torch.cuda.synchronize()
    need = lib.srhip_sgam_flash_bwd_workspace(n, hw)
    dg = None if dgamma == 'null' else b.out('dgamma', 1)
    if dgamma == 'accumulate':
        b.all['dgamma'].t.fill_(prior)
    _ok(lib.srhip_sgam_flash_bwd(p['dy'], p['q'], p['k'], p['v'], b.ptr('o'), b.ptr('lse'), p['gamma'], b.out('dq', n, hw, 8), b.out('dk', n, hw, 8),
                                 b.out('dv', n, hw, 64), dg, int(dgamma == 'accumulate'), b.workspace('ws', need), need, n, hw, 8, 64, _stream()),
        'sgam_flash_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'split'])
@pytest.mark.parametrize('family,n,hw', A.SGAM_CASES, ids=['%s-%dx%d' % c for c in A.SGAM_CASES])
def test_sgam_forward_and_every_gradient_at_the_tile_edges(family, n, hw, exact):
    """srhip_sgam_flash_fwd / _bwd, both arithmetics: y, o, lse, dq, dk, dv, dgamma of every image.
    Worst err / bar on the MI355X -- exact: random 0.33 (18 x 961: 0.35), sharp 0.60, ascending 0.73, descending 0.18;
    split: random 0.62 (18 x 961: 0.36), sharp 0.47, ascending 0.42, descending 0.46."""
    inp, ref, t32, emu, scales = _sgam_ref(family, n, hw)
    table = A.bars(ref, t32, 'sgam', family == 'random', None if exact else emu, scales)
    tab = A.Table('sgam %s %s %dx%d' % ('exact' if exact else 'split', family, n, hw))
    with _Arith(exact):
        first = _sgam_run(inp, n, hw)
        second = _sgam_run(inp, n, hw)
    outs = SGAM_OUT + ('dgamma',)
    tab.buffers(first, outs)
    tab.buffers(second, outs)
    tab.check_all({k: first.get(k) for k in outs}, ref, table, scales)
    tab.rerun(first, second, outs)
    tab.done()


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'split'])
def test_sgam_dgamma_written_accumulated_and_not_asked_for(exact):
    """accumulate_dgamma = 0 onto a NaN slot gives the sum; = 1 onto 0.5 gives 0.5 + that sum (one fp32 addition of the value the
    first form wrote: bit equality); dgamma = NULL; dq, dk, dv are the same bits in all three.
    Worst err / bar on the MI355X: 0.12 exact, 0.07 split."""
    n, hw = 2, A.SGAM_DGAMMA_HW
    inp, ref, t32, emu, scales = _sgam_ref('random', n, hw)
    table = A.bars(ref, t32, 'sgam', True, None if exact else emu, scales)
    tab = A.Table('sgam dgamma %s' % ('exact' if exact else 'split'))
    with _Arith(exact):
        runs = {m: _sgam_run(inp, n, hw, m) for m in ('write', 'accumulate', 'null')}
    for m, b in runs.items():
        tab.buffers(b, SGAM_OUT + (() if m == 'null' else ('dgamma',)))
        for k in SGAM_OUT:
            tab.same_bits('%s %s' % (m, k), b.get(k), runs['write'].get(k))
    total = runs['write'].get('dgamma')
    tab.check('dgamma', total, ref['dgamma'], table['dgamma'][0])
    tab.check('0.5 + dg', runs['accumulate'].get('dgamma'), 0.5 + ref['dgamma'], table['dgamma'][0] * float(ref['dgamma'].abs()) /
              float((0.5 + ref['dgamma']).abs()))
    tab.same_bits('0.5 + dg', runs['accumulate'].get('dgamma'), torch.tensor([0.5]) + total)
    tab.done()


# --------------------------------------------------------------------------------------------- #
# CGAM
# --------------------------------------------------------------------------------------------- #

CGAM_OUT = ('y', 'att', 'dx')


def _cgam_ref(n, hw, scale):
    def make():
        inp = A.cgam_inputs(n, hw, scale)
        return inp, A.cgam_eval(inp, F64), A.cgam_eval(inp, F32)
    return _once(('cgam', n, hw, scale), make)


def _cgam_run(inp, n, hw, dgamma='write', prior=0.5):
    lib, b = _lib(), A.Buffers(DEV)
    p = {k: b.put(k, inp[k]) for k in ('x', 'gamma', 'dy')}
    need = lib.srhip_cgam_workspace(n, hw)
    _ok(lib.srhip_cgam_fwd(p['x'], p['gamma'], b.out('y', n, hw, 64), b.out('att', n, 64, 64), b.workspace('ws_fwd', need), need, n, hw, 64,
                           _stream()), 'cgam_fwd')
    torch.cuda.synchronize()
    dg = None if dgamma == 'null' else b.out('dgamma', 1)
    if dgamma == 'accumulate':
        b.all['dgamma'].t.fill_(prior)
    _ok(lib.srhip_cgam_bwd(p['dy'], p['x'], b.ptr('att'), p['gamma'], b.out('dx', n, hw, 64), dg, int(dgamma == 'accumulate'),
                           b.workspace('ws_bwd', need), need, n, hw, 64, _stream()), 'cgam_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('n,hw,scale', A.CGAM_CASES, ids=['%dx%d-scale%.1f' % c for c in A.CGAM_CASES])
def test_cgam_forward_and_gradients_at_the_split_edges(n, hw, scale):
    """srhip_cgam_fwd / _bwd: y, the saved att, dx (residual path included), dgamma.  hw = 16 k +- 1 are the steps of the gram
    kernel's pixel loop, 128 k +- 1 its blocks.  Worst err / bar on the MI355X: 0.37 at scale 0.3, 0.33 at 2 x 729, scale 1."""
    inp, ref, t32 = _cgam_ref(n, hw, scale)
    table = A.bars(ref, t32, 'cgam')
    tab = A.Table('cgam %dx%d scale %.1f' % (n, hw, scale))
    first, second = _cgam_run(inp, n, hw), _cgam_run(inp, n, hw)
    outs = CGAM_OUT + ('dgamma',)
    tab.buffers(first, outs)
    tab.buffers(second, outs)
    tab.check_all({k: first.get(k) for k in outs}, ref, table)
    tab.rerun(first, second, outs)
    tab.done()


def test_cgam_dgamma_written_accumulated_and_not_asked_for():
    """The three dgamma forms of srhip_cgam_bwd; y, att and dx are the same bits in all three.  Worst err / bar on the MI355X: 0.07."""
    n, hw = 2, A.CGAM_DGAMMA_HW
    inp, ref, t32 = _cgam_ref(n, hw, 0.3)
    table = A.bars(ref, t32, 'cgam')
    tab = A.Table('cgam dgamma')
    runs = {m: _cgam_run(inp, n, hw, m) for m in ('write', 'accumulate', 'null')}
    for m, b in runs.items():
        tab.buffers(b, CGAM_OUT + (() if m == 'null' else ('dgamma',)))
        for k in CGAM_OUT:
            tab.same_bits('%s %s' % (m, k), b.get(k), runs['write'].get(k))
    total = runs['write'].get('dgamma')
    tab.check('dgamma', total, ref['dgamma'], table['dgamma'][0])
    tab.same_bits('0.5 + dg', runs['accumulate'].get('dgamma'), torch.tensor([0.5]) + total)
    tab.done()


# --------------------------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------------------------- #


def test_refusals_leave_every_buffer_untouched():
    """The list tests/test_attn_kernels_ref_cpu.py has passed without a device, again on real guarded buffers: every call returns its
    error code from the host-side checks, and nothing -- output, input stand-in, workspace or band -- is written."""
    from tests.pointwise_ref import Guarded
    lib = _lib()
    bufs = {k: Guarded((2 * 33 * 64,), DEV) for k in 'abcdefghijkl'}
    bufs['ws'] = Guarded((1 << 16,), DEV)
    p = {k: g.ptr() for k, g in bufs.items()}
    p['ws_bytes'] = 4 << 16
    bad = []
    for label, code, call in A.global_attn_refusals(lib, p):
        rc = call()
        if rc != code or not lib.srhip_last_error():
            bad.append((label, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(g.untouched() for g in bufs.values()), [k for k, g in bufs.items() if not g.untouched()]
