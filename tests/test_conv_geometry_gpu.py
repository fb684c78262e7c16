"""Every conv kernel family at its tile-edge geometries (the table: tests/conv_geometry_cases.py).

tests/test_conv_routes_gpu.py proves which arithmetic each route runs, at one shape per route.  This sweep holds the kernels to the
same emulation (tests/conv_emulation.py) and the same bars (TAU of the route table, imported) at the places a tiled implicit-GEMM
kernel goes wrong: fewer reduction chunks than pipeline stages, M tiles that span many samples, images smaller than the filter,
stride-2 data gradients with empty phases, every patch-tile class, channel tails on every N tile, the row-tap kernel's paired tails
and empty splits.  A correct kernel's error relative to |conv|(|x|, |w|) does not grow at an edge, so no bar is raised here.

Every case
  * runs through the entry points the route table uses (its _run); outputs the row hands over itself (row-stride and out= forms) lie
    in pointwise_ref.Guarded allocations or in a channel slice of a wider buffer: bands and pad columns intact, every body element written
    (the wrappers allocate the other outputs and every workspace themselves; the one direct call, the tail kernel's short workspace,
    brings its own Guarded workspace of exactly the bytes it names);
  * must lie within TAU[arith] * |conv|(|x|, |w|) + 2 * 2^-24 * |ref| of the emulation of the arithmetic its family runs;
  * must have been launched as the table says: srhip_conv2d_last_route names the family, and for the classes a tile shape defines
    (patch PH x PW class, weight-gradient tile, paired-tail remainder) that shape -- a heuristic that moves a case onto another kernel
    fails the case instead of leaving it testing nothing;
  * runs twice with equal bits, and equals bit for bit the other knob settings the code documents as identical (patch family and
    persistent walk at any grid against the LDS-DMA kernel, batched against per-phase stride-2 data gradients, scalar against
    vectorised split-K reduce).
Each case prints its record line(s), err / bound per output and the guard result with -s.

Largest err / bound per family, measured on the MI355X over the whole table (602 cases; the bars are the route table's TAU, 20 * 2^-24
for the 16-bit arithmetics and 32 * 2^-24 for fp32, and were not moved -- the route table's own worst are 0.21 and 0.22):
  k32 0.129 (M129, bf16x3)            regtile 0.179 (auto-M65, fp32)        dma 0.143 (epi29, fp32)          patch 0.150 (c128-pers, bf16x3)
  narrow 0.165 (c3-9x14, fp32)        dot 0.017 (M5-x16)                    legacy 0.124 (x3-k7-c65-7x5)     dil 0.205 (d2-5x7-wgrad, bf16x3)
  rowtap 0.211 (wo1-ho3-n3, bf16x3)   wdma 0.161 (reduce-generic, fp32)     tail1x1 0.118 (ws-1)             wreg 0.150 (xchan-7x5)
  wlegacy 0.071 (P17)
No case came near its bar: the error relative to |conv|(|x|, |w|) does not grow at a tile edge."""
import ctypes
import zlib

import pytest
import torch

from tests import conv_emulation as E
from tests import conv_geometry_cases as C
from tests.test_conv_routes_gpu import DEV, KNOB_DEFAULTS, TAU, U, _lib, _rand, _run

pytestmark = pytest.mark.gpu


def last_route(lib):
    """[{field: value}] of srhip_conv2d_last_route: one dict per kernel launch of the last conv call on this thread."""
    buf = ctypes.create_string_buffer(4096)
    n = lib.srhip_conv2d_last_route(buf, len(buf))
    recs = []
    for line in buf.value.decode().splitlines():
        fam, *fields = line.split()
        rec = {'fam': fam, 'line': line}
        for f in fields:
            k, v = f.split('=')
            rec[k] = v if k == 'tile' else int(v)
        recs.append(rec)
    return n, recs


def _matches(rec, want):
    return all(rec.get(k) == v for k, v in want.items())


def patch_class_holds(pc, rec, oh, ow):
    """Does the recorded PH x PW tile put an oh x ow output image into patch class pc?  (The class comes from the record: the test
    does not restate plan_patch.)"""
    ph, pw = (int(v) for v in rec['tile'].split('x'))
    th, tw = -(-oh // ph), -(-ow // pw)
    rr, rc = oh % ph != 0, ow % pw != 0
    return {'pw<16': pw < 16, '16<=pw<32': 16 <= pw < 32, '32<=pw<47': 32 <= pw < 47, 'ragged-row': rr and not rc, 'ragged-col': rc and not rr,
            'ragged-both': rr and rc, 'ph-clipped': ph == oh and ph < 128 // pw, 'one-tile': th == 1 and tw == 1, 'tiles_w>=3': tw >= 3}[pc]


def _set(lib, knobs):
    for key, v in knobs.items():
        assert lib.srhip_debug_set(key, v) == 0


def _reset(lib, knobs):
    for key in knobs:
        lib.srhip_debug_set(key, KNOB_DEFAULTS[key])


def _tail_short_workspace(row, g):
    """srhip_conv2d_wgrad of the attention tail's scaled 64 -> 64 1 x 1 conv with a workspace ONE BYTE short of what the workspace query
    names (the pixel-contraction kernel's need, larger than the split-K plan's): the register kernel must take the call.  The workspace is
    a Guarded allocation of exactly the query's bytes."""
    from sradsgan_amd import _hip
    from tests.pointwise_ref import Guarded
    lib = _lib()
    n, cin, h, w, cout, k, s, p = row['shape']
    x, dy = _rand((n, cin, h, w), g), _rand((n, cout, h, w), g)
    xr, xc = _rand((n, 1, h, w), g).abs() + 0.5, _rand((n, cin), g).abs() + 0.5
    need = lib.srhip_conv2d_wgrad_workspace(n, h, w, cin, cout, k, k, s, p)
    ws = Guarded(((need + 3) // 4,), DEV)
    dw, db = Guarded((cout, cin, k, k), DEV), Guarded((cout,), DEV)
    _hip.check(lib.srhip_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.ptr(), db.ptr(), xr.data_ptr(), xc.data_ptr(), 0, ws.ptr(), need - 1, n, h, w,
                                      cin, cout, k, k, s, p, cin, cout, None), 'conv2d_wgrad')
    xs = x * xr * xc.view(n, cin, 1, 1)

    def emu(a, with_abs=True):
        r, ar = E.conv_wgrad(xs, dy, (cout, cin, k, k), s, p, a, with_abs=with_abs)
        return r, (ar if ar is not None else torch.zeros_like(r))

    def emu_b(a, with_abs=True):
        return dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
    guards = [dict(guard=ws, body=None, pad=None, accumulate=True), dict(guard=dw, body=dw.t, pad=None, accumulate=False),
              dict(guard=db, body=db.t, pad=None, accumulate=False)]
    return [('dw', dw.t, emu, True), ('db', db.t, emu_b, False)], guards


def _once(row, rid, lib):
    """One run of the row from its seed: (results, guards, launches, records)."""
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(rid.encode()))
    if row.get('ws_short'):
        results, guards = _tail_short_workspace(row, g)
    else:
        guards = []
        results = _run(row, g, guards)
    n, recs = last_route(lib)
    return results, guards, n, recs


def check_case(row):
    from sradsgan_amd import ops
    lib = _lib()
    rid = row['id']
    nimg, cin, h, w, cout, k, s, p = row['shape']
    d = row.get('d', 1)
    try:
        _set(lib, row['knobs'])
        with ops.conv_math(row['mode']):
            if 'multi_ok' in row:
                assert lib.srhip_conv2d_wgrad_multi_ok(nimg, h, w, cin, cout, k, k, s, p) == row['multi_ok'], '%s: srhip_conv2d_wgrad_multi_ok' % rid
            results, guards, nl, recs = _once(row, rid, lib)
            again = _once(row, rid, lib)[0]
        torch.cuda.synchronize()
    finally:
        _reset(lib, row['knobs'])
    print('\n'.join('%s: %s' % (rid, r['line']) for r in recs))
    # ---- the route ----
    for want in (row['route'], row.get('route2')):
        if want:
            assert any(_matches(r, want) for r in recs), '%s: no launch matches %s: the case has left its kernel\n%s' % (
                rid, want, '\n'.join(r['line'] for r in recs))
    if 'nlaunch' in row:
        assert nl == row['nlaunch'], '%s: %d launches, expected %d' % (rid, nl, row['nlaunch'])
    if row.get('patch'):
        rec = next(r for r in recs if _matches(r, row['route']))
        oh, ow = (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1
        assert patch_class_holds(row['patch'], rec, oh, ow), '%s: tile %s on a %d x %d image is not in patch class %s' % (rid, rec['tile'], oh, ow, row['patch'])
    # ---- guards: bands, pad columns, every body element written ----
    for gd in guards:
        assert gd['guard'].bands_intact(), '%s: wrote outside its buffer' % rid
        if gd['pad'] is not None and gd['pad'].numel():
            assert bool(torch.isnan(gd['pad']).all()), '%s: wrote into the pad columns of its rows' % rid
        if gd['body'] is not None:
            assert not bool(torch.isnan(gd['body']).any()), '%s: left output elements unwritten (or wrote NaN)' % rid
    if guards:
        print('%s: %d guarded buffer(s) intact, bodies written' % (rid, len(guards)))
    # ---- accuracy against the emulation of the family's arithmetic; repeatability ----
    worst = 0.0
    for (name, got, emu, disc), (_, got2, _, _) in zip(results, again):
        expect = row['expect'] if disc else 'fp32'
        ref, absref = emu(expect)
        ratio = E.assert_conv_close(got, ref, absref, TAU[expect], what='%s %s (%s)' % (rid, name, expect))
        worst = max(worst, ratio)
        print('%s %s: %s err/bound %.3f at tau %g * 2^-24' % (rid, name, expect, ratio, TAU[expect] / U))
        assert torch.equal(got, got2), '%s %s: two runs differ' % (rid, name)
    # ---- documented bit-identities ----
    for other in row.get('same') or ():
        try:
            _set(lib, other)
            with ops.conv_math(row['mode']):
                alt, _, _, alt_recs = _once(row, rid, lib)
            torch.cuda.synchronize()
        finally:
            _reset(lib, other)
        assert [r['line'] for r in alt_recs] != [r['line'] for r in recs], '%s: knobs %s launched the same kernels: the identity compares nothing' % (rid, other)
        for (name, got, _, _), (_, got2, _, _) in zip(results, alt):
            assert torch.equal(got, got2), '%s %s: differs from the run with knobs %s, documented as bit-identical' % (rid, name, other)
        print('%s: bit-identical with knobs %s (%s)' % (rid, other, ', '.join(sorted({r['fam'] for r in alt_recs}))))
    return worst


@pytest.mark.parametrize('row', [pytest.param(r, id=r['id']) for r in C.ROWS])
def test_conv_geometry(row):
    worst = check_case(row)
    print('%s: family %s class %s worst err/bound %.3f' % (row['id'], row['fam'], row['cls'], worst))
