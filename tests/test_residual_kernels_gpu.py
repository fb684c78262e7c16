"""csrc/prelu.hip, csrc/ndsrgan.hip and the gamma residual of csrc/amssrn.hip -- one entry point at a time through the C ABI (ctypes)
at 255, 256 and 257 float4 items (one block, and one thread more or less), one item, and 131,076 items (one trip of the 512-block
stride loops of prelu_bwd / gamma_res_bwd plus a tail); rows dense and as a channel slice of a wider buffer; in place over either
operand; every slope of either sign; inputs holding 0, -0.0, +-inf, NaN and denormals; every NULL pattern the header allows.

Protocol of tests/test_cbam_gpu.py: every tensor lies in a pointwise_ref.Guarded allocation (64-element sentinel bands, outputs NaN;
of a wide buffer only the slice is ever written), the partial arrays are exactly srhip_prelu_parts() / srhip_gamma_parts() floats,
bands and inputs are intact after every call and every kernel runs twice with equal bits.  Every pass that is a fixed sequence of
fp32 operations is compared BIT FOR BIT with that sequence on the CPU (tests/leaf_kernels_ref.py), upsample_nearest_bwd with the
rows-then-columns sum; the slope and gamma sums with err / bound of tests/reduction_ref.py.  Every figure is printed before its assert."""
import pytest
import torch
import torch.nn.functional as F

from tests import leaf_kernels_ref as L
from tests.test_reductions_gpu import _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32
ROW_CASES = [(items, layout) for items in L.ITEM_COUNTS for layout in L.LAYOUTS]
SMALL_CASES = [(items, layout) for items in L.SMALL_ITEMS for layout in L.LAYOUTS]


def _geom(items, layout):
    rows, ch = L.ITEM_SHAPES[items]
    extra, off = L.LAYOUTS[layout]
    return rows, ch, ch + extra, off


def _scalar(b, name, v):
    return b.put(name, torch.tensor([v], dtype=F32))


def _reduce(b, nparts, accumulate=0, prior=None, name='da'):
    """srhip_prelu_slope_reduce of b's 'partials' into a guarded one-float slot (NaN, or `prior`)."""
    _ok(_lib().srhip_prelu_slope_reduce(b.ptr('partials'), nparts, b.out(name, 1, fill=prior), accumulate, _stream()), 'prelu_slope_reduce')
    torch.cuda.synchronize()
    return b.get(name)


# --------------------------------------------------------------------------------------------- #
# PReLU
# --------------------------------------------------------------------------------------------- #


def _run_prelu_fwd(z, a, geom, inplace):
    rows, ch, ld, off = geom
    b = L.Buffers(DEV)
    pz = b.put_wide('z', z, ld, off)
    py = pz if inplace else b.out_wide('y', rows, ch, ld, off)
    if inplace:
        b.src.pop('z')
    _ok(_lib().srhip_prelu_fwd(pz, ld, py, ld, _scalar(b, 'a', a), rows, ch, _stream()), 'prelu_fwd')
    torch.cuda.synchronize()
    return b


def _run_prelu_bwd(g, z, a, geom, alias):
    rows, ch, ld, off = geom
    lib, b = _lib(), L.Buffers(DEV)
    assert lib.srhip_prelu_parts() == L.PARTS
    pg, pz = b.put_wide('g', g, ld, off), b.put_wide('z', z, ld, off)
    pdz = {None: None, 'z': pz, 'g': pg}[alias] or b.out_wide('dz', rows, ch, ld, off)
    if alias:
        b.src.pop(alias)
    _ok(lib.srhip_prelu_bwd(pg, ld, pz, ld, pdz, ld, _scalar(b, 'a', a), b.out('partials', lib.srhip_prelu_parts()), rows, ch, _stream()),
        'prelu_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('items,layout', ROW_CASES, ids=['%d-%s' % c for c in ROW_CASES])
def test_prelu_forward_and_backward_every_slope_layout_and_alias(items, layout):
    """srhip_prelu_fwd, srhip_prelu_bwd (+ srhip_prelu_slope_reduce over its 512 partials): y and dz bit for bit, out of place and
    in place over z and over g, on the special-value rows and on clean ones; da of the clean rows against fp64.
    Worst err / bar of da on the MI355X: 0.02 (131,076 items: err 3.7e-8, fp32 torch 3.7e-8, bar 1.9e-6)."""
    geom = _geom(items, layout)
    rows, ch, ld, off = geom
    tab = L.table('prelu %d items %s' % (items, layout))
    for family, (g, z) in (('special', L.special_rows(rows, ch)), ('clean', L.clean_rows(rows, ch))):
        for a in L.PRELU_SLOPES:
            tag = '%s a %+.2f ' % (family, a)
            y_ref, dz_ref = L.prelu_fwd_ref32(z, a), L.prelu_bwd_ref32(g, z, a)
            for inplace in (False, True):
                first, second = (_run_prelu_fwd(z, a, geom, inplace) for _ in range(2))
                tab.guards(first, second)
                name = 'z' if inplace else 'y'
                tab.bits(tag + 'y%s' % (' in place' if inplace else ''), first.get(name), y_ref)
                tab.true(tag + 'rest of the wide buffer untouched', first.rest_untouched(name))
                tab.rerun(tag + 'y', first.get(name), second.get(name))
            base = None
            for alias in (None, 'z', 'g'):
                first, second = (_run_prelu_bwd(g, z, a, geom, alias) for _ in range(2))
                tab.guards(first, second)
                name = alias or 'dz'
                tab.bits(tag + 'dz over %s' % name, first.get(name), dz_ref)
                tab.true(tag + 'rest of the wide buffer untouched', first.rest_untouched(name))
                tab.rerun(tag + 'dz', first.get(name), second.get(name))
                tab.rerun(tag + 'partials', first.get('partials'), second.get('partials'))
                base = base or first
                tab.rerun(tag + 'partials == out of place', first.get('partials'), base.get('partials'))
            if family == 'clean':
                da = _reduce(base, L.PARTS)
                tab.guards(base)
                tab.check(tag + 'da', da, L.prelu_slope_eval(g, z, F64), L.prelu_slope_eval(g, z, F32))
    tab.done()


@pytest.mark.parametrize('nparts', L.REDUCE_NPARTS)
def test_slope_reduce_every_partial_count_written_and_accumulated(nparts):
    """srhip_prelu_slope_reduce on partials of its own: accumulate 0 overwrites a NaN; accumulate 1 adds, in one fp32 addition, the
    value accumulate 0 wrote."""
    parts = L.clean_rows(1, nparts, 9)[0].reshape(-1)
    tab = L.table('slope_reduce %d' % nparts)
    runs = []
    for _ in range(2):
        b = L.Buffers(DEV)
        b.put('partials', parts)
        runs.append((b, _reduce(b, nparts), _reduce(b, nparts, 1, 0.5, 'acc')))
        tab.guards(b)
    (_, da, acc), (_, da2, acc2) = runs
    tab.check('da', da, parts.double().sum().reshape(1), parts.sum().reshape(1))
    tab.bits('0.5 + da', acc, L.f32(0.5) + da)
    tab.rerun('da', da, da2)
    tab.rerun('acc', acc, acc2)
    tab.done()


# --------------------------------------------------------------------------------------------- #
# gamma residual
# --------------------------------------------------------------------------------------------- #


def _run_gamma(a, bb, g, count, with_db):
    lib, b = _lib(), L.Buffers(DEV)
    assert lib.srhip_gamma_parts() == L.PARTS
    pb, pgam = b.put('b', bb), _scalar(b, 'gamma', L.GAMMA)
    _ok(lib.srhip_gamma_res_fwd(b.put('a', a), pb, pgam, b.out('out', count), count, _stream()), 'gamma_res_fwd')
    db = b.out('db', count)
    _ok(lib.srhip_gamma_res_bwd(b.put('g', g), pb, pgam, db if with_db else None, b.out('partials', lib.srhip_gamma_parts()), count,
                                _stream()), 'gamma_res_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('items', L.ITEM_COUNTS)
def test_gamma_residual_forward_backward_with_and_without_db(items):
    """srhip_gamma_res_fwd, srhip_gamma_res_bwd: out and db bit for bit, dgamma (512 partials, then srhip_prelu_slope_reduce)
    against fp64; db = NULL writes nothing and gives the same partials.
    Worst err / bar of dgamma on the MI355X: 0.03 (255 items: err 5.7e-8, fp32 torch 3.7e-9, bar 1.9e-6)."""
    count = 4 * items
    a, bb, g = L.gamma_inputs(count)
    tab = L.table('gamma_res %d items' % items)
    first, second, nodb = _run_gamma(a, bb, g, count, True), _run_gamma(a, bb, g, count, True), _run_gamma(a, bb, g, count, False)
    tab.guards(first, second, nodb)
    tab.bits('out', first.get('out'), L.gamma_fwd_ref32(a, bb, L.GAMMA))
    tab.bits('db', first.get('db'), L.gamma_db_ref32(g, L.GAMMA))
    tab.true('db = NULL: untouched', nodb.all['db'].untouched())
    for k in ('out', 'db', 'partials'):
        tab.rerun(k, first.get(k), second.get(k))
    tab.rerun('partials == without db', first.get('partials'), nodb.get('partials'))
    dgamma = _reduce(first, L.PARTS, name='dgamma')
    tab.guards(first)
    tab.check('dgamma', dgamma, L.gamma_sum_eval(g, bb, F64), L.gamma_sum_eval(g, bb, F32))
    tab.done()


def test_prelu_and_gamma_chained_against_fp64_autograd():
    """out = a + gamma * prelu(z): prelu_fwd -> gamma_res_fwd, then gamma_res_bwd -> prelu_bwd with the two reduces, against torch
    fp64 autograd of F.prelu; the yardstick is the same autograd in fp32."""
    rows, ch, slope = 257, 12, 0.25
    gout, z = L.clean_rows(rows, ch, 3)
    a = L.clean_rows(rows, ch, 4)[1]
    lib, b, st = _lib(), L.Buffers(DEV), _stream()
    count = rows * ch
    pz, ps, pgam = b.put('z', z), _scalar(b, 'slope', slope), _scalar(b, 'gamma', L.GAMMA)
    _ok(lib.srhip_prelu_fwd(pz, ch, b.out('y', rows, ch), ch, ps, rows, ch, st), 'prelu_fwd')
    _ok(lib.srhip_gamma_res_fwd(b.put('a', a), b.ptr('y'), pgam, b.out('out', rows, ch), count, st), 'gamma_res_fwd')
    _ok(lib.srhip_gamma_res_bwd(b.put('gout', gout), b.ptr('y'), pgam, b.out('dy', rows, ch), b.out('gparts', L.PARTS), count, st), 'gamma_res_bwd')
    _ok(lib.srhip_prelu_slope_reduce(b.ptr('gparts'), L.PARTS, b.out('dgamma', 1), 0, st), 'prelu_slope_reduce')
    _ok(lib.srhip_prelu_bwd(b.ptr('dy'), ch, pz, ch, b.out('dz', rows, ch), ch, ps, b.out('partials', L.PARTS), rows, ch, st), 'prelu_bwd')
    _ok(lib.srhip_prelu_slope_reduce(b.ptr('partials'), L.PARTS, b.out('da', 1), 0, st), 'prelu_slope_reduce')
    torch.cuda.synchronize()
    res = {}
    for dtype in (F64, F32):
        zz, sl, gm = z.to(dtype).requires_grad_(), torch.tensor([slope], dtype=dtype, requires_grad=True), torch.tensor([L.GAMMA], dtype=dtype, requires_grad=True)
        out = a.to(dtype) + gm * F.prelu(zz, sl)
        out.backward(gout.to(dtype))
        res[dtype] = dict(out=out.detach(), dz=zz.grad, da=sl.grad, dgamma=gm.grad)
    tab = L.table('prelu + gamma chain')
    tab.guards(b)
    for k in ('out', 'dz', 'da', 'dgamma'):
        tab.check(k, b.get(k), res[F64][k], res[F32][k])
    tab.done()


# --------------------------------------------------------------------------------------------- #
# NDSRGAN's scaled residuals
# --------------------------------------------------------------------------------------------- #

ALPHA, BETA = 0.2, 0.3
FWD_PATTERNS = [(c, outs, alias) for c in (True, False) for outs in ('y', 'z', 'yz') for alias in (False,)] + [(True, 'yz', True), (False, 'z', True)]
# operand -> (ld - ch, first column): every operand has a row stride of its own
FWD_LAYOUT = {'r': (4, 4), 'c': (0, 0), 's': (8, 4), 'y': (12, 8), 'z': (4, 0)}


def _run_scaled_fwd(t, rows, ch, with_c, outs, r_is_s):
    lib, b = _lib(), L.Buffers(DEV)
    ld = {k: ch + e for k, (e, _) in FWD_LAYOUT.items()}
    p = {k: b.put_wide(k, t[k], ld[k], FWD_LAYOUT[k][1]) for k in ('r', 'c', 's')}
    if r_is_s:
        p['s'], ld['s'] = p['r'], ld['r']
    py = b.out_wide('y', rows, ch, ld['y'], FWD_LAYOUT['y'][1]) if 'y' in outs else None
    pz = b.out_wide('z', rows, ch, ld['z'], FWD_LAYOUT['z'][1]) if 'z' in outs else None
    _ok(lib.srhip_scaled_res_fwd(p['r'], ld['r'], p['c'] if with_c else None, ld['c'], p['s'] if 'z' in outs else None, ld['s'], ALPHA, BETA,
                                 py, ld['y'], pz, ld['z'], rows, ch, _stream()), 'scaled_res_fwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('items', L.SMALL_ITEMS)
def test_scaled_res_forward_every_null_pattern(items):
    """srhip_scaled_res_fwd: c NULL or not; y only, z only, both; r == s as ops calls it.  Bit for bit, in the reference's operation
    order y = r + c * alpha, z = s + beta * y."""
    rows, ch = L.ITEM_SHAPES[items]
    t = dict(zip(('r', 'c', 's'), L.rows_inputs(rows, ch, 3, 1)))
    tab = L.table('scaled_res_fwd %d items' % items)
    for with_c, outs, r_is_s in FWD_PATTERNS:
        tag = 'c %d out %s r==s %d ' % (with_c, outs, r_is_s)
        y_ref, z_ref = L.scaled_res_fwd_ref32(t['r'], t['c'] if with_c else None, t['r'] if r_is_s else t['s'], ALPHA, BETA)
        first, second = (_run_scaled_fwd(t, rows, ch, with_c, outs, r_is_s) for _ in range(2))
        tab.guards(first, second)
        for k, want in (('y', y_ref), ('z', z_ref)):
            if k in outs:
                tab.bits(tag + k, first.get(k), want)
                tab.true(tag + k + ': rest of the wide buffer untouched', first.rest_untouched(k))
                tab.rerun(tag + k, first.get(k), second.get(k))
    tab.done()


KA, KB, KC = 0.06, 0.3, 0.7
BWD_PATTERNS = [('dc only', True, False, False, 0)] + [('dr%s%s width ch+%s' % (' dc' if dc else '', ' e' if e else '', w), dc, True, e, w)
                                                       for dc in (False, True) for e in (False, True) for w in (0, 4, 12)]
LDR_EXTRA = 12


def _run_scaled_bwd(t, rows, ch, with_dc, with_dr, with_e, width):
    lib, b = _lib(), L.Buffers(DEV)
    pdz, pe = b.put_wide('dz', t['dz'], ch + 4, 4), b.put_wide('e', t['e'], ch, 0)
    pdc = b.out_wide('dc', rows, ch, ch + 8, 4) if with_dc else None
    pdr = b.out_wide('dr', rows, ch, ch + LDR_EXTRA, 0) if with_dr else None
    _ok(lib.srhip_scaled_res_bwd(pdz, ch + 4, pe if with_e else None, ch, KA, KB, KC, pdc, ch + 8, pdr, ch + LDR_EXTRA, width, rows, ch, _stream()),
        'scaled_res_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('items', L.SMALL_ITEMS)
def test_scaled_res_backward_zero_fill_and_the_columns_after_it(items):
    """srhip_scaled_res_bwd: dr NULL; dc NULL; e NULL and not; width = ch, ch + 4 and ldr = ch + 12: dr[0:ch] and dc bit for bit,
    dr[ch:width] is +0.0 and dr[width:ldr] is never written."""
    rows, ch = L.ITEM_SHAPES[items]
    t = dict(zip(('dz', 'e'), L.rows_inputs(rows, ch, 2, 2)))
    tab = L.table('scaled_res_bwd %d items' % items)
    for label, with_dc, with_dr, with_e, extra in BWD_PATTERNS:
        width = ch + extra
        dc_ref, dr_ref = L.scaled_res_bwd_ref32(t['dz'], t['e'] if with_e else None, KA, KB, KC)
        first, second = (_run_scaled_bwd(t, rows, ch, with_dc, with_dr, with_e, width) for _ in range(2))
        tab.guards(first, second)
        if with_dc:
            tab.bits(label + ': dc', first.get('dc'), dc_ref)
            tab.true(label + ': rest of dc untouched', first.rest_untouched('dc'))
            tab.rerun(label + ': dc', first.get('dc'), second.get('dc'))
        if with_dr:
            whole = first.all['dr'].t.detach().cpu()
            tab.bits(label + ': dr[0:ch]', first.get('dr'), dr_ref)
            tab.bits(label + ': dr[ch:width] == +0.0', whole[:, ch:width].contiguous(), torch.zeros(rows, extra))
            tab.true(label + ': dr[width:ldr] untouched', first.rest_untouched('dr', 0, width))
            tab.rerun(label + ': dr', first.all['dr'].t.detach().cpu(), second.all['dr'].t.detach().cpu())
    tab.done()


def _run_lrelu(dy, y, slope, geom, inplace):
    rows, ch, ld, off = geom
    b = L.Buffers(DEV)
    pdy, py = b.put_wide('dy', dy, ld, off), b.put_wide('y', y, ch + 4, 0)
    pdx = pdy if inplace else b.out_wide('dx', rows, ch, ld, off)
    if inplace:
        b.src.pop('dy')
    _ok(_lib().srhip_lrelu_bwd_strided(pdy, ld, py, ch + 4, pdx, ld, slope, rows, ch, _stream()), 'lrelu_bwd_strided')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('items,layout', SMALL_CASES, ids=['%d-%s' % c for c in SMALL_CASES])
def test_lrelu_bwd_strided_in_place_and_out_of_place(items, layout):
    """srhip_lrelu_bwd_strided: dx = y > 0 ? dy : dy * slope bit for bit; y (its own row stride) holds 0, -0.0, NaN, +-inf and
    denormals at both ends: zero, -0.0 and NaN take the slope."""
    geom = _geom(items, layout)
    dy, y = L.special_rows(geom[0], geom[1])
    tab = L.table('lrelu_bwd_strided %d items %s' % (items, layout))
    for slope in L.LRELU_SLOPES:
        want = L.lrelu_bwd_strided_ref32(dy, y, slope)
        for inplace in (False, True):
            first, second = (_run_lrelu(dy, y, slope, geom, inplace) for _ in range(2))
            tab.guards(first, second)
            name, tag = ('dy', 'slope %.1f in place ' % slope) if inplace else ('dx', 'slope %.1f ' % slope)
            tab.bits(tag + 'dx', first.get(name), want)
            tab.true(tag + 'rest of the wide buffer untouched', first.rest_untouched(name))
            tab.rerun(tag + 'dx', first.get(name), second.get(name))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# nearest upsampling
# --------------------------------------------------------------------------------------------- #

UP_CASES = [(r, c) + nhw for r in L.UP_R for c in L.UP_C for nhw in L.UP_NHW]


def _run_upsample(x, dy, r):
    n, h, w, c = x.shape
    lib, b = _lib(), L.Buffers(DEV)
    _ok(lib.srhip_upsample_nearest_fwd(b.put('x', x), b.out('y', n, h * r, w * r, c), n, h, w, c, r, _stream()), 'upsample_nearest_fwd')
    _ok(lib.srhip_upsample_nearest_bwd(b.put('dy', dy), b.out('dx', n, h, w, c), n, h, w, c, r, _stream()), 'upsample_nearest_bwd')
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize('r,c,n,h,w', UP_CASES, ids=['r%d-c%d-%dx%dx%d' % u for u in UP_CASES])
def test_upsample_nearest_copy_and_rows_then_columns_sum(r, c, n, h, w):
    """srhip_upsample_nearest_fwd: an exact copy of x[b, oy / r, ox / r]; _bwd: the r x r block summed rows then columns, bit for bit.
    Against fp64 the worst err / bar on the MI355X is 0.07 (r 3, c 8, 3 x 5 x 7: err 1.4e-7, fp32 torch 8.3e-8, bar 1.9e-6)."""
    gen = torch.Generator().manual_seed(r + 10 * c + 100 * n + h + w)
    x, dy = torch.randn(n, h, w, c, generator=gen), torch.randn(n, h * r, w * r, c, generator=gen) + 0.5
    tab = L.table('upsample r %d c %d %dx%dx%d' % (r, c, n, h, w))
    first, second = _run_upsample(x, dy, r), _run_upsample(x, dy, r)
    tab.guards(first, second)
    tab.bits('y', first.get('y'), L.upsample_nearest_ref(x, r))
    tab.bits('dx', first.get('dx'), L.emulate_upsample_nearest_bwd(dy, r))
    leaf = torch.zeros(n, h, w, c, requires_grad=True)
    L.upsample_nearest_ref(leaf, r).backward(dy)
    tab.check('dx vs fp64', first.get('dx'), L.upsample_nearest_bwd_ref(dy, r), leaf.grad)
    for k in ('y', 'dx'):
        tab.rerun(k, first.get(k), second.get(k))
    tab.done()


def test_ndsrgan_passes_chained_against_fp64_autograd():
    """up = upsample(lrelu(r + 0.2 c), 2): scaled_res_fwd -> (LeakyReLU on the CPU side of the test) -> upsample_nearest_fwd, then
    upsample_nearest_bwd -> lrelu_bwd_strided in place -> scaled_res_bwd, against torch fp64 autograd."""
    n, h, w, c, r = 2, 5, 7, 8, 2
    rows = n * h * w
    rr, cc = L.rows_inputs(rows, c, 2, 5)
    dup = torch.randn(n, h * r, w * r, c, generator=torch.Generator().manual_seed(12))
    lib, b, st = _lib(), L.Buffers(DEV), _stream()
    _ok(lib.srhip_scaled_res_fwd(b.put('r', rr), c, b.put('c', cc), c, None, c, 0.2, 0.0, b.out('y', rows, c), c, None, c, rows, c, st), 'scaled_res_fwd')
    torch.cuda.synchronize()
    act = F.leaky_relu(b.get('y'), 0.2)
    _ok(lib.srhip_upsample_nearest_fwd(b.put('act', act), b.out('up', n, h * r, w * r, c), n, h, w, c, r, st), 'upsample_nearest_fwd')
    _ok(lib.srhip_upsample_nearest_bwd(b.put('dup', dup), b.out('dact', rows, c), n, h, w, c, r, st), 'upsample_nearest_bwd')
    torch.cuda.synchronize()
    dact = b.get('dact')
    _ok(lib.srhip_lrelu_bwd_strided(b.ptr('dact'), c, b.ptr('act'), c, b.ptr('dact'), c, 0.2, rows, c, st), 'lrelu_bwd_strided')
    _ok(lib.srhip_scaled_res_bwd(b.ptr('dact'), c, None, c, 0.2, 1.0, 0.0, b.out('dc', rows, c), c, b.out('dr', rows, c), c, c, rows, c, st),
        'scaled_res_bwd')
    torch.cuda.synchronize()
    res = {}
    for dtype in (F64, F32):
        r_, c_ = rr.to(dtype).requires_grad_(), cc.to(dtype).requires_grad_()
        up = F.interpolate(F.leaky_relu(r_ + 0.2 * c_, 0.2).view(n, h, w, c).permute(0, 3, 1, 2), scale_factor=r, mode='nearest').permute(0, 2, 3, 1)
        up.backward(dup.to(dtype))
        res[dtype] = dict(up=up.detach(), dr=r_.grad, dc=c_.grad)
    tab = L.table('ndsrgan chain')
    tab.true('bands intact', not [k for k in b.broken() if 'input changed' not in k])
    tab.true('upsample_nearest_bwd wrote every element', bool(torch.isfinite(dact).all()))
    for k in ('up', 'dr', 'dc'):
        tab.check(k, b.get(k), res[F64][k], res[F32][k])
    tab.done()


# --------------------------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------------------------- #


def test_refusals_leave_every_buffer_untouched():
    """Among them the in-place calls with two row strides: rows would overwrite other rows' unread inputs."""
    L.run_refusals(_lib(), DEV, L.residual_refusals)
