"""csrc/elementwise.hip (column sums excepted: tests/test_reductions_gpu.py) -- the four 2x2 max-pool kernels and their records,
pixel shuffle forward / backward in block form (r = 2, 3) and general form (every other r), the LeakyReLU backward in its plain, tail
and sign-bit forms, cat / split -- through the C ABI (ctypes) against the references of tests/pointwise_ref.py.

None of these kernels does more than one rounding, so every comparison is bit equality with the reference evaluated in fp32.
Outputs start as NaN (integers -7, mask bytes 0xA5) inside a larger allocation with a 64-element sentinel band on both sides, which
must be unchanged afterwards (tests/test_reductions_gpu.py's protocol)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_ref as P
from tests.test_reductions_gpu import _Table, _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _G(*shape, dtype=torch.float32, misalign=0):
    return P.Guarded(shape, DEV, dtype, misalign)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _exact(tab, name, got, ref):
    tab.same_bits(name, _bits(got), _bits(ref))


def _bands(tab, **outs):
    for name, g in outs.items():
        if not g.bands_intact():
            tab.bad.append((name, 'sentinel band overwritten'))


# --------------------------------------------------------------------------------------------- #
# max pool 2x2
# --------------------------------------------------------------------------------------------- #


def _decode_records(rec, n, ho, wo, c):
    """srhip_maxpool2x2_fwd_idx's records as the header documents them: one 16-bit record per 4 channels of an output pixel, channel
    k of the quad in bits 3 k .. 3 k + 2 -- arg-max position (2 bits) and `maximum > 0` (1 bit); bits 12 .. 15 are zero.  Returns
    pos, positive [n][ho][wo][c] and the spare bits."""
    r = rec.cpu().to(torch.int32) & 0xFFFF
    f = torch.stack([(r >> (3 * k)) & 7 for k in range(4)], 1).view(n, ho, wo, c)
    return f & 3, f >> 2, r >> 12


@pytest.mark.parametrize('family', P.POOL_FAMILIES)
@pytest.mark.parametrize('shape', P.POOL_SHAPES, ids=[P.shape_id(s) for s in P.POOL_SHAPES])
def test_max_pool_forward_records_and_both_backwards(shape, family):
    """srhip_maxpool2x2_fwd / _fwd_idx: y equal to the reference and to F.max_pool2d; the records decoded here (today only the
    consumer kernel reads them) hold the reference's first-maximum position and sign bit.  srhip_maxpool2x2_bwd / _bwd_idx with
    relu_input 0 and 1: dx equal to the reference; on a ReLU output also to fp32 CPU autograd of max_pool2d(relu(z))."""
    n, c, h, w = shape
    ho, wo = h // 2, w // 2
    x, dy, z = P.pool_inputs(family, shape)
    ref_y, ref_pos = P.maxpool2x2_ref(x)
    lib = _lib()
    xd, dyd = x.to(DEV), dy.to(DEV)
    tab = _Table('maxpool2x2 %s %s' % (P.shape_id(shape), family))
    y = _G(n, ho, wo, c)
    _ok(lib.srhip_maxpool2x2_fwd(xd.data_ptr(), y.ptr(), n, h, w, c, _stream()), 'maxpool2x2_fwd')
    y2, rec = _G(n, ho, wo, c), _G(n * ho * wo * (c // 4), dtype=torch.int16)
    _ok(lib.srhip_maxpool2x2_fwd_idx(xd.data_ptr(), y2.ptr(), rec.ptr(), n, h, w, c, _stream()), 'maxpool2x2_fwd_idx')
    torch.cuda.synchronize()
    _bands(tab, y=y, y_idx=y2, rec=rec)
    aten = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    for name, got in (('fwd', y.t), ('fwd_idx', y2.t)):
        _exact(tab, name + ' y vs reference', got, ref_y)
        _exact(tab, name + ' y vs F.max_pool2d', got, aten)
    pos, positive, spare = _decode_records(rec.t, n, ho, wo, c)
    tab.same_bits('record position', pos, ref_pos.to(torch.int32))
    tab.same_bits('record sign bit', positive, (ref_y > 0).to(torch.int32))
    tab.same_bits('record spare bits', spare, torch.zeros_like(spare))
    for relu in (0, 1):
        ref_dx = P.maxpool2x2_bwd_ref(dy, x, relu)
        dx, dxi = _G(n, h, w, c), _G(n, h, w, c)
        _ok(lib.srhip_maxpool2x2_bwd(dyd.data_ptr(), xd.data_ptr(), dx.ptr(), n, h, w, c, relu, _stream()), 'maxpool2x2_bwd')
        _ok(lib.srhip_maxpool2x2_bwd_idx(dyd.data_ptr(), rec.ptr(), dxi.ptr(), n, h, w, c, relu, _stream()), 'maxpool2x2_bwd_idx')
        torch.cuda.synchronize()
        _bands(tab, dx=dx, dx_idx=dxi)
        _exact(tab, 'bwd relu_input %d' % relu, dx.t, ref_dx)
        _exact(tab, 'bwd_idx relu_input %d' % relu, dxi.t, ref_dx)
    if z is not None:
        zr = z.permute(0, 3, 1, 2).requires_grad_()
        (dz,) = torch.autograd.grad(F.max_pool2d(F.relu(zr), 2, 2), zr, dy.permute(0, 3, 1, 2))
        tab.same_bits('bwd relu_input 1 vs fp32 autograd of max_pool2d(relu(z))', dx.t.cpu(), dz.permute(0, 2, 3, 1).contiguous())
    tab.done()


# --------------------------------------------------------------------------------------------- #
# pixel shuffle (+ LeakyReLU)
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('r', P.SHUFFLE_R)
def test_pixel_shuffle_forward_and_backward_are_exact(r):
    """r = 2, 3: the block kernels; r = 4: the general kernels, which the ABI runs for every other r.  Through the C ABI and through
    ops.pixel_shuffle_act, with and without the fused LeakyReLU, on random inputs with exact zeros and on inputs that are their own
    signed flat index; the backward takes a dout that is not the forward's input and an `out` with zeros and negatives (a zero takes
    the slope).  3x5x7 with 12 output channels is 315 threads in block form: a block boundary and a ragged tail.  Every pointer is
    16-byte aligned: the general kernels make 16-byte accesses on out / din."""
    from sradsgan_amd import ops
    lib = _lib()
    tab = _Table('pixel shuffle r %d' % r)
    for n, h, w in P.SHUFFLE_NHW:
        for cout in P.SHUFFLE_COUT:
            for integer in (False, True):
                x, dout = P.shuffle_inputs(n, h, w, cout, r, integer)
                xd, dd = x.to(DEV), dout.to(DEV)
                for slope in P.SHUFFLE_ACTS:
                    case = '%dx%dx%d c %d %s slope %s' % (n, h, w, cout, 'int' if integer else 'rnd', slope)
                    ref = P.pixel_shuffle_ref(x, r, slope)
                    aten = F.pixel_shuffle(x.permute(0, 3, 1, 2), r)
                    aten = (aten if slope is None else F.leaky_relu(aten, slope)).permute(0, 2, 3, 1)
                    act, sl = int(slope is not None), float(slope or 0.0)
                    out = _G(n, h * r, w * r, cout)
                    _ok(lib.srhip_pixel_shuffle_fwd(xd.data_ptr(), out.ptr(), n, h, w, cout, r, sl, act, _stream()), 'pixel_shuffle_fwd')
                    torch.cuda.synchronize()
                    _bands(tab, out=out)
                    _exact(tab, case + ' fwd', out.t, ref)
                    _exact(tab, case + ' fwd vs ATen', out.t, aten)
                    ref_din = P.pixel_shuffle_bwd_ref(dout, ref, r, slope)
                    din = _G(n, h, w, cout * r * r)
                    outd = out.t.contiguous()
                    _ok(lib.srhip_pixel_shuffle_bwd(dd.data_ptr(), outd.data_ptr() if act else None, din.ptr(), n, h, w, cout, r, sl, act, _stream()),
                        'pixel_shuffle_bwd')
                    torch.cuda.synchronize()
                    _bands(tab, din=din)
                    _exact(tab, case + ' bwd', din.t, ref_din)
                    # the same through the autograd op (NCHW view of the NHWC tensors)
                    xs = xd.permute(0, 3, 1, 2).requires_grad_()
                    o = ops.pixel_shuffle_act(xs, r, slope)
                    (g,) = torch.autograd.grad(o, xs, dd.permute(0, 3, 1, 2))
                    _exact(tab, case + ' ops fwd', o.detach().permute(0, 2, 3, 1), ref)
                    _exact(tab, case + ' ops bwd', g.permute(0, 2, 3, 1), ref_din)
    if tab.bad:
        print(tab.bad[:10])
    tab.done()


# --------------------------------------------------------------------------------------------- #
# LeakyReLU backward
# --------------------------------------------------------------------------------------------- #

_lrelu_cache = {}


def _lrelu_case(count):
    if count not in _lrelu_cache:
        _lrelu_cache[count] = P.lrelu_inputs(count)
    return _lrelu_cache[count]


@pytest.mark.parametrize('count', P.LRELU_COUNTS)
def test_lrelu_backward_vector_body_tail_and_grid_stride(count):
    """srhip_lrelu_bwd, bit for bit: counts below one float4, with a scalar tail, one float4 past the 4096-block cap (the grid-stride
    trip) and that plus a tail; y holds 0, -0.0, NaN, +-inf and denormals at the front and in the tail; slopes 0.2, 0 and 1."""
    dy, y = _lrelu_case(count)
    dyd, yd = dy.to(DEV), y.to(DEV)
    tab = _Table('lrelu_bwd count %d' % count)
    for slope in P.LRELU_SLOPES:
        dx = _G(count)
        _ok(_lib().srhip_lrelu_bwd(dyd.data_ptr(), yd.data_ptr(), dx.ptr(), count, slope, _stream()), 'lrelu_bwd')
        torch.cuda.synchronize()
        _bands(tab, dx=dx)
        _exact(tab, 'slope %s' % slope, dx.t, P.lrelu_bwd_ref(dy, y, slope))
    tab.done()


@pytest.mark.parametrize('count', [105, 1023, 1024])
def test_lrelu_backward_from_a_base_4_bytes_into_an_allocation(count):
    """No 16-byte loads are possible, so the whole count goes through the scalar tail kernel (count 1024 too, which has no tail of
    its own).  Also count = 0: OK, nothing written."""
    dy, y = _lrelu_case(count)
    lib = _lib()
    tab = _Table('lrelu_bwd misaligned count %d' % count)
    for which in ('dx', 'all'):
        gdy, gy, dx = _G(count, misalign=int(which == 'all')), _G(count, misalign=int(which == 'all')), _G(count, misalign=1)
        gdy.t.copy_(dy)
        gy.t.copy_(y)
        assert dx.ptr() % 16 == 4 and (which == 'dx' or gdy.ptr() % 16 == 4)
        _ok(lib.srhip_lrelu_bwd(gdy.ptr(), gy.ptr(), dx.ptr(), count, 0.2, _stream()), 'lrelu_bwd')
        torch.cuda.synchronize()
        _bands(tab, dx=dx, dy=gdy, y=gy)
        _exact(tab, 'misaligned ' + which, dx.t, P.lrelu_bwd_ref(dy, y, 0.2))
    dx = _G(8)
    _ok(lib.srhip_lrelu_bwd(gdy.ptr(), gy.ptr(), dx.ptr(), 0, 0.2, _stream()), 'lrelu_bwd')
    torch.cuda.synchronize()
    assert dx.untouched()
    tab.done()


@pytest.mark.parametrize('n4', P.LRELU_BITS_N4)
def test_lrelu_backward_with_sign_bits_against_the_reference(n4):
    """srhip_lrelu_bwd_bits: mode 1 (reads y, writes the mask) and then mode 2 (reads the mask), each against the REFERENCE; the mask is
    exactly srhip_lrelu_mask_bytes(count) bytes in the documented layout (bits past the count zero), with intact bands around it.
    n4 = 63 / 64 / 65: a partial wave chunk, a whole one, one float4 into the next; 1,048,577: the grid-stride trip."""
    count = 4 * n4
    dy, y = _lrelu_case(count)
    dyd, yd = dy.to(DEV), y.to(DEV)
    lib = _lib()
    nbytes = lib.srhip_lrelu_mask_bytes(count)
    assert nbytes == (n4 + 63) // 64 * 32
    tab = _Table('lrelu_bwd_bits n4 %d' % n4)
    for slope in (0.2, 0.0):
        ref = P.lrelu_bwd_ref(dy, y, slope)
        mask, dx1, dx2 = _G(nbytes, dtype=torch.uint8), _G(count), _G(count)
        _ok(lib.srhip_lrelu_bwd_bits(dyd.data_ptr(), yd.data_ptr(), mask.ptr(), dx1.ptr(), count, slope, _stream()), 'lrelu_bwd_bits')
        _ok(lib.srhip_lrelu_bwd_bits(dyd.data_ptr(), None, mask.ptr(), dx2.ptr(), count, slope, _stream()), 'lrelu_bwd_bits')
        torch.cuda.synchronize()
        _bands(tab, mask=mask, dx1=dx1, dx2=dx2)
        _exact(tab, 'slope %s from y' % slope, dx1.t, ref)
        _exact(tab, 'slope %s from the mask' % slope, dx2.t, ref)
        tab.same_bits('mask bytes', mask.t.cpu(), P.lrelu_mask_ref(y))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# cat / split
# --------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize('case', sorted(P.CAT_CASES))
def test_cat_and_split_channels_are_exact(case):
    rows, chans = P.CAT_CASES[case]
    ts = P.cat_inputs(rows, chans)
    wide = P.cat_ref(ts)
    lib = _lib()
    k = len(ts)
    tab = _Table('cat/split ' + case)
    td = [t.to(DEV) for t in ts]
    ctab = (ctypes.c_int * k)(*chans)
    out = _G(rows, sum(chans))
    _ok(lib.srhip_cat_channels((ctypes.c_void_p * k)(*[t.data_ptr() for t in td]), ctab, k, out.ptr(), rows, _stream()), 'cat_channels')
    torch.cuda.synchronize()
    _bands(tab, out=out)
    _exact(tab, 'cat', out.t, wide)
    parts = [_G(rows, c) for c in chans]
    _ok(lib.srhip_split_channels(wide.to(DEV).data_ptr(), ctab, k, (ctypes.c_void_p * k)(*[g.ptr() for g in parts]), rows, _stream()),
        'split_channels')
    torch.cuda.synchronize()
    _bands(tab, **{'part%d' % i: g for i, g in enumerate(parts)})
    for i, (g, t) in enumerate(zip(parts, P.split_ref(wide, chans))):
        _exact(tab, 'split %d' % i, g.t, t)
    tab.done()


def test_refusals_leave_every_buffer_untouched():
    """Odd h or w, c % 4 != 0, c < 4, null tensors, cat / split of 1 or 9 tensors or of 6 channels, a sign-bit call with count % 4 != 0
    or a tensor 4 bytes off: SRHIP_ERR_ARG from the host-side checks, nothing written."""
    lib = _lib()
    bufs = {k: _G(256, dtype=torch.int16 if k == 'rec' else (torch.uint8 if k == 'mask' else torch.float32)) for k in ('x', 'y', 'rec', 'out', 'mask')}
    bad = []
    for label, call in P.elementwise_refusals(lib, {k: g.ptr() for k, g in bufs.items()}):
        rc = call()
        if rc == 0 or not lib.srhip_last_error():
            bad.append((label, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(g.untouched() for g in bufs.values()), [k for k, g in bufs.items() if not g.untouched()]
