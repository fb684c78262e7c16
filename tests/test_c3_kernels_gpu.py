"""The kernels that make one pass over a full-size 64-channel tensor with <= 4 channels on the other side, at the edges of their launch
geometry: the head conv 3 -> 64 (plain, record-writing, record-reading), the narrow convs 64 -> 3 / 64 -> 4 (forward and data gradient,
plain and with the head conv's record mask) and the two weight gradients 3 -> 64 (+ bias, record mask) and 64 -> 3.

Every route here runs exact fp32 in every arithmetic mode, so the bar is the fp32 bar of tests/test_conv_routes_gpu.py against the
float64 emulation of tests/conv_emulation.py (|got - ref| <= 32 * 2^-24 * |conv|(|x|, |w|) + 2 * 2^-24 * |ref|, element by element; the
bound grows with the reduction through the abs reference, which is how that file bars the weight gradients too).  Stock torch in fp32
on the CPU must pass the same bar for the same inputs: that is checked first, so a failure of the bar itself shows before the GPU runs.

Shapes are the smallest the routes take (>= 65536 pixels):
  head forward / weight gradients  (2, 181, 183): W odd, a multiple of neither 32 nor 128, N * H = 362 no multiple of the 4 rows a block
                                   of the head kernel walks; (131, 251, 2): the zero-padded staging row at both ends of every row, image
                                   boundaries inside most blocks; (1, 363, 183) for the weight gradients: N * H one more than a multiple
                                   of the two rows a split takes there;
  narrow convs                     (1, 250, 263): partial 16 x 16 patches on both edges."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_emulation as E

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TAU = 32 * E.U24
SLOPE = 0.2
HEAD_SHAPES = [(2, 181, 183), (131, 251, 2)]
WGRAD_SHAPES = HEAD_SHAPES + [(1, 363, 183)]
NARROW_SHAPE = (1, 250, 263)


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * 7 ** i for i, k in enumerate(key)) + 12345)


def _close(what, got, ref, absref):
    ratio = E.assert_conv_close(got, ref, absref, TAU, what=what)
    print('%s: err / bound %.3f' % (what, ratio))


def _record_halves(y):
    """The record the kernel must leave for its own output y [N, 64, H, W]: per pixel two int32 words, bit c of word c // 32 = y > 0."""
    yp = y.permute(0, 2, 3, 1).reshape(-1, 64).cpu()
    pos = (yp > 0).to(torch.int64)
    sh = torch.arange(32, dtype=torch.int64)
    halves = torch.stack([(pos[:, :32] << sh).sum(1), (pos[:, 32:] << sh).sum(1)], 1)
    return torch.where(halves >= (1 << 31), halves - (1 << 32), halves).to(torch.int32)


def _mask_of(bits, n, h, w):
    """bool [N, 64, H, W] on the CPU from a record."""
    words = bits.cpu().view(torch.int32).view(-1, 2).to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, dtype=torch.int64)
    m = torch.cat([(words[:, :1] >> sh) & 1, (words[:, 1:] >> sh) & 1], 1)
    return m.view(n, h, w, 64).permute(0, 3, 1, 2).bool()


# ---- head conv forward ---------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('cin', [3, 1])
@pytest.mark.parametrize('shape', HEAD_SHAPES)
def test_head_forward_plain_record_writing_record_reading(shape, cin):
    from sradsgan_amd import ops
    n, h, w = shape
    g = _gen(n, h, w, cin)
    x, ddx = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(64, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(64, generator=g) * 0.1
    ref, absref = E.conv_fwd(x, wt, 1, 1, 'fp32')
    ref_act, abs_act = E.epilogue(ref, absref, bias=b, slope=SLOPE)
    _close('stock fp32 conv', F.conv2d(x, wt, padding=1), ref, absref)
    _close('stock fp32 conv + bias + lrelu', F.leaky_relu(F.conv2d(x, wt, b, padding=1), SLOPE), ref_act, abs_act)

    assert ops.head_mask_ok((n, cin, h, w), (64, cin, 3, 3), 1, 1)
    xd, wd, bd = _cl(x), wt.to(DEV), b.to(DEV)
    _close('plain', ops.conv2d_fwd_raw(xd, wd, None, 1, 1), ref, absref)
    y = ops.conv2d_fwd_raw(xd, wd, bd, 1, 1, SLOPE)
    _close('bias + lrelu', y, ref_act, abs_act)
    y_rec, bits = ops.conv2d_fwd_head_mask_raw(xd, wd, bd, SLOPE)
    assert _same(y_rec, y)
    assert torch.equal(bits.cpu().view(torch.int32).view(-1, 2), _record_halves(y_rec))
    # record-reading: mask * conv(ddx, w), the mask from the record just written
    mask = _mask_of(bits, n, h, w)
    assert bool(mask.any()) and not bool(mask.all())
    r2, a2 = E.conv_fwd(ddx, wt, 1, 1, 'fp32')
    r2, a2 = E.epilogue(r2, a2, actmask=mask.double() * 2 - 1, mask_slope=SLOPE)
    _close('record-reading', ops.conv2d_fwd_head_mask_raw(_cl(ddx), wd, None, SLOPE, bits=bits), r2, a2)


@pytest.mark.parametrize('cin', [3, 1])
@pytest.mark.parametrize('shape', HEAD_SHAPES)
def test_head_record_of_nan_and_zero_outputs(shape, cin):
    """The record against y > 0 of the kernel's own output where y holds NaN (one NaN input pixel) and exact zeros (channel 5: zero
    weights and bias): both give bit 0.  In the last image, so the NaN sits in a block that ends short of its 4 rows."""
    from sradsgan_amd import ops
    n, h, w = shape
    g = _gen(n, h, w, cin, 1)
    x = torch.randn(n, cin, h, w, generator=g)
    x[n - 1, cin - 1, h - 1, w - 2] = float('nan')
    wt = torch.randn(64, cin, 3, 3, generator=g) * 0.3
    b = torch.randn(64, generator=g) * 0.1
    wt[5] = 0.0
    b[5] = 0.0
    b[9] = 0.0
    y, bits = ops.conv2d_fwd_head_mask_raw(_cl(x), wt.to(DEV), b.to(DEV), SLOPE)
    yc = y.cpu()
    assert bool(torch.isnan(yc).any()) and bool((yc[:, 5] == 0).any()) and bool((yc > 0).any()) and bool((yc < 0).any())
    assert _same(y, ops.conv2d_fwd_raw(_cl(x), wt.to(DEV), b.to(DEV), 1, 1, SLOPE))
    assert torch.equal(bits.cpu().view(torch.int32).view(-1, 2), _record_halves(y))


# ---- narrow convs: 64 -> 3 / 64 -> 4 forward and data gradient ------------------------------------------------------------- #
@pytest.mark.parametrize('c,k', [(64, 3), (64, 4), (16, 3), (32, 3)])
def test_narrow_forward_and_data_gradient(c, k):
    from sradsgan_amd import ops
    n, h, w = NARROW_SHAPE
    g = _gen(c, k, 2)
    x = torch.randn(n, c, h, w, generator=g)
    wf = torch.randn(k, c, 3, 3, generator=g) * (9 * c) ** -0.5          # forward c -> k
    b = torch.randn(k, generator=g) * 0.1
    wg = torch.randn(c, k, 3, 3, generator=g) * (9 * c) ** -0.5          # the conv k -> c whose data gradient is c -> k
    ref, absref = E.epilogue(*E.conv_fwd(x, wf, 1, 1, 'fp32'), bias=b)
    _close('stock fp32 forward', F.conv2d(x, wf, b, padding=1), ref, absref)
    _close('forward %d -> %d' % (c, k), ops.conv2d_fwd_raw(_cl(x), wf.to(DEV), b.to(DEV), 1, 1), ref, absref)
    ref, absref = E.conv_dgrad(x, wg, (n, k, h, w), 1, 1, 'fp32')
    _close('stock fp32 data gradient', F.conv_transpose2d(x, wg, padding=1), ref, absref)
    _close('data gradient %d -> %d' % (c, k), ops.conv2d_dgrad_raw(_cl(x), wg.to(DEV), (n, k, h, w), 1, 1), ref, absref)


@pytest.mark.parametrize('slope', [SLOPE, 0.0])
def test_masked_data_gradient_is_the_plain_kernel_on_the_masked_gradient(slope):
    """Bit for bit.  dy holds a NaN where the record masks it out: with slope 0 it stays NaN * 0 = NaN and reaches dx, as the plain
    kernel on the explicitly masked gradient gives it."""
    from sradsgan_amd import ops
    n, h, w = NARROW_SHAPE
    g = _gen(h, w, 3)
    x = torch.randn(n, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(64, generator=g) * 0.1
    dy = torch.randn(n, 64, h, w, generator=g)
    _, bits = ops.conv2d_fwd_head_mask_raw(_cl(x), wt.to(DEV), b.to(DEV), SLOPE)
    mask = _mask_of(bits, n, h, w)
    off = (~mask[0, 7]).nonzero()[0]                                     # a masked-out element of channel 7
    dy[0, 7, off[0], off[1]] = float('nan')
    dyd, md = _cl(dy), _cl(mask)
    masked = torch.where(md, dyd, dyd * slope).contiguous(memory_format=torch.channels_last)
    want = ops.conv2d_dgrad_raw(masked, wt.to(DEV), (n, 3, h, w), 1, 1)
    got = ops.conv2d_dgrad_head_mask_raw(dyd, wt.to(DEV), (n, 3, h, w), bits, slope)
    assert _same(got, want)
    assert bool(torch.isnan(got).any()) and not bool(torch.isnan(got).all())


# ---- weight gradients ------------------------------------------------------------------------------------------------------ #
def _colsum(dy):
    return dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))


@pytest.mark.parametrize('shape', WGRAD_SHAPES)
def test_head_weight_and_bias_gradient_plain_and_record_masked(shape):
    from sradsgan_amd import ops
    n, h, w = shape
    g = _gen(n, h, w, 4)
    x, dy = torch.randn(n, 3, h, w, generator=g), torch.randn(n, 64, h, w, generator=g)
    wt = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(64, generator=g) * 0.1
    ref, absref = E.conv_wgrad(x, dy, (64, 3, 3, 3), 1, 1, 'fp32')
    _close('stock fp32 weight gradient', torch.nn.grad.conv2d_weight(x, (64, 3, 3, 3), dy, padding=1), ref, absref)
    _close('stock fp32 bias gradient', dy.sum((0, 2, 3)), *_colsum(dy))
    xd, dyd = _cl(x), _cl(dy)
    dw, db = ops.conv2d_wgrad_raw(xd, dyd, (64, 3, 3, 3), 1, 1, True)
    _close('dw 3 -> 64', dw, ref, absref)
    _close('db', db, *_colsum(dy))
    _, bits = ops.conv2d_fwd_head_mask_raw(xd, wt.to(DEV), b.to(DEV), SLOPE)
    masked = torch.where(_mask_of(bits, n, h, w), dy, dy * SLOPE)          # one fp32 product, as the kernel applies it
    dw, db = ops.conv2d_wgrad_raw(xd, dyd, (64, 3, 3, 3), 1, 1, True, head_bits=(bits, SLOPE))
    _close('dw 3 -> 64, record mask', dw, *E.conv_wgrad(x, masked, (64, 3, 3, 3), 1, 1, 'fp32'))
    _close('db, record mask', db, *_colsum(masked))


@pytest.mark.parametrize('shape', WGRAD_SHAPES)
def test_tail_weight_and_bias_gradient(shape):
    from sradsgan_amd import ops
    n, h, w = shape
    g = _gen(n, h, w, 5)
    x, dy = torch.randn(n, 64, h, w, generator=g), torch.randn(n, 3, h, w, generator=g)
    ref, absref = E.conv_wgrad(x, dy, (3, 64, 3, 3), 1, 1, 'fp32')
    _close('stock fp32 weight gradient', torch.nn.grad.conv2d_weight(x, (3, 64, 3, 3), dy, padding=1), ref, absref)
    dw, db = ops.conv2d_wgrad_raw(_cl(x), _cl(dy), (3, 64, 3, 3), 1, 1, True)
    _close('dw 64 -> 3', dw, ref, absref)
    _close('db', db, *_colsum(dy))
