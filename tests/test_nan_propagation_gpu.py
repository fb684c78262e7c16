"""The NaN policy of csrc/common.h -- a NaN activation must surface; max and ReLU behave like ATen's -- held at the sites that take
a maximum with zero or over a window: the 2x2 max pools (elementwise.hip), the LPIPS stem's ReLU (lpips.hip), the ReLU of the
classifier's dense layers (classify.hip) and of the channel-attention MLPs (ca.hip, hat.hip).  One NaN goes in, the expected NaN set
comes out, everything else stays finite and equal to the stock-torch operation on the CPU (fp64 reference, the bar of
tests/test_reductions_gpu.py set by fp32 torch)."""
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_ref as P
from tests.test_reductions_gpu import _Table, _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
NAN = float('nan')


def _rnd(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def _check_finite_part(tab, name, got, ref64, t32, nan_mask):
    """NaN exactly on nan_mask (as in stock torch, t32), the rest under the bar."""
    got = got.detach().cpu()
    tab.same_bits(name + ': NaN set', torch.isnan(got), nan_mask)
    tab.same_bits(name + ': NaN set of stock torch', torch.isnan(t32), nan_mask)
    keep = ~nan_mask
    tab.check(name + ': the rest', got[keep], ref64[keep], t32[keep])


@pytest.mark.parametrize('position', [0, 1, 2, 3])
def test_max_pool_2x2_returns_nan_for_a_window_that_holds_one(position):
    """A NaN at each of the four window positions in turn, next to finite neighbours: that window's output is NaN, every other
    output equals F.max_pool2d, for srhip_maxpool2x2_fwd and _fwd_idx.  What the backward does on such a window is unspecified;
    the x-reading and the record-reading backward must still agree bit for bit there."""
    n, c, h, w = 2, 8, 4, 6
    x, dy, _ = P.pool_inputs('random', (n, c, h, w))
    i, j = divmod(position, 2)
    spots = [(0, 0 + i, 2 + j, 5), (1, 2 + i, 4 + j, 0)]               # one window that is not the first, one in the last row and column
    for b, yy, xx, ch in spots:
        x[b, yy, xx, ch] = NAN
    aten = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    want = torch.zeros(n, h // 2, w // 2, c, dtype=torch.bool)
    want[0, 0, 1, 5] = want[1, 1, 2, 0] = True
    assert torch.equal(torch.isnan(aten), want) and torch.equal(torch.isnan(P.maxpool2x2_ref(x)[0]), want)
    lib = _lib()
    xd, dyd = x.to(DEV), dy.to(DEV)
    tab = _Table('maxpool2x2 NaN at window position %d' % position)
    y, y2 = P.Guarded((n, h // 2, w // 2, c), DEV), P.Guarded((n, h // 2, w // 2, c), DEV)
    rec = P.Guarded((n * (h // 2) * (w // 2) * (c // 4),), DEV, torch.int16)
    _ok(lib.srhip_maxpool2x2_fwd(xd.data_ptr(), y.ptr(), n, h, w, c, _stream()), 'maxpool2x2_fwd')
    _ok(lib.srhip_maxpool2x2_fwd_idx(xd.data_ptr(), y2.ptr(), rec.ptr(), n, h, w, c, _stream()), 'maxpool2x2_fwd_idx')
    torch.cuda.synchronize()
    for name, g in (('fwd', y), ('fwd_idx', y2)):
        got = g.t.cpu()
        tab.same_bits(name + ': NaN set', torch.isnan(got), want)
        tab.same_bits(name + ': every other output', got[~want], aten[~want])
        if not g.bands_intact():
            tab.bad.append((name, 'sentinel band overwritten'))
    for relu in (0, 1):
        dx, dxi = P.Guarded((n, h, w, c), DEV), P.Guarded((n, h, w, c), DEV)
        _ok(lib.srhip_maxpool2x2_bwd(dyd.data_ptr(), xd.data_ptr(), dx.ptr(), n, h, w, c, relu, _stream()), 'maxpool2x2_bwd')
        _ok(lib.srhip_maxpool2x2_bwd_idx(dyd.data_ptr(), rec.ptr(), dxi.ptr(), n, h, w, c, relu, _stream()), 'maxpool2x2_bwd_idx')
        torch.cuda.synchronize()
        tab.same_bits('bwd and bwd_idx agree, relu_input %d' % relu, dx.t.cpu().view(torch.int32), dxi.t.cpu().view(torch.int32))
    tab.done()


def test_lpips_stem_spreads_a_nan_pixel_over_its_receptive_field():
    """ops.lpips_stem_raw (scaling layer + 11x11 stride-4 conv + ReLU): every output pixel whose receptive field covers the NaN
    input pixel is NaN in all 64 channels, every other output is finite -- what F.relu(F.conv2d(...)) does."""
    from sradsgan_amd import ops
    gen = torch.Generator().manual_seed(7)
    m, h, w = 2, 37, 45
    x = torch.rand(m, 3, h, w, generator=gen)
    wt, bias = 0.05 * _rnd(gen, 64, 3, 11, 11), 0.1 * _rnd(gen, 64)
    img, ch, py, px = 1, 2, 18, 9
    x[img, ch, py, px] = NAN
    shift = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)

    def stock(dtype):
        v = (2 * x.to(dtype) - 1 - shift.to(dtype)) / scale.to(dtype)
        return F.relu(F.conv2d(v, wt.to(dtype), bias.to(dtype), stride=4, padding=2))
    ref, t32 = stock(torch.float64), stock(torch.float32)
    ho, wo = ref.shape[2:]
    want = torch.zeros(m, 64, ho, wo, dtype=torch.bool)
    for oy in range(ho):
        for ox in range(wo):
            if oy * 4 - 2 <= py <= oy * 4 + 8 and ox * 4 - 2 <= px <= ox * 4 + 8:
                want[img, :, oy, ox] = True
    assert 4 <= int(want[img, 0].sum()) <= 9
    w_hwio = wt.permute(2, 3, 1, 0).contiguous().to(DEV)
    got = ops.lpips_stem_raw(x.to(DEV), w_hwio, bias.to(DEV), normalize=True)
    torch.cuda.synchronize()
    tab = _Table('lpips stem NaN')
    _check_finite_part(tab, 'stem', got, ref, t32, want)
    tab.done()


def test_dense_relu_keeps_a_nan_row_nan():
    """classify.dense_fwd (srhip_cls_dense_fwd, relu on, dropout off): a NaN feature in one row makes that row NaN in every output and
    leaves the other rows finite and equal to relu(x w + b)."""
    from sradsgan_amd import classify
    gen = torch.Generator().manual_seed(9)
    m, k, n = 5, 264, 40
    x, wt, bias = _rnd(gen, m, k), 0.1 * _rnd(gen, k, n), 0.1 * _rnd(gen, n)
    x[3, 129] = NAN
    want = torch.zeros(m, n, dtype=torch.bool)
    want[3] = True
    ref = F.relu(x.double() @ wt.double() + bias.double())
    t32 = F.relu(x @ wt + bias)
    got = classify.dense_fwd(x.to(DEV), wt.to(DEV), bias.to(DEV), relu=True)
    torch.cuda.synchronize()
    tab = _Table('classifier dense NaN')
    _check_finite_part(tab, 'dense', got, ref, t32, want)
    tab.done()


def _ca_stock(u, fc1, b1, fc2, b2, dtype):
    """s [n][c] = sigmoid(fc2 relu(fc1 mean_hw u + b1) + b2) in stock torch; u [n][c][h][w]."""
    a = u.to(dtype).mean((2, 3))
    hid = F.relu(F.linear(a, fc1.to(dtype), None if b1 is None else b1.to(dtype)))
    return torch.sigmoid(F.linear(hid, fc2.to(dtype), None if b2 is None else b2.to(dtype)))


@pytest.mark.parametrize('biased', [False, True])
def test_channel_attention_gate_of_an_image_with_a_nan_is_nan(biased):
    """ops.ca_residual (ca.hip), with and without biases: out = s * u + x with x = 0, so the gate shows in the output.  A NaN in one
    pixel of one image makes that image's mean NaN in one channel, its hidden layer and so its whole gate NaN: every element of that
    image's output is NaN; the other images are finite and equal the reference."""
    from sradsgan_amd import ops
    gen = torch.Generator().manual_seed(11 + int(biased))
    n, c, h, w, hid = 3, 64, 6, 7, 4
    u = _rnd(gen, n, c, h, w) + 0.5
    fc1, fc2 = 0.3 * _rnd(gen, hid, c, 1, 1), 0.3 * _rnd(gen, c, hid, 1, 1)
    b1, b2 = (0.2 * _rnd(gen, hid), 0.2 * _rnd(gen, c)) if biased else (None, None)
    u[1, 17, 3, 4] = NAN
    want = torch.zeros(n, c, h, w, dtype=torch.bool)
    want[1] = True
    stock = lambda dt: _ca_stock(u, fc1.view(hid, c), b1, fc2.view(c, hid), b2, dt)[:, :, None, None] * u.to(dt)
    dev = lambda t: None if t is None else t.to(DEV)
    got = ops.ca_residual(dev(u), torch.zeros_like(u).to(DEV), dev(fc1), dev(fc2), None, dev(b1), dev(b2))
    torch.cuda.synchronize()
    tab = _Table('ca_residual NaN, biases %s' % biased)
    _check_finite_part(tab, 's * u', got, stock(torch.float64), stock(torch.float32), want)
    tab.done()


def test_hat_channel_attention_gate_of_an_image_with_a_nan_is_nan():
    """srhip_hat_ca_fwd (hat.hip): the gate s of the image that holds a NaN pixel is NaN in every channel, the gates of the other
    images are finite and equal the reference."""
    gen = torch.Generator().manual_seed(13)
    n, c, h, w, hid = 3, 60, 5, 8, 6
    u = _rnd(gen, n, c, h, w) + 0.5
    w1, b1, w2, b2 = 0.3 * _rnd(gen, hid, c), 0.2 * _rnd(gen, hid), 0.3 * _rnd(gen, c, hid), 0.2 * _rnd(gen, c)
    u[2, 59, 4, 7] = NAN
    want = torch.zeros(n, c, dtype=torch.bool)
    want[2] = True
    und = u.permute(0, 2, 3, 1).contiguous().to(DEV)
    s, mz = P.Guarded((n, c), DEV), P.Guarded((n, c + hid), DEV)
    args = [t.to(DEV) for t in (w1, b1, w2, b2)]
    _ok(_lib().srhip_hat_ca_fwd(und.data_ptr(), *[t.data_ptr() for t in args], s.ptr(), mz.ptr(), n, h * w, c, hid, _stream()), 'hat_ca_fwd')
    torch.cuda.synchronize()
    tab = _Table('hat_ca_fwd NaN')
    _check_finite_part(tab, 's', s.t, _ca_stock(u, w1, b1, w2, b2, torch.float64), _ca_stock(u, w1, b1, w2, b2, torch.float32), want)
    if not (s.bands_intact() and mz.bands_intact()):
        tab.bad.append('sentinel band overwritten')
    tab.done()
