"""The NaN policy of csrc/common.h -- a NaN activation must surface; max and ReLU behave like ATen's -- held at the sites that take
a maximum with zero or over a window: the 2x2 max pools (elementwise.hip), the LPIPS stem's ReLU (lpips.hip), the ReLU of the
classifier's dense layers (classify.hip) and of the channel-attention MLPs (ca.hip, hat.hip).  One NaN goes in, the expected NaN set
comes out, everything else stays finite and equal to the stock-torch operation on the CPU (fp64 reference, the bar of
tests/test_reductions_gpu.py set by fp32 torch).

The same policy at every clamp, clip, norm and soft-max: the gradient penalty (losses.hip: Linf norm, hinge), the loss reductions, Adam
with the discriminator's weight clip (optim.hip), the diffusion sampler's clamp (diffusion.hip), the soft-max / arg-max kernels
(diffusion.hip, global_attn.hip, hat.hip, hat_wide.hip, amssrn.hip, classify.hip) and -- a byte cannot carry a NaN -- byte 0 at the three
quantisers.  The expected NaN set is written out by hand AND asserted equal to stock torch's on the CPU in fp32 and fp64; every element
outside it is compared (never a sample), and how many those are is asserted."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gan_options_ref as GO
from tests import gdp_ref as GR
from tests import pointwise_ref as P
from tests import reduction_ref as R
from tests.reduction_ref import ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_LR
from tests.test_reductions_gpu import _Table, _lib, _ok, _p, _stream

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


# --------------------------------------------------------------------------------------------- #
# gradient penalty (losses.hip): srhip_gp_norm_penalty_* and the six kinds of srhip_gp_penalty_*
# --------------------------------------------------------------------------------------------- #

GP_NPIX = 773                                                   # four blocks of 256 pixels, the last one ragged
GP_KINDS = [('old', 'L2', 'LS')] + [('kinds', n, p) for n, p in GO.PAIRS]


def _gp_placements(c):
    """(label, pixel, channel of the NaN, value of that pixel's other channels or None for what gp_inputs put there).  The last two
    are the two orders inside a pixel that a running maximum can meet: the NaN before a larger finite channel, and after it."""
    out = [('pixel 0 channel 0', 0, 0, None), ('pixel 300 last channel', 300, c - 1, None),
           ('last pixel middle channel', GP_NPIX - 1, c // 2, None)]
    if c > 1:
        out += [('NaN before a larger channel', 300, 0, 2.0), ('NaN after a larger channel', 300, c - 1, 2.0)]
    return out


def _gp_call(lib, entry, norm, pen, direction, *args):
    from sradsgan_amd import ops
    if entry == 'old':
        fn = lib.srhip_gp_norm_penalty_fwd if direction == 'fwd' else lib.srhip_gp_norm_penalty_bwd
        _ok(fn(*args, _stream()), 'gp_norm_penalty_' + direction)
    else:
        fn = lib.srhip_gp_penalty_fwd if direction == 'fwd' else lib.srhip_gp_penalty_bwd
        _ok(fn(*args, ops.GP_NORMS[norm], ops.GP_PENALTIES[pen], _stream()), 'gp_penalty_' + direction)


@pytest.mark.parametrize('entry,norm,pen', GP_KINDS, ids=['%s-%s-%s' % k for k in GP_KINDS])
@pytest.mark.parametrize('c', [1, 3, 4])
def test_gradient_penalty_is_nan_when_one_gradient_channel_is(c, entry, norm, pen):
    """One NaN channel in one pixel of the [773][C] gradient image: the penalty is NaN, as the reference expression (sradsgan.py:624-637)
    is in stock torch -- torch.max(|g|, 1) and ReLU keep a NaN.  The backward (gout = 1) of every OTHER pixel is bit-identical to the
    backward of the same image with 0.5 in the NaN's place (pixels are independent, 1 / npix is unchanged) and meets the fp64 bar; the
    gradient AT the NaN pixel is unspecified, only the sentinel bands are asserted for it.  Once per kind the same through
    ops.gp_penalty and autograd."""
    from sradsgan_amd import ops
    lib = _lib()
    base = GO.gp_inputs(GP_NPIX, c)
    one = torch.ones(1, device=DEV)
    ws = torch.empty(lib.srhip_reduce_workspace() // 4, device=DEV)
    tab = _Table('gp NaN %s %s/%s C=%d' % (entry, norm, pen, c))
    for label, pix, ch, others in _gp_placements(c):
        clean = base.clone()
        if others is not None:
            clean[pix] = others
        clean[pix, ch] = 0.5
        g = clean.clone()
        g[pix, ch] = NAN
        keep = torch.ones(GP_NPIX, dtype=torch.bool)
        keep[pix] = False                                        # by hand: the NaN pixel alone is exempt
        # the expected forward, by hand: NaN -- and so says the reference expression in stock torch, and the fp64 restatement
        for dt in (torch.float32, torch.float64):
            assert math.isnan(float(GO.gp_expression(GO.as4(g.to(dt)), norm, pen))), (label, dt)
        assert math.isnan(float(GO.gp_ref(g, 1.0, norm, pen)[0])), label
        gd, cd = g.to(DEV), clean.to(DEV)
        out, dg, dclean = P.Guarded((1,), DEV), P.Guarded((GP_NPIX, c), DEV), P.Guarded((GP_NPIX, c), DEV)
        _gp_call(lib, entry, norm, pen, 'fwd', _p(gd), out.ptr(), _p(ws), ws.numel() * 4, GP_NPIX, c)
        _gp_call(lib, entry, norm, pen, 'bwd', _p(gd), _p(one), dg.ptr(), GP_NPIX, c)
        _gp_call(lib, entry, norm, pen, 'bwd', _p(cd), _p(one), dclean.ptr(), GP_NPIX, c)
        torch.cuda.synchronize()
        got, got_clean = dg.t.cpu(), dclean.t.cpu()
        assert got[keep].numel() == (GP_NPIX - 1) * c
        tab.same_bits(label + ': penalty is NaN', torch.isnan(out.t.cpu()), torch.ones(1, dtype=torch.bool))
        tab.same_bits(label + ': dg of the other pixels', got[keep].view(torch.int32), got_clean[keep].view(torch.int32))
        ref, t32 = GO.gp_ref(clean, 1.0, norm, pen)[1], GO.gp_autograd(clean, 1.0, norm, pen)[1]
        tab.check(label + ': those against fp64', got[keep], ref[keep], t32[keep])
        if not (out.bands_intact() and dg.bands_intact() and dclean.bands_intact()):
            tab.bad.append((label, 'sentinel band overwritten'))
        if c == 3 and others is None and pix == GP_NPIX - 1 and (entry == 'old' or (norm, pen) != ('L2', 'LS')):
            x = gd.clone().requires_grad_()                      # ops.gp_penalty picks this very entry point for (norm, pen)
            v = ops.gp_penalty(GO.as4(x), norm, pen)
            v.backward()
            torch.cuda.synchronize()
            tab.same_bits('ops.gp_penalty: NaN', torch.isnan(v.detach().cpu()), torch.tensor(True))
            tab.same_bits('ops.gp_penalty: dg of the other pixels', x.grad.cpu()[keep].view(torch.int32), got_clean[keep].view(torch.int32))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# loss reductions (losses.hip)
# --------------------------------------------------------------------------------------------- #

LOSS_N = 2051                # 512 float4 items over three blocks + the 3-element scalar tail (2048..2050) that block 0 owns


@pytest.mark.parametrize('where', ['body', 'tail', 'b'])
def test_loss_reductions_are_nan_when_one_element_is(where):
    """srhip_l1_mean_fwd, srhip_mse_mean_fwd, srhip_smooth_l1_mean_fwd (tensor and scalar target) and srhip_mean_fwd with one NaN in the
    float4 body, in the scalar tail, or in the second operand: the scalar is NaN, as the nn.*Loss modules give it on the CPU."""
    lib = _lib()
    a, b = R.loss_inputs(LOSS_N)
    s = R.scalar_target_inputs(LOSS_N, 1.0)
    spot = {'body': 1000, 'tail': LOSS_N - 2, 'b': 1000}[where]
    assert (spot >= LOSS_N // 4 * 4) == (where == 'tail')
    (b if where == 'b' else a)[spot] = NAN
    s[spot] = NAN
    ws = torch.empty(lib.srhip_reduce_workspace() // 4, device=DEV)
    ad, bd, sd = a.to(DEV), b.to(DEV), s.to(DEV)
    tail = (_p(ws), ws.numel() * 4, LOSS_N, _stream())
    runs = [('l1_mean', lambda o: lib.srhip_l1_mean_fwd(_p(ad), _p(bd), o, *tail), lambda dt: torch.nn.L1Loss()(a.to(dt), b.to(dt)), R.l1_ref(a, b, 1.0)[0]),
            ('mse_mean', lambda o: lib.srhip_mse_mean_fwd(_p(ad), _p(bd), o, *tail), lambda dt: torch.nn.MSELoss()(a.to(dt), b.to(dt)), R.mse_ref(a, b, 1.0)[0]),
            ('smooth_l1_mean', lambda o: lib.srhip_smooth_l1_mean_fwd(_p(ad), _p(bd), 0.0, o, *tail),
             lambda dt: torch.nn.SmoothL1Loss()(a.to(dt), b.to(dt)), R.smooth_l1_ref(a, b, 1.0)[0])]
    if where != 'b':                                              # one operand only
        runs += [('smooth_l1_mean(target 1)', lambda o: lib.srhip_smooth_l1_mean_fwd(_p(sd), None, 1.0, o, *tail),
                  lambda dt: torch.nn.SmoothL1Loss()(s.to(dt), torch.ones(LOSS_N, dtype=dt)), R.smooth_l1_ref(s, 1.0, 1.0)[0]),
                 ('mean', lambda o: lib.srhip_mean_fwd(_p(ad), o, *tail), lambda dt: a.to(dt).mean(), R.mean_ref(a, 1.0)[0])]
    tab = _Table('loss NaN in %s' % where)
    yes = torch.ones(1, dtype=torch.bool)                         # by hand: the scalar is NaN, and nothing else is there to compare
    for name, run, stock, ref64 in runs:
        out = P.Guarded((1,), DEV)
        _ok(run(out.ptr()), name)
        torch.cuda.synchronize()
        tab.same_bits(name + ': NaN', torch.isnan(out.t.cpu()), yes)
        for dt in (torch.float32, torch.float64):
            tab.same_bits(name + ': stock torch %s' % str(dt)[6:], torch.isnan(stock(dt)).reshape(1), yes)
        tab.same_bits(name + ': fp64 restatement', torch.isnan(ref64).reshape(1), yes)
        if not out.bands_intact():
            tab.bad.append((name, 'sentinel band overwritten'))
    tab.done()


# --------------------------------------------------------------------------------------------- #
# Adam with the discriminator's weight clip (optim.hip)
# --------------------------------------------------------------------------------------------- #

ADAM_NAN_N = 2052            # 513 float4 items: three blocks
INF = float('inf')
# case -> (tensor, element, value, hand-written NaN sets {step: (p, m, v)} as "is that element NaN")
ADAM_NAN_CASES = {
    'g[0]=nan': ('g', 0, NAN, {1: (True, True, True), 2: (True, True, True)}),
    'g[5]=nan': ('g', 5, NAN, {1: (True, True, True), 2: (True, True, True)}),
    'g[2051]=nan': ('g', 2051, NAN, {1: (True, True, True), 2: (True, True, True)}),
    'p[5]=nan': ('p', 5, NAN, {1: (True, False, False), 2: (True, False, False)}),
    # m = inf, v = inf, m / (sqrt(v) + eps) = inf / inf = NaN; the next finite gradient makes m = inf + (g - inf) / 8 = NaN, v stays inf
    'g[5]=inf': ('g', 5, INF, {1: (True, False, False), 2: (True, True, False)}),
}


def _adam_inputs():
    p0, grads = R.adam_inputs(ADAM_NAN_N)
    gen = torch.Generator().manual_seed(515)
    grads = [grads[0], grads[4]]                                  # two steps of gradient scale 1
    for g in grads:
        g[:R.ADAM_FROZEN] = torch.randn(R.ADAM_FROZEN, generator=gen)     # a live head: the NaN's lane-mates get real updates
    return p0, grads


def _adam_device(p0, grads, clip):
    """srhip_adam_step once per gradient on guarded arenas.  Returns [(p, m, v) after each step], bands intact."""
    lib = _lib()
    n = p0.numel()
    p, m, v = (P.Guarded((n,), DEV) for _ in range(3))
    p.t.copy_(p0), m.t.zero_(), v.t.zero_()
    state = torch.zeros(4, device=DEV)
    steps = []
    for g in grads:
        gd = g.to(DEV)
        _ok(lib.srhip_adam_step(p.ptr(), _p(gd), m.ptr(), v.ptr(), _p(state), n, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, clip, _stream()),
            'adam_step')
        torch.cuda.synchronize()
        steps.append(tuple(x.t.cpu().clone() for x in (p, m, v)))
    return steps, all(x.bands_intact() for x in (p, m, v))


@pytest.mark.parametrize('clip', [0.0, 0.01])
@pytest.mark.parametrize('case', list(ADAM_NAN_CASES))
def test_adam_keeps_a_nan_weight_nan_with_and_without_the_clip(case, clip):
    """srhip_adam_step, two steps, the second with a finite gradient, after a NaN (or +inf) in one gradient element or a NaN already in
    one weight: the NaN sets of p, exp_avg and exp_avg_sq after each step are the hand-written ones and those of torch.optim.Adam (+
    clamp_) on the CPU; every other element -- the three lane-mates of the same float4 among them -- is bit-identical to the device
    run without the NaN and meets the fp64 bar."""
    which, e, value, sets = ADAM_NAN_CASES[case]
    p0, grads = _adam_inputs()
    clean, ok_clean = _adam_device(p0, grads, clip)
    p1, g1 = p0.clone(), [g.clone() for g in grads]
    (p1 if which == 'p' else g1[0])[e] = value
    got, ok = _adam_device(p1, g1, clip)
    t32, t64 = R.adam_stock(p1, g1, clip, torch.float32), R.adam_stock(p1, g1, clip, torch.float64)
    ref = R.adam_ref(p1, g1, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, clip)
    tab = _Table('adam NaN %s clip=%g' % (case, clip))
    keep = torch.ones(ADAM_NAN_N, dtype=torch.bool)
    keep[e] = False
    for step in (1, 2):
        for k, name in enumerate(('p', 'exp_avg', 'exp_avg_sq')):
            label = 'step %d %s' % (step, name)
            want = torch.zeros(ADAM_NAN_N, dtype=torch.bool)
            want[e] = sets[step][k]
            x, x32, x64 = got[step - 1][k], t32[step - 1][k], t64[step - 1][k]
            tab.same_bits(label + ': NaN set', torch.isnan(x), want)
            tab.same_bits(label + ': NaN set of torch fp32', torch.isnan(x32), want)
            tab.same_bits(label + ': NaN set of torch fp64', torch.isnan(x64), want)
            tab.same_bits(label + ': +inf set of torch fp32', x == INF, x32 == INF)
            assert x[keep].numel() == ADAM_NAN_N - 1
            tab.same_bits(label + ': every other element', x[keep].view(torch.int32), clean[step - 1][k][keep].view(torch.int32))
            tab.check(label + ': those against fp64', x[keep], ref[step - 1][k][keep], x32[keep])
    if not (ok and ok_clean):
        tab.bad.append('sentinel band overwritten')
    tab.done()


# --------------------------------------------------------------------------------------------- #
# diffusion sampler (diffusion.hip)
# --------------------------------------------------------------------------------------------- #

SAMPLER_ROWS = 50
SAMPLER_MODES = [('noise given', True, 1), ('noise given, t = 0', True, 0), ('noise drawn', False, 1), ('no noise, t = 0', False, 0)]
SAMPLER_SEED, SAMPLER_STEP = 17, 3


def _in_rows(t, ld):
    """t [rows][ch] on the device inside rows of stride ld; the padding holds NaN: reading it would show."""
    buf = torch.full((t.shape[0], ld), NAN, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize('ch,ld', [(3, 3), (6, 8)], ids=['50x3', '50x6-in-8'])
def test_sampler_step_keeps_a_nan_at_its_element(ch, ld):
    """srhip_diff_sampler_step (gdp_kernels.sampler_step) on 50 x 3 elements (150: no multiple of 4, the `e >= total` exit runs) and on
    50 x 6 inside rows of 8: a NaN in x0 (first and last element), in xt, or in a supplied noise comes out at exactly that element --
    x_recon.clamp_(-1, 1) keeps it -- and every other element is bit-identical to the NaN-free call, with the noise given, drawn in the
    kernel or absent (t = 0: a NaN in the unused noise changes nothing).  x0 = +-inf gives the value of x0 = +-1."""
    from sradsgan_amd.model import gdp_kernels as K
    rows, total = SAMPLER_ROWS, SAMPLER_ROWS * ch
    gen = torch.Generator().manual_seed(40 + ch)
    x0, xt, z = 1.6 * _rnd(gen, rows, ch), 2.0 * _rnd(gen, rows, ch), torch.randn(rows, ch, generator=gen)
    c1, c2, lv = (float(v[500]) for v in GR.posterior(GR.betas64('linear', 1000)))
    drawn = K.randn_rows(torch.empty(rows, ch, device=DEV), SAMPLER_SEED, SAMPLER_STEP).cpu()
    tab = _Table('sampler step NaN %dx%d ld %d' % (rows, ch, ld))

    def device(a0, at, an, given, t_nonzero):
        out = P.Guarded((rows, ld), DEV)
        out.t.fill_(777.0)
        K.sampler_step(_in_rows(a0, ld), _in_rows(at, ld), out.t[:, :ch], c1, c2, lv, t_nonzero, noise=_in_rows(an, ld) if given else None,
                       seed=SAMPLER_SEED, step=SAMPLER_STEP)
        torch.cuda.synchronize()
        res = out.t.cpu()
        if not (out.bands_intact() and bool((res[:, ch:] == 777.0).all())):
            tab.bad.append('sentinel band or row padding overwritten')
        return res[:, :ch].clone()

    def stock(dt, a0, at, an, given, t_nonzero):
        v = c1 * a0.to(dt).clamp(-1.0, 1.0) + c2 * at.to(dt)                  # x_recon.clamp_(-1., 1.), then the posterior mean
        return v + math.exp(0.5 * lv) * (an if given else drawn).to(dt) if t_nonzero else v

    for mode, given, t_nonzero in SAMPLER_MODES:
        clean = device(x0, xt, z, given, t_nonzero)
        tab.check(mode + ': NaN-free call', clean, stock(torch.float64, x0, xt, z, given, t_nonzero), stock(torch.float32, x0, xt, z, given, t_nonzero))
        for label, which, e in (('x0 first', 0, 0), ('x0 last', 0, total - 1), ('xt', 1, 77), ('noise', 2, 77)):
            if which == 2 and not given:
                continue
            ins = [x0.clone(), xt.clone(), z.clone()]
            ins[which].view(-1)[e] = NAN
            want = torch.zeros(rows, ch, dtype=torch.bool)
            want.view(-1)[e] = not (which == 2 and not t_nonzero)          # by hand: that element, unless the noise is not used
            got = device(*ins, given, t_nonzero)
            name = '%s, NaN in %s' % (mode, label)
            tab.same_bits(name + ': NaN set of torch fp64', torch.isnan(stock(torch.float64, *ins, given, t_nonzero)), want)
            _check_finite_part(tab, name, got, stock(torch.float64, *ins, given, t_nonzero), stock(torch.float32, *ins, given, t_nonzero), want)
            assert got[~want].numel() == total - int(want.sum()) and int(want.sum()) == int(not (which == 2 and not t_nonzero))
            tab.same_bits(name + ': every other element', got[~want].view(torch.int32), clean[~want].view(torch.int32))
        for sign in (1.0, -1.0):
            big, unit = x0.clone(), x0.clone()
            big.view(-1)[total - 2], unit.view(-1)[total - 2] = sign * INF, sign
            assert torch.equal(stock(torch.float32, big, xt, z, given, t_nonzero), stock(torch.float32, unit, xt, z, given, t_nonzero))
            tab.same_bits('%s, x0 = %+g as x0 = %+g' % (mode, sign * INF, sign), device(big, xt, z, given, t_nonzero).view(torch.int32),
                          device(unit, xt, z, given, t_nonzero).view(torch.int32))
    tab.done()


@pytest.mark.parametrize('planted_in', ['x_T', 'condition'])
def test_sampling_from_a_nan_start_returns_a_nan_image_and_leaves_the_other_alone(planted_in):
    """The six-step loop of tests/test_gdp_gpu.py's small net on a batch of two, its draws those of seed 5, with one NaN planted in
    image 1 of x_T, or of the condition: image 1 of the result contains NaN, image 0 is finite and bit-identical to the clean run --
    which is the seeded run.  A NaN in x_T also travels through c2 * x_t, whatever the clamp does; a NaN in the condition reaches the
    result through the U-Net's prediction and the sampler's clamp alone (x_t stays finite), which is the case of a broken network."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp
    net = GR.init_(gdp.UNet(**GR.SMALL)).to(DEV)
    G = gdp.GaussianDiffusion(net, image_size=12, channels=3, conditional=True)
    G.set_new_noise_schedule(GR.LOOP_SCHEDULE, DEV)
    cond = GR.small_input()[:, 3:].contiguous().to(DEV)
    seed = 5
    draws = torch.stack([gdp.randn_rows(torch.empty(2, 12, 12, 3, device=DEV), seed, k).permute(0, 3, 1, 2) for k in range(7)]).contiguous()
    planted, bad_cond = draws.clone(), cond.clone()
    if planted_in == 'x_T':
        planted[0, 1, 2, 7, 4] = NAN
    else:
        bad_cond[1, 2, 7, 4] = NAN
    with ops.conv_math('fp32'):
        seeded = G.super_resolution_batch(cond, seed=seed).cpu()
        clean = G.super_resolution_batch(cond, noise=draws).cpu()
        got = G.super_resolution_batch(bad_cond, noise=planted).cpu()
    assert tuple(got.shape) == (2, 3, 12, 12)
    assert bool(torch.isfinite(clean).all()) and torch.equal(clean.view(torch.int32), seeded.view(torch.int32))
    assert bool(torch.isnan(got[1]).any())
    assert bool(torch.isfinite(got[0]).all()) and got[0].numel() == 3 * 12 * 12
    assert torch.equal(got[0].view(torch.int32), clean[0].view(torch.int32))


# --------------------------------------------------------------------------------------------- #
# byte outputs: a byte cannot carry a NaN, the three quantisers write 0 (include/sradsgan_hip.h)
# --------------------------------------------------------------------------------------------- #


def test_byte_outputs_write_zero_for_a_nan():
    """srhip_diff_quant_u8, srhip_quant_sse (through the per-image sums against a known partner image) and srhip_scene_blend_u8: the
    byte of a NaN element is 0, every other byte is that of the NaN-free input.  (No comparison with torch's or numpy's cast of a NaN to
    uint8: that is undefined.)"""
    lib = _lib()
    gen = torch.Generator().manual_seed(23)
    # ---- diffusion quantiser
    rows, ch, e = 50, 3, 100
    x = 1.5 * _rnd(gen, rows, ch)
    want = torch.from_numpy(GR.quantize(x.numpy()))
    x.view(-1)[e] = NAN
    want.view(-1)[e] = 0
    out = P.Guarded((rows, ch), DEV, torch.uint8)
    xd = x.to(DEV)
    _ok(lib.srhip_diff_quant_u8(_p(xd), ch, out.ptr(), rows, ch, -1.0, 1.0, _stream()), 'diff_quant_u8')
    torch.cuda.synchronize()
    assert torch.equal(out.t.cpu(), want) and out.bands_intact()
    # ---- validation metrics: byte = trunc(255 v) for v in [0, 1)
    n, per = 2, 3 * 9 * 11
    nb = lib.srhip_metric_blocks()
    byte = lambda t: (t * 255.0).to(torch.int64)
    for nan_in in ('a', 'b'):
        a, b = torch.rand(n, per, generator=gen), torch.rand(n, per, generator=gen)
        a[1, 200] = b[1, 200] = 100.5 / 255.0                     # the known partner byte: 100
        qa, qb = byte(a), byte(b)
        assert int(qa[1, 200]) == 100 and int(qb[1, 200]) == 100
        (a if nan_in == 'a' else b)[1, 200] = NAN
        (qa if nan_in == 'a' else qb)[1, 200] = 0                 # by hand: the NaN counts as byte 0, so this element adds 100^2
        part = P.Guarded((n, nb, 2), DEV, torch.int64)
        ad, bd = a.to(DEV), b.to(DEV)
        _ok(lib.srhip_quant_sse(_p(ad), _p(bd), part.ptr(), n, per, _stream()), 'quant_sse')
        torch.cuda.synchronize()
        sums = part.t.cpu().sum(1)
        assert part.bands_intact()
        assert torch.equal(sums[:, 0], ((qa - qb) ** 2).sum(1)) and torch.equal(sums[:, 1], qb.sum(1)), (nan_in, sums)
        others = torch.ones(per, dtype=torch.bool)
        others[200] = False
        assert int(sums[1, 0]) == int(((qa - qb)[1, others] ** 2).sum()) + 100 * 100
    # ---- scene blend: six 32 x 32 tiles side by side without overlap, the NaN in tile 4 (HR origin 32, 32)
    from tests import scene_ref
    from tests.test_scene_gpu import _run
    tiles = scene_ref.random_tiles(6, 32, 32, 5)
    assert tuple(scene_ref.origins(32, 48, 16, 0)[4]) == (16, 16)
    _, clean_u8, _ = _run(32, 48, 2, 16, 0, tiles)
    tiles[4, 1, 3, 5] = NAN
    f32, u8, _ = _run(32, 48, 2, 16, 0, tiles)
    spot = torch.zeros(64, 96, 3, dtype=torch.bool)
    spot[35, 37, 1] = True
    assert torch.equal(torch.isnan(f32), spot) and int(u8[35, 37, 1]) == 0
    assert u8[~spot].numel() == 64 * 96 * 3 - 1 and torch.equal(u8[~spot], clean_u8[~spot])


# --------------------------------------------------------------------------------------------- #
# soft-max and arg-max kernels.  They take the row maximum with fmaxf (or a comparison a NaN fails), which drops a NaN, but
# expf(NaN - m) poisons the row sum: the row comes out NaN, as torch's softmax does.  Pinned here so that a rewrite cannot lose it.
# Each kernel against the fp32 / fp64 restatement and the bar of its own test file; the expected NaN sets are written out by hand:
#   NaN in one query row  -> that query's output row (of that head) and its lse
#   NaN in one key row    -> every query that sees the key: its whole window / quadrant / image (of that head), output and lse
#   NaN in one value elem -> that channel of every query that sees the value (0 * NaN = NaN); the lse stays finite
# --------------------------------------------------------------------------------------------- #

WHERE = ['query', 'key', 'value']


def _nan_set_and_rest(tab, name, got, want, count, t32, ref64, err_of, bar_of):
    """The NaN set of got is `want` (`count` elements, by hand) and so is the fp32 and the fp64 restatement's; EVERY other element is
    under bar_of(err of the fp32 restatement's rest), both measured by err_of on the rest alone."""
    got, t32, ref64 = got.detach().cpu(), t32.detach().cpu(), ref64.detach().cpu()
    assert int(want.sum()) == count and want.shape == got.shape, (name, int(want.sum()), count)
    tab.same_bits(name + ': NaN set', torch.isnan(got), want)
    tab.same_bits(name + ': NaN set, fp32 restatement', torch.isnan(t32), want)
    tab.same_bits(name + ': NaN set, fp64 restatement', torch.isnan(ref64), want)
    keep = ~want
    assert int(keep.sum()) == got.numel() - count
    e, e32 = err_of(got[keep], ref64[keep]), err_of(t32[keep], ref64[keep])
    b = bar_of(e32)
    print('%-46s %-22s the rest (%d): err %.3e  fp32 %.3e  bar %.3e%s' % (tab.case, name, int(keep.sum()), e, e32, b, '' if e <= b else '   <-- FAIL'))
    if not e <= b:
        tab.bad.append((name, e, e32, b))


@pytest.mark.parametrize('where', WHERE)
def test_diffusion_attention_rows_that_meet_a_nan_are_nan(where):
    """srhip_diff_attn_fwd and srhip_diff_attn_fwd_lse at n 1, heads 2, ch 32, t 36 (two key tiles, the second ragged; the sharp inputs
    of tests/test_gdp_gpu.py), one NaN in head 1: query token 5, or key / value token 35 in the ragged tile.  Restatement
    gdp_train_ref.attention_grad; bars of tests/test_gdp_gpu.py (out) and tests/test_gdp_train_gpu.py (lse)."""
    from oracle import sradsgan_ref as O
    from tests import gdp_train_ref as T
    from tests.test_gdp_gpu import attention_bar, rel_err
    from tests.test_gdp_train_gpu import lse_bar
    lib = _lib()
    n, heads, ch, t = 1, 2, 32, 36
    qkv = O.det_fill('gdp.attn.%d.%d.%d.%d' % (n, heads, ch, t), (n, t, heads * 3 * ch), 6.0)
    hd, tok, dim = 1, (5 if where == 'query' else 35), 3
    qkv[0, tok, hd * 3 * ch + WHERE.index(where) * ch + dim] = NAN
    want_out, want_lse = torch.zeros(n, t, heads * ch, dtype=torch.bool), torch.zeros(n, heads, t, dtype=torch.bool)
    if where == 'query':
        want_out[0, tok, hd * ch:(hd + 1) * ch] = True
        want_lse[0, hd, tok] = True
    elif where == 'key':
        want_out[0, :, hd * ch:(hd + 1) * ch] = True
        want_lse[0, hd, :] = True
    else:
        want_out[0, :, hd * ch + dim] = True
    counts = {'query': (ch, 1), 'key': (t * ch, t), 'value': (t, 0)}[where]
    dout = torch.ones(n, t, heads * ch)
    out64, lse64, _ = T.attention_grad(qkv, heads, dout, torch.float64)
    out32, lse32, _ = T.attention_grad(qkv, heads, dout, torch.float32)
    qd = qkv.to(DEV)
    plain, with_lse, lse = P.Guarded((n, t, heads * ch), DEV), P.Guarded((n, t, heads * ch), DEV), P.Guarded((n, heads, t), DEV)
    _ok(lib.srhip_diff_attn_fwd(_p(qd), plain.ptr(), n, t, heads, ch, _stream()), 'diff_attn_fwd')
    _ok(lib.srhip_diff_attn_fwd_lse(_p(qd), with_lse.ptr(), lse.ptr(), n, t, heads, ch, _stream()), 'diff_attn_fwd_lse')
    torch.cuda.synchronize()
    tab = _Table('gdp attention NaN in a %s' % where)
    _nan_set_and_rest(tab, 'fwd out', plain.t, want_out, counts[0], out32, out64, rel_err, attention_bar)
    _nan_set_and_rest(tab, 'fwd_lse out', with_lse.t, want_out, counts[0], out32, out64, rel_err, attention_bar)
    _nan_set_and_rest(tab, 'fwd_lse lse', lse.t, want_lse, counts[1], lse32, lse64, rel_err, lse_bar)
    if not (plain.bands_intact() and with_lse.bands_intact() and lse.bands_intact()):
        tab.bad.append('sentinel band overwritten')
    tab.done()


def _attn_table(tab, bufs, names, wants, counts, ref, t32, family, split=None):
    """The outputs `names` of an attn_kernels_ref.Buffers run against attn_kernels_ref's evaluations, err and bars, on the rest alone."""
    from tests import attn_kernels_ref as A
    for name in names:
        keep = ~wants[name]
        sp = None if split is None else {name: split[name][keep]}
        bar = A.bars({name: ref[name][keep]}, {name: t32[name][keep]}, family, True, sp)[name][0]
        _nan_set_and_rest(tab, name, bufs.get(name), wants[name], counts[name], t32[name], ref[name], A.err, lambda e32, bar=bar: bar)
    if bufs.broken_bands():
        tab.bad.append(('sentinel band overwritten', bufs.broken_bands()))


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'split'])
@pytest.mark.parametrize('where', WHERE)
def test_sgam_flash_attention_rows_that_meet_a_nan_are_nan(where, exact):
    """srhip_sgam_flash_fwd at hw 40 (two key tiles, the second ragged), two images, both arithmetics: y, o and lse of image 1 with one
    NaN in its q (pixel 5), k or v (pixel 39); image 0 stays finite."""
    from tests import attn_kernels_ref as A
    from tests.test_global_attn_kernels_gpu import _Arith, _sgam_run
    n, hw = 2, 40
    inp = A.sgam_inputs('random', n, hw)
    pix, dim = (5 if where == 'query' else 39), 3
    inp[{'query': 'q', 'key': 'k', 'value': 'v'}[where]][1, pix, dim] = NAN
    wants = {'y': torch.zeros(n, hw, 64, dtype=torch.bool), 'o': torch.zeros(n, hw, 64, dtype=torch.bool), 'lse': torch.zeros(n, hw, dtype=torch.bool)}
    if where == 'query':
        wants['y'][1, pix] = wants['o'][1, pix] = wants['lse'][1, pix] = True
    elif where == 'key':
        wants['y'][1] = wants['o'][1] = wants['lse'][1] = True
    else:
        wants['y'][1, :, dim] = wants['o'][1, :, dim] = True
    big, small = {'query': (64, 1), 'key': (hw * 64, hw), 'value': (hw, 0)}[where]
    ref, t32 = A.sgam_eval(inp, torch.float64), A.sgam_eval(inp, torch.float32)
    split = None if exact else A.sgam_split_emulation(inp)
    with _Arith(exact):
        bufs = _sgam_run(inp, n, hw)
    tab = _Table('sgam %s NaN in a %s' % ('exact' if exact else 'split', where))
    _attn_table(tab, bufs, ('y', 'o', 'lse'), wants, {'y': big, 'o': big, 'lse': small}, ref, t32, 'sgam', split)
    tab.done()


@pytest.mark.parametrize('pix,ch', [(0, 0), (20, 31), (39, 63)])
def test_cgam_soft_max_of_an_image_with_a_nan_is_nan(pix, ch):
    """srhip_cgam_fwd at hw 40, two images: a NaN in x[1, pix, ch] makes row and column ch of image 1's 64 x 64 energy NaN, so every row
    of its soft-max holds one: att and y of image 1 are NaN throughout, image 0 stays finite."""
    from tests import attn_kernels_ref as A
    from tests.test_global_attn_kernels_gpu import _cgam_run
    n, hw = 2, 40
    inp = A.cgam_inputs(n, hw, 0.3)
    inp['x'][1, pix, ch] = NAN
    wants = {'y': torch.zeros(n, hw, 64, dtype=torch.bool), 'att': torch.zeros(n, 64, 64, dtype=torch.bool)}
    wants['y'][1] = wants['att'][1] = True
    ref, t32 = A.cgam_eval(inp, torch.float64), A.cgam_eval(inp, torch.float32)
    bufs = _cgam_run(inp, n, hw)
    tab = _Table('cgam NaN at pixel %d channel %d' % (pix, ch))
    _attn_table(tab, bufs, ('y', 'att'), wants, {'y': hw * 64, 'att': 64 * 64}, ref, t32, 'cgam')
    tab.done()


def _window_wants(where, n, h, w, c, heads, ws, shift, img, py, px, hd, dim):
    """By hand: the window of pixel (py, px) under a cyclic shift is the set of pixels with the same ((y - shift) mod h) // ws and
    ((x - shift) mod w) // ws; the shift mask adds -100, it removes no key, so a NaN key reaches every query of its window."""
    d = c // heads
    out, lse = torch.zeros(n, h, w, c, dtype=torch.bool), torch.zeros(n, h, w, heads, dtype=torch.bool)
    win = lambda y, x: (((y - shift) % h) // ws, ((x - shift) % w) // ws)
    mates = [(y, x) for y in range(h) for x in range(w) if win(y, x) == win(py, px)]
    assert len(mates) == ws * ws
    if where == 'query':
        out[img, py, px, hd * d:(hd + 1) * d] = True
        lse[img, py, px, hd] = True
        return out, lse, d, 1
    for y, x in mates:
        if where == 'key':
            out[img, y, x, hd * d:(hd + 1) * d] = True
            lse[img, y, x, hd] = True
        else:
            out[img, y, x, hd * d + dim] = True
    return (out, lse, ws * ws * d, ws * ws) if where == 'key' else (out, lse, ws * ws, 0)


@pytest.mark.parametrize('shift', [0, 4], ids=['unshifted', 'shifted'])
@pytest.mark.parametrize('where', WHERE)
def test_hat_window_attention_rows_that_meet_a_nan_are_nan(where, shift):
    """srhip_hat_attn_fwd, SA at window 8 on 2 x 16 x 16 (eight windows), unshifted and shifted by 4: one NaN in q, k or v of pixel
    (9, 3) of image 1, head 2."""
    from tests import attn_kernels_ref as A
    from tests.test_hat_kernels_gpu import _attn_run
    n, h, w, ws, c, heads = 2, 16, 16, 8, 96, 6
    inp = A.hat_attn_inputs(('NaN', 0, ws, shift, n, h, w, 'random'))
    img, py, px, hd, dim = 1, 9, 3, 2, 5
    inp['qkv'][img, py, px, WHERE.index(where) * c + hd * (c // heads) + dim] = NAN
    want_out, want_lse, c_out, c_lse = _window_wants(where, n, h, w, c, heads, ws, shift, img, py, px, hd, dim)
    ref, t32 = A.hat_attn_eval(inp, torch.float64), A.hat_attn_eval(inp, torch.float32)
    bufs = _attn_run(inp)
    tab = _Table('hat attn shift %d NaN in a %s' % (shift, where))
    _attn_table(tab, bufs, ('out', 'lse'), {'out': want_out, 'lse': want_lse}, {'out': c_out, 'lse': c_lse}, ref, t32, 'hat_attn')
    tab.done()


@pytest.mark.parametrize('shift', [0, 8], ids=['unshifted', 'shifted'])
@pytest.mark.parametrize('where', WHERE)
def test_hat_wide_window_attention_rows_that_meet_a_nan_are_nan(where, shift):
    """srhip_hatw_attn_fwd, SA at window 16 with six heads of 24 channels on 2 x 32 x 32 (eight windows; the geometry of its own kernel
    test), unshifted and shifted by 8: one NaN in q, k or v of pixel (19, 5) of image 1, head 2."""
    from tests import hat_wide_ref as W
    from tests.test_hat_wide_kernels_gpu import _attn_run
    d, heads, n, h, w = 24, 6, 2, 32, 32
    c = d * heads
    inp = W.attn_inputs((W.SA, d, heads, shift, n, h, w, 'random'))
    img, py, px, hd, dim = 1, 19, 5, 2, 7
    inp['qkv'][img, py, px, WHERE.index(where) * c + hd * d + dim] = NAN
    want_out, want_lse, c_out, c_lse = _window_wants(where, n, h, w, c, heads, W.WS, shift, img, py, px, hd, dim)
    ref, t32 = W.attn_eval(inp, torch.float64), W.attn_eval(inp, torch.float32)
    bufs = _attn_run(inp)
    tab = _Table('hatw attn shift %d NaN in a %s' % (shift, where))
    _attn_table(tab, bufs, ('out', 'lse'), {'out': want_out, 'lse': want_lse}, {'out': c_out, 'lse': c_lse}, ref, t32, 'hat_attn')
    tab.done()


@pytest.mark.parametrize('where', WHERE)
def test_quadrant_attention_rows_that_meet_a_nan_are_nan(where):
    """srhip_nl_quad_fwd at 3 x 17 x 31 (seven blocks, image boundaries inside a block): one NaN in theta, phi or g of pixel (9, 20) of
    image 1, which lies in the quadrant rows 8..16 x columns 15..30 (144 pixels).  y and the saved row sum l against
    leaf_kernels_ref.nl_eval under the bar of tests/test_nl_quad_kernels_gpu.py.  The saved row maximum m is the one output whose NaN set
    is NOT torch's: the kernel's running maximum passes over a NaN logit where amax returns it (nothing reads m without l, which is
    NaN there), so m is pinned to what include/sradsgan_hip.h says: the maximum of the row's other logits, -inf when all are NaN."""
    from tests import leaf_kernels_ref as L
    from tests.test_nl_quad_kernels_gpu import _outputs, _run
    n, h, w = L.NL_INDEPENDENCE
    inp = L.nl_inputs('unit', n, h, w)
    img, py, px, dim = 1, 9, 20, 3
    inp[{'query': 'theta', 'key': 'phi', 'value': 'g'}[where]][img, py, px, dim] = NAN
    rows, cols = slice(8, 17), slice(15, 31)                       # by hand: h // 2 = 8, w // 2 = 15
    want_y, want_l = torch.zeros(n, h, w, 8, dtype=torch.bool), torch.zeros(n, h, w, dtype=torch.bool)
    if where == 'query':
        want_y[img, py, px] = want_l[img, py, px] = True
    elif where == 'key':
        want_y[img, rows, cols] = want_l[img, rows, cols] = True
    else:
        want_y[img, rows, cols, dim] = True
    c_y, c_l = {'query': (8, 1), 'key': (144 * 8, 144), 'value': (144, 0)}[where]
    ref, t32 = L.nl_eval(inp, torch.float64), L.nl_eval(inp, torch.float32)
    bufs = _run(inp)
    got = _outputs(bufs, n, h, w)
    tab = _Table('nl_quad NaN in a %s' % where)
    _nan_set_and_rest(tab, 'y', got['y'], want_y, c_y, t32['y'], ref['y'], R.err, R.bound)
    _nan_set_and_rest(tab, 'l', got['l'], want_l, c_l, t32['l'], ref['l'], R.err, R.bound)
    # the saved maximum, everywhere: the maximum of the logits that are not NaN (-inf for a NaN query, whose logits all are), by hand
    # from the fp64 logits -- torch's amax returns NaN on those rows, so there the restatement is nl_logits with the NaN logits left out
    m_ref, m_32 = torch.zeros(n, h, w, dtype=torch.float64), torch.zeros(n, h, w)
    clean32 = {k: v.float() for k, v in inp.items()}
    for q, s64 in zip(L.nl_quadrants(h, w), L.nl_logits(inp)):
        s32 = L._quad(clean32['theta'], q) @ L._quad(clean32['phi'], q).transpose(1, 2)
        L._unquad(m_ref, q, torch.nan_to_num(s64, nan=-INF).amax(-1))
        L._unquad(m_32, q, torch.nan_to_num(s32, nan=-INF).amax(-1))
    low = m_ref == -INF
    assert int(low.sum()) == int(where == 'query') and torch.equal(torch.isnan(ref['m']), want_l) and torch.equal(m_ref[~want_l], ref['m'][~want_l])
    tab.same_bits('m: no NaN; -inf for the NaN query alone', torch.stack([torch.isnan(got['m']), got['m'] == -INF]), torch.stack([torch.zeros_like(low), low]))
    tab.check('m, every finite one (%d)' % int((~low).sum()), got['m'][~low], m_ref[~low], m_32[~low])
    if bufs.broken():
        tab.bad.append(('sentinel band overwritten or input changed', bufs.broken()))
    tab.done()


@pytest.mark.parametrize('col', [0, 10, 20])
def test_classifier_soft_max_and_arg_max_with_a_nan_logit(col):
    """srhip_cls_softmax_ce_fwd_bwd and srhip_cls_confusion on 21 x 21 logits (six blocks of four row waves, the last ragged) with one
    NaN in row 7 at the first, a middle or the last class: that row's loss, its dlogits and the batch sum are NaN as log_softmax's
    are; every other row is under classify_ref.ce_bounds; the prediction of row 7 is the NaN's class, as torch.argmax (and numpy's)
    treat a NaN as the maximum, and the confusion table counts it there."""
    from sradsgan_amd import classify as S
    from tests import classify_ref as C
    from tests.test_classify_gpu import _logits
    m, c, row = 21, 21, 7
    z, y = _logits('normal', m, c, 1000 * m + 10 * c)
    clean = z.clone()
    z[row, col] = NAN
    want_row = torch.zeros(m, dtype=torch.bool)
    want_row[row] = True
    want_dz = want_row[:, None].expand(m, c).clone()
    onehot = F.one_hot(y.long(), c)
    stock = {}
    for dt in (torch.float32, torch.float64):
        logp = torch.log_softmax(z.to(dt), 1)
        stock[dt] = (-(logp * onehot.to(dt)).sum(1), (logp.exp() - onehot.to(dt)) / m)
    zd, yd = z.to(DEV), y.to(DEV)
    row_loss, total, dz = P.Guarded((m,), DEV), P.Guarded((1,), DEV, torch.float64), P.Guarded((m, c), DEV)
    pred, table = P.Guarded((m,), DEV, torch.int32), P.Guarded((c, c), DEV, torch.int32)
    table.t.zero_()
    lib = _lib()
    _ok(lib.srhip_cls_softmax_ce_fwd_bwd(_p(zd), _p(yd), row_loss.ptr(), total.ptr(), dz.ptr(), m, c, 1.0 / m, _stream()), 'cls_softmax_ce')
    _ok(lib.srhip_cls_confusion(_p(zd), _p(yd), pred.ptr(), table.ptr(), m, c, _stream()), 'cls_confusion')
    torch.cuda.synchronize()
    tab = _Table('classifier NaN logit at class %d' % col)
    loss_b, dz_b = C.ce_bounds(clean, y, 1.0 / m)                   # rows are independent: the other rows' bounds are the clean ones
    for name, got, want, k, bnd in (('row loss', row_loss.t.cpu(), want_row, 0, loss_b), ('dlogits', dz.t.cpu(), want_dz, 1, dz_b)):
        assert int(want.sum()) == (1, c)[k]
        tab.same_bits(name + ': NaN set', torch.isnan(got), want)
        for dt in stock:
            tab.same_bits(name + ': NaN set of log_softmax %s' % str(dt)[6:], torch.isnan(stock[dt][k]), want)
        keep = ~want
        assert int(keep.sum()) == (m - 1) * (1, c)[k]
        ratio = float(((got.double() - stock[torch.float64][k]).abs() / bnd)[keep].max())
        print('%-46s %-22s the rest (%d): err / bound %.3g' % (tab.case, name, int(keep.sum()), ratio))
        if not ratio <= 1.0:
            tab.bad.append((name, ratio))
    tab.same_bits('batch sum is NaN', torch.isnan(total.t.cpu()), torch.ones(1, dtype=torch.bool))
    assert math.isnan(float(stock[torch.float64][0].sum()))
    want_pred = torch.argmax(clean, 1)
    want_pred[row] = col                                            # by hand: the NaN is the maximum
    assert torch.equal(torch.argmax(z, 1), want_pred) and torch.equal(torch.argmax(z.double(), 1), want_pred)
    assert np.array_equal(np.argmax(z.numpy(), axis=1), want_pred.numpy())
    tab.same_bits('predictions', pred.t.cpu().long(), want_pred)
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (y.numpy().astype(np.int64), want_pred.numpy()), 1)
    tab.same_bits('confusion table', table.t.cpu().long(), torch.from_numpy(cm))
    if not all(g.bands_intact() for g in (row_loss, total, dz, pred, table)):
        tab.bad.append('sentinel band overwritten')
    tab.done()
