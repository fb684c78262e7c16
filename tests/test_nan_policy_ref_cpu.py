"""The fp64 restatements that tests/test_nan_propagation_gpu.py leans on -- tests/gan_options_ref.py (gradient penalty),
tests/reduction_ref.py (the older penalty, loss reductions, Adam) and tests/gdp_ref.py (the sampler's reverse step, quantisation) --
must themselves treat a NaN as stock torch does, or a GPU test would compare two NaN-droppers.  One NaN in, the NaN set compared with
the stock-torch expression, on the inputs of the GPU tests at a tenth of their size.  No device is needed."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import gan_options_ref as GO
from tests import gdp_ref as GR
from tests import reduction_ref as R
from tests.reduction_ref import ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_LR

NAN, INF = float('nan'), float('inf')
NPIX = 77


def _placements(c):
    out = [(0, 0, None), (30, c - 1, None), (NPIX - 1, c // 2, None)]
    if c > 1:
        out += [(30, 0, 2.0), (30, c - 1, 2.0)]                   # Linf: the NaN before a larger finite channel, and after it
    return out


@pytest.mark.parametrize('c', [1, 3, 4])
def test_penalty_restatements_return_nan_like_the_reference_expression(c):
    """gan_options_ref.gp_ref (all six kinds) and reduction_ref.gp_ref: the value is NaN where sradsgan.py:624-637 in stock torch is, and
    the gradient of every pixel without a NaN is finite in both."""
    for pix, ch, others in _placements(c):
        g = GO.gp_inputs(NPIX, c)
        if others is not None:
            g[pix] = others
        g[pix, ch] = NAN
        keep = torch.ones(NPIX, dtype=torch.bool)
        keep[pix] = False
        for norm, pen in GO.PAIRS:
            value, dg = GO.gp_ref(g, 1.0, norm, pen)
            assert math.isnan(float(value)), (norm, pen, pix, ch)
            assert bool(torch.isfinite(dg[keep]).all())
            for dt in (torch.float32, torch.float64):
                v, tdg = GO.gp_autograd(g, 1.0, norm, pen, dt)
                assert math.isnan(float(v)) and bool(torch.isfinite(tdg[keep]).all()), (norm, pen, dt)
        value, dg = R.gp_ref(g, 1.0)
        assert math.isnan(float(value)) and bool(torch.isfinite(dg[keep]).all())
        # the pixel's norm itself, against torch.max / norm on the same row
        for norm in GO.NORMS:
            nrm = GO.pixel_norm(g.double(), norm)
            assert torch.equal(torch.isnan(nrm), ~keep), norm


@pytest.mark.parametrize('where', ['body', 'tail', 'b'])
def test_loss_restatements_return_nan_like_the_loss_modules(where):
    n = 205
    a, b = R.loss_inputs(n)
    s = R.scalar_target_inputs(n, 1.0)
    spot = {'body': 100, 'tail': n - 1, 'b': 100}[where]
    (b if where == 'b' else a)[spot] = NAN
    s[spot] = NAN
    pairs = [(R.l1_ref(a, b, 1.0)[0], torch.nn.L1Loss()), (R.mse_ref(a, b, 1.0)[0], torch.nn.MSELoss()),
             (R.smooth_l1_ref(a, b, 1.0)[0], torch.nn.SmoothL1Loss())]
    for value, stock in pairs:
        assert math.isnan(float(value))
        assert math.isnan(float(stock(a, b))) and math.isnan(float(stock(a.double(), b.double())))
    if where != 'b':
        assert math.isnan(float(R.smooth_l1_ref(s, 1.0, 1.0)[0])) and math.isnan(float(torch.nn.SmoothL1Loss()(s, torch.ones(n))))
        assert math.isnan(float(R.mean_ref(a, 1.0)[0])) and math.isnan(float(a.mean()))


ADAM_N = 204
ADAM_CASES = {'g[0]=nan': ('g', 0, NAN), 'g[5]=nan': ('g', 5, NAN), 'g[203]=nan': ('g', ADAM_N - 1, NAN), 'p[5]=nan': ('p', 5, NAN),
              'g[5]=inf': ('g', 5, INF)}


@pytest.mark.parametrize('clip', [0.0, 0.01])
@pytest.mark.parametrize('case', list(ADAM_CASES))
def test_adam_restatement_has_the_nan_sets_of_torch_adam(case, clip):
    """reduction_ref.adam_ref over two steps, the second with a finite gradient: the NaN and +inf sets of p, m and v after each step are
    those of torch.optim.Adam followed by p.data.clamp_(-clip, clip), in fp32 and in fp64."""
    which, e, value = ADAM_CASES[case]
    gen = torch.Generator().manual_seed(204)
    p0 = 0.04 * torch.randn(ADAM_N, generator=gen)
    grads = [torch.randn(ADAM_N, generator=gen) for _ in range(2)]
    (p0 if which == 'p' else grads[0])[e] = value
    ref = R.adam_ref(p0, grads, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, clip)
    for dt in (torch.float32, torch.float64):
        stock = R.adam_stock(p0, grads, clip, dt)
        for step in range(2):
            for k, name in enumerate(('p', 'exp_avg', 'exp_avg_sq')):
                assert torch.equal(torch.isnan(ref[step][k]), torch.isnan(stock[step][k])), (name, step, dt)
                assert torch.equal(ref[step][k] == INF, stock[step][k] == INF), (name, step, dt)
                assert int(torch.isnan(stock[step][k]).sum()) <= 1 and not bool(torch.isnan(stock[step][k][torch.arange(ADAM_N) != e]).any())
    assert bool(torch.isnan(ref[1][0][e]))                        # the weight stays NaN in every case, with and without the clip


@pytest.mark.parametrize('planted_in', ['x_T', 'condition'])
def test_sampler_restatement_keeps_a_nan_prediction_like_clamp_(monkeypatch, planted_in):
    """gdp_ref.sample's reverse step around a point-wise stand-in for the U-Net: a NaN planted in image 1 of x_T, or of the condition,
    comes out at that element alone, as the stock expression x_recon.clamp_(-1., 1.) followed by the posterior mean gives it.  A NaN
    in x_T also travels through c2 * x_t whatever the clamp does; one in the condition reaches the result through the prediction and
    the clamp alone (x_t stays finite), so that case fails for a clamp that drops a NaN (np.fmin(np.fmax(x, -1), 1))."""
    monkeypatch.setattr(GR, 'unet_forward', lambda sd, x, t, cfg, prefix='': 1.7 * x[:, :3] - 0.2 * x[:, 3:])
    o = GR.LOOP_SCHEDULE
    betas = GR.betas64(o['schedule'], o['n_timestep'], o['linear_start'], o['linear_end'])
    c1, c2, lv = GR.posterior(betas)
    gen = torch.Generator().manual_seed(15)
    cond = torch.rand(2, 3, 1, 5, generator=gen, dtype=torch.float64) * 2 - 1
    noise = torch.randn(7, 2, 3, 1, 5, generator=gen, dtype=torch.float64)
    (noise[0] if planted_in == 'x_T' else cond)[1, 2, 0, 3] = NAN
    got = GR.sample(None, cond, noise, betas, None)
    img = noise[0].clone()
    for k, i in enumerate(reversed(range(6))):                     # the stock expression, with the in-place clamp_ of the reference
        x_recon = 1.7 * img - 0.2 * cond
        x_recon.clamp_(-1., 1.)
        img = float(c1[i]) * x_recon + float(c2[i]) * img + (math.exp(0.5 * float(lv[i])) * noise[k + 1] if i > 0 else 0.0)
    want = torch.zeros(2, 3, 1, 5, dtype=torch.bool)
    want[1, 2, 0, 3] = True                                        # by hand: the stand-in is point-wise, so that element alone
    assert torch.equal(torch.isnan(got), want) and torch.equal(torch.isnan(img), want)
    fin = torch.isfinite(img)
    assert float((got[fin] - img[fin]).abs().max()) < 1e-12


def test_quantisation_restatement_writes_byte_zero_for_a_nan():
    """gdp_ref.quantize states what the device documents: a NaN element is byte 0 (numpy's own cast of a NaN to uint8 is undefined and
    warns); every other byte is that of the NaN-free rows."""
    gen = torch.Generator().manual_seed(23)
    x = (1.5 * (torch.rand(5, 3, generator=gen) * 2 - 1)).numpy()
    clean = GR.quantize(x)
    x[2, 1] = NAN
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = GR.quantize(x)
    assert got.dtype == np.uint8 and got[2, 1] == 0
    keep = np.ones((5, 3), bool)
    keep[2, 1] = False
    assert np.array_equal(got[keep], clean[keep]) and keep.sum() == 14
