"""LPIPS as a loss, host side: the differentiable fp64 restatement (tests/lpips_loss_ref.py) checked against itself (gradcheck) and
against tests/lpips_ref.py's metric, the closed form of the head gradient that csrc/lpips.hip evaluates against autograd, and the
argument validation of LPIPS.loss and TrainStep that needs no device.  No GPU call."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_loss_ref as L
from tests import lpips_ref as R


@pytest.fixture(scope='module')
def G():
    return np.load(R.GOLDEN)


@pytest.fixture(scope='module')
def sd():
    return R.alexnet_state_dict()


def test_loss_restatement_is_the_mean_of_the_metric(G, sd):
    lin = [G['lin%d' % k] for k in range(5)]
    sr, hr = torch.from_numpy(G['s0_sr']), torch.from_numpy(G['s0_hr'])
    want = R.lpips(sr, hr, sd, lin).mean()
    got = L.loss(sr, hr, sd, lin)
    assert got.dim() == 0 and abs(float(got - want)) <= 1e-14 * float(want)


def test_reference_gradient_passes_gradcheck(G, sd):
    """fp64 autograd of the restatement against central differences on a 1 x 3 x 31 x 31 image (the smallest LPIPS accepts)."""
    lin = [G['lin%d' % k] for k in range(5)]
    hr = R.hash_image((1, 3, 31, 31), 61).double()
    sr = (0.75 * hr + 0.25 * R.hash_image((1, 3, 31, 31), 62).double()).requires_grad_(True)
    # ReLUs and max pools are piecewise linear: a 1e-7 step keeps the two probes of an element on one piece
    assert torch.autograd.gradcheck(lambda p: L.loss(p, hr, sd, lin), (sr,), eps=1e-7, atol=1e-9, rtol=1e-4, nondet_tol=0.0, fast_mode=True)


@pytest.mark.parametrize('c,hw', [(64, (3, 5)), (192, (1, 2)), (256, (4, 4))])
def test_closed_form_head_gradient_matches_autograd(c, hw):
    """The formula of srhip_lpips_head_bwd in fp64 against autograd of the safe-root restatement, with one all-zero pred pixel, one
    all-zero target pixel and one pixel that is zero in both."""
    h, w = hw
    f = F.relu(R.hash16(2 * c * h * w, c + h).double().reshape(2, c, h, w) + 0.1) * 3
    t = F.relu(R.hash16(2 * c * h * w, c + h + 7).double().reshape(2, c, h, w) + 0.1) * 3
    f[0, :, 0, 0] = 0
    t[1, :, 0, w - 1] = 0
    f[1, :, h - 1, 0] = 0
    t[1, :, h - 1, 0] = 0
    lw = (R.hash16(c, 3 * c) + 0.5).double()
    s = 0.37 / (2 * h * w)
    ref = L.head_grad_autograd(f, t, lw, s)
    got = L.head_grad_closed_form(f, t, lw, s)
    assert torch.isfinite(ref).all() and torch.isfinite(got).all() and float(ref.abs().max()) > 0
    assert bool((got[0, :, 0, 0] == 0).all()) and bool((got[1, :, h - 1, 0] == 0).all()) and bool((got[f <= 0] == 0).all())
    assert float(ref[1, :, 0, w - 1].abs().max()) > 0                       # a zero target pixel still pulls on pred
    err = float((got - ref).abs().max())
    print('closed form vs autograd, C=%d %dx%d: %.2e of max|ref| %.2e' % (c, h, w, err, float(ref.abs().max())))
    assert err <= 1e-12 * float(ref.abs().max())


def test_plain_root_gives_nan_at_a_zero_pixel_and_the_safe_root_does_not():
    """why the restatement departs from torch's plain sqrt: the documented n == 0 rule"""
    f = torch.ones(1, 4, 1, 2, dtype=torch.float64)
    f[0, :, 0, 0] = 0
    t = torch.ones_like(f)
    w = torch.ones(4, dtype=torch.float64)
    p = f.clone().requires_grad_(True)
    R.head(t, p, w).sum().backward()
    assert torch.isnan(p.grad[0, :, 0, 0]).all()
    q = f.clone().requires_grad_(True)
    L.head(t, q, w).sum().backward()
    assert torch.isfinite(q.grad).all() and torch.equal(L.head(t, f, w), R.head(t, f, w))


def test_loss_refuses_cpu_tensors_and_a_target_that_requires_grad():
    from sradsgan_amd.lpips import LPIPS
    m = LPIPS()
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.loss(x, x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.loss(x.clone().requires_grad_(True), torch.rand(1, 3, 32, 32))
    with pytest.raises(ValueError, match='pred only'):                      # checked before the device is: pure argument validation
        m.loss(x, x.clone().requires_grad_(True))


def test_library_exports_the_backward_entry_points():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    for name in ('srhip_lpips_head_bwd', 'srhip_maxpool3x3s2_bwd', 'srhip_lpips_stem_bwd'):
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    x = torch.zeros(1)
    p = x.data_ptr()                                                        # host memory: never dereferenced on an argument error
    assert lib.srhip_lpips_head_bwd(p, p, p, p, 1.0, p, 2, 1, 3, 3, 30, None) == -1 and b'C % 4' in lib.srhip_last_error()
    assert lib.srhip_lpips_head_bwd(p, p, p, None, 1.0, p, 2, 1, 3, 3, 64, None) == -1
    assert lib.srhip_maxpool3x3s2_bwd(p, p, None, p, 1, 2, 5, 64, 1, None) == -1 and b'H, W >= 3' in lib.srhip_last_error()
    assert lib.srhip_maxpool3x3s2_bwd(p, p, None, p, 1, 5, 5, 6, 1, None) == -1
    assert lib.srhip_lpips_stem_bwd(p, p, p, 1, 6, 31, 1, None) == -1
    assert lib.srhip_lpips_stem_bwd(p, None, p, 1, 31, 31, 1, None) == -1


def test_train_step_validates_the_lpips_arguments_before_touching_the_device():
    from sradsgan_amd import train_step as TS
    from sradsgan_amd.lpips import LPIPS
    with pytest.raises(ValueError, match='weight_lpips'):
        TS.check_lpips_args(None, 1.0, False)
    with pytest.raises(ValueError, match='weight_lpips'):
        TS.check_lpips_args(LPIPS(), -0.5, False)
    with pytest.raises(ValueError, match='use_graph'):
        TS.check_lpips_args(LPIPS(), 1.0, True)
    assert TS.check_lpips_args(None, 0.0, True) is None                     # weight 0: nothing is asked of the model or the mode
    m = LPIPS()
    assert TS.check_lpips_args(m, 0.5, False) is m
