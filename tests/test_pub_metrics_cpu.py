"""The papers' evaluation protocol without a GPU: the restatement the GPU tests compare against (tests/pub_metrics_ref.py) agrees with
itself in its two forms, the departure of the fp64 luma from BasicSR's float32 intermediate is measured and bounded, and every refusal
of sradsgan_amd.metrics and of the trainers' eval_protocol arguments is raised before any library call."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import pub_metrics_ref as R

T = 16      # the SSIM kernel's tile side; test_library_reports_its_geometry holds the library to it

# (N, H, W, crop, y) of the GPU test; one image of each is enough here
SHAPES = [(1, 11, 11, 0, False), (1, 19, 19, 4, True), (2, 23, 37, 0, False), (2, 23, 37, 0, True), (3, 40, 29, 3, True),
          (1, T + 10, T + 11, 0, False), (1, 2 * T + 10, T + 9, 2, True), (1, 300, 520, 4, True)]

# Departure of this package's fp64 Y from Y rounded through BasicSR's float32 intermediate, worst over SHAPES x {random, near_copy},
# as measured when this test was written (printed by test_luma_departure_from_float32_intermediate; DESIGN.md section 9 records them).
# The float32 rounding of Y / 255 moves Y by up to 255 * 2^-25 = 7.6e-6: against byte differences of order 1 that is 1e-5 relative in
# the MSE, i.e. 1e-4 dB at the most, and a few 1e-8 in SSIM; the images here gave 2.865e-8 and 8.880e-6 dB.
RECORDED_SSIM_DEPARTURE = 2.9e-8
RECORDED_PSNR_DEPARTURE_DB = 8.9e-6


def test_window():
    g = R.gaussian()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15
    assert abs(g[0] - 0.00102838) < 5e-9 and np.array_equal(g, g[::-1]) and g.argmax() == 5


def test_full_and_separable_restatements_agree():
    worst = 0.0
    for i, (n, h, w, crop, y) in enumerate(SHAPES):
        for kind in ('random', 'near_copy'):
            a, b = R.pair(kind, h, w, 3, 100 + i)
            full = R.metrics(a, b, crop, y)
            sep = R.metrics(a, b, crop, y, ssim_fn=R.ssim_separable)
            worst = max(worst, abs(full['ssim'] - sep['ssim']))
            assert full['mse'] == sep['mse']
    print('full vs separable SSIM, worst |difference| = %.3e' % worst)
    assert worst <= 1e-10


def test_luma_departure_from_float32_intermediate():
    ds = dp = 0.0
    for i, (n, h, w, crop, y) in enumerate(SHAPES):
        for kind in ('random', 'near_copy'):
            a, b = R.pair(kind, h, w, 3, 100 + i)
            ours = R.metrics(a, b, crop, True)
            theirs = R.metrics(a, b, crop, True, luma_fn=R.luma_basicsr)
            ds = max(ds, abs(ours['ssim'] - theirs['ssim']))
            dp = max(dp, abs(ours['psnr'] - theirs['psnr']))
    print('fp64 Y vs float32-intermediate Y: SSIM %.3e, PSNR %.3e dB' % (ds, dp))
    assert 0.0 < ds < 10 * RECORDED_SSIM_DEPARTURE and 0.0 < dp < 10 * RECORDED_PSNR_DEPARTURE_DB


def test_restatement_on_known_images():
    a, b = R.pair('equal_constants', 23, 37, 3, 0)
    for y in (False, True):
        m = R.metrics(a, b, 0, y)
        assert m['mse'] == 0.0 and m['psnr'] == float('inf') and abs(m['ssim'] - 1.0) < 1e-12
    # white against black: Y = 235 against 16, mse = 219^2
    w, k = np.full((13, 13, 3), 255, np.uint8), np.zeros((13, 13, 3), np.uint8)
    assert abs(R.metrics(w, k, 0, True)['mse'] - 219.0 ** 2) < 1e-9 and R.metrics(w, k, 0, False)['mse'] == 65025.0
    # the crop removes exactly the border: a difference confined to it vanishes
    c = k.copy()
    c[0, :] = 9
    assert R.metrics(c, k, 1, False)['mse'] == 0.0 and R.metrics(c, k, 0, False)['mse'] > 0.0
    # 0.5f * 255.f = 127.5 and 0.1f * 255.f = 25.5 exactly in float32: both round to the even neighbour
    q = R.quantise(np.array([-1.0, 0.0, 0.1, 0.5, 1.0, 2.0, np.inf, -np.inf, np.nan], np.float32))
    assert q.tolist() == [0, 0, 26, 128, 255, 255, 255, 0, 0]


def test_library_reports_its_geometry():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip, metrics
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    partials, tile = metrics.library_config()
    assert tile == T and partials >= 64
    lib = _hip.lib()
    rc = lib.srhip_pub_ssim(None, None, None, 1, 16, 16, 3, 0, 0, 0, None)
    assert rc == -1 and b'null tensor' in lib.srhip_last_error()


def _refusing_library(monkeypatch):
    from sradsgan_amd import _hip

    def no_lib():
        raise AssertionError('a refusal reached the library')
    monkeypatch.setattr(_hip, 'lib', no_lib)


def test_refusals_before_any_library_call(monkeypatch):
    from sradsgan_amd import metrics as M
    _refusing_library(monkeypatch)
    u = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    f = torch.zeros(2, 3, 16, 16)
    for fn, x in ((M.published_metrics_u8, u), (M.published_metrics, f)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(x, x)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(x, x, 2, True)
        for bad in (-1, 1.0, '1', None, True):
            with pytest.raises(ValueError, match='crop_border'):
                fn(x, x, bad)
        with pytest.raises(ValueError, match='SSIM window'):
            fn(x, x, 3)                                                  # 16 - 6 = 10 < 11
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.published_metrics_u8(u[0], u[0])                               # [H, W, C]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.quantise(f)
    for name in ('calculate_psnr', 'calculate_ssim'):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            getattr(M, name)(u[0], u[0], 2, True)
        with pytest.raises(ValueError):
            getattr(M, name)(u, u)                                       # a batch is not an image
        with pytest.raises(ValueError, match='SSIM window'):
            getattr(M, name)(u[0], u[0], crop_border=3)
    # shape mismatch
    with pytest.raises(ValueError, match='shape mismatch'):
        M.published_metrics_u8(u, u[:, :15])
    with pytest.raises(ValueError, match='shape mismatch'):
        M.published_metrics(f, f[:1])
    # wrong dtype for the entry
    with pytest.raises(ValueError, match='uint8'):
        M.published_metrics_u8(f.permute(0, 2, 3, 1), f.permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match='float32'):
        M.published_metrics(u.permute(0, 3, 1, 2), u.permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match='float32'):
        M.published_metrics(f.double(), f.double())
    with pytest.raises(ValueError, match='float32'):
        M.quantise(u)
    # channels
    with pytest.raises(ValueError, match='1 or 3 channels'):
        M.published_metrics_u8(u[..., :2], u[..., :2])
    with pytest.raises(ValueError, match='1 or 3 channels'):
        M.published_metrics(torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError, match='y_channel needs 3'):
        M.published_metrics_u8(u[..., :1], u[..., :1], 0, True)
    with pytest.raises(ValueError, match='y_channel needs 3'):
        M.published_metrics(f[:, :1], f[:, :1], y_channel=True)
    # ranks
    with pytest.raises(ValueError):
        M.published_metrics_u8(u[0, 0], u[0, 0])
    with pytest.raises(ValueError):
        M.published_metrics(f[0], f[0])


def test_evaluate_scene_refusals(monkeypatch):
    from sradsgan_amd import scene
    _refusing_library(monkeypatch)
    gen = torch.nn.Conv2d(3, 3, 1)
    with pytest.raises(ValueError, match='multiple of scale'):
        scene.evaluate_scene(gen, torch.zeros(96, 126, 3, dtype=torch.uint8), 4, 12, 3)
    with pytest.raises(ValueError, match='uint8'):
        scene.evaluate_scene(gen, torch.zeros(96, 128, 3), 4, 12, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        scene.evaluate_scene(gen, torch.zeros(96, 128, 3, dtype=torch.uint8), 4, 12, 3)


def test_eval_protocol_arguments():
    from sradsgan_amd import trainer as T_
    d = T_.default_args()
    assert d.eval_protocol == 'reference' and d.eval_crop_border is None and d.eval_y_channel is True
    assert T_.evaluation_protocol(d) is None
    assert T_.evaluation_protocol(argparse.Namespace(scale_factor=4)) is None                     # absent fields: off
    assert T_.evaluation_protocol(T_.default_args(eval_protocol='published')) == dict(crop_border=8, y_channel=True)
    assert T_.evaluation_protocol(argparse.Namespace(scale_factor=4, eval_protocol='published')) == dict(crop_border=4, y_channel=True)
    got = T_.evaluation_protocol(T_.default_args(eval_protocol='published', eval_crop_border=0, eval_y_channel=False))
    assert got == dict(crop_border=0, y_channel=False)
    for bad in ('basicsr', 'Published', '', None, True):
        with pytest.raises(ValueError, match='eval_protocol'):
            T_.evaluation_protocol(T_.default_args(eval_protocol=bad))
    for bad in (-1, 2.0, '4', True):
        with pytest.raises(ValueError, match='eval_crop_border'):
            T_.evaluation_protocol(T_.default_args(eval_protocol='published', eval_crop_border=bad))
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='eval_y_channel'):
            T_.evaluation_protocol(T_.default_args(eval_protocol='published', eval_y_channel=bad))
    # the trainer reads them before it asks for a GPU
    with pytest.raises(ValueError, match='eval_protocol'):
        T_.SRADSGAN(T_.default_args(eval_protocol='paper'))
