"""The degradation kernels (csrc/degrade.hip) and what is built on them -- degrade.BatchBlur, SRMDPreprocessing,
degraded_training_batch, the trainer's switches -- on the device.  The blur's summation order is part of its contract, so every byte
and every float is compared EXACTLY with the numpy restatement tests/degrade_ref.py, and the bytes with the reference's recorded
ones (tests/golden/degrade.npz); only the reference's own fp32 blur, summed in another order, gets the summation bound."""
import os

import numpy as np
import pytest
import torch

from tests import degrade_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'degrade.npz'))
CASES = [tuple(int(v) for v in row) for row in GOLDEN['cases']]                    # (l, scale, H, W)


def _case(l):
    return {k[len('l%d_' % l):]: GOLDEN[k] for k in GOLDEN.files if k.startswith('l%d_' % l)}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _kernels(n, l, seed):
    """n different kernels of both kinds, float32 [n, l, l] numpy."""
    from sradsgan_amd import degrade as G
    return G.random_batch_kernel(n, l=l, rate_iso=0.5, generator=torch.Generator().manual_seed(seed)).numpy()


def _blur_u8(src, kernels):
    from sradsgan_amd import degrade as G
    out = G.blur_u8(torch.from_numpy(src).to(DEV), torch.from_numpy(np.ascontiguousarray(kernels)).to(DEV))
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == src.shape
    return out.cpu().numpy()


# --------------------------------------------------------------------------------------------- #
# srhip_blur_u8
# --------------------------------------------------------------------------------------------- #

def test_blur_u8_where_every_output_reflects_at_both_ends():
    """11 x 11 with l = 21: lo = 10 = H - 1, the largest padding the contract admits."""
    src = np.random.RandomState(1).randint(0, 256, (3, 11, 11, 3)).astype(np.uint8)
    k = _kernels(3, 21, 1)
    assert np.array_equal(_blur_u8(src, k), R.blur_u8(src, k))


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('l', [1, 4, 11, 15, 21])
def test_blur_u8_odd_row_bytes_every_store_phase_and_even_kernels(l, c):
    """23 x 19: rows of 19 c bytes (odd for c = 1, 3) start at every byte phase, so heads, whole dwords and tails all run; l = 4 pads
    2 before and 1 after; l = 1 is the identity up to the quantiser."""
    src = np.random.RandomState(10 * l + c).randint(0, 256, (3, 23, 19, c)).astype(np.uint8)
    k = _kernels(3, l, l + c)
    assert np.array_equal(_blur_u8(src, k), R.blur_u8(src, k))


@pytest.mark.parametrize('l', [4, 21])
def test_blur_u8_past_one_tile_in_both_axes(l):
    """70 x 69: more than two 32-wide tiles (and past any tile of 64) in both axes, halos crossing the seams, ragged last tiles."""
    src = np.random.RandomState(l).randint(0, 256, (3, 70, 69, 3)).astype(np.uint8)
    k = _kernels(3, l, 50 + l)
    assert np.array_equal(_blur_u8(src, k), R.blur_u8(src, k))


@pytest.mark.parametrize('l,i0,j0', [(21, 3, 17), (4, 3, 0), (11, 0, 9)])
def test_blur_u8_orientation_is_cross_correlation_rows_first(l, i0, j0):
    """A kernel that is 1 at the single off-centre tap (i0, j0), i0 != j0, gives q(xpad[y + i0][x + j0]): a reflected shift, computed
    here by indexing.  A convolution (flipped kernel) or swapped axes would shift the other way."""
    h, w, c = 23, 19, 3
    src = np.random.RandomState(l).randint(0, 256, (2, h, w, c)).astype(np.uint8)
    k = np.zeros((2, l, l), np.float32)
    k[:, i0, j0] = 1.0
    lo = l // 2
    want = np.empty_like(src)
    for y in range(h):
        for x in range(w):
            sy, sx = R.reflect_index(y - lo + i0, h), R.reflect_index(x - lo + j0, w)
            v = src[:, sy, sx, :].astype(np.float32) / np.float32(255.0)
            want[:, y, x, :] = (v * np.float32(255.0)).astype(np.int32).astype(np.uint8)
    got = _blur_u8(src, k)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, _blur_u8(src, np.ascontiguousarray(k.transpose(0, 2, 1))))     # the test can tell rows from columns


def test_blur_u8_bytes_do_not_depend_on_the_batch():
    src = np.random.RandomState(7).randint(0, 256, (3, 37, 35, 3)).astype(np.uint8)
    k = _kernels(3, 15, 7)
    whole = _blur_u8(src, k)
    for b in range(3):
        assert np.array_equal(_blur_u8(src[b:b + 1], k[b:b + 1])[0], whole[b])                     # alone
        first = [b] + [i for i in range(3) if i != b]
        last = first[1:] + [b]
        assert np.array_equal(_blur_u8(src[first], k[first])[0], whole[b])                         # first of three
        assert np.array_equal(_blur_u8(src[last], k[last])[2], whole[b])                           # last of three
    perm = [2, 0, 1]
    assert np.array_equal(_blur_u8(src[perm], k[perm]), whole[perm])
    assert np.array_equal(_blur_u8(src, k), whole)                                                 # a re-run is bit-identical


# --------------------------------------------------------------------------------------------- #
# srhip_blur_f32
# --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('l', [4, 21])
@pytest.mark.parametrize('per_sample', [False, True])
@pytest.mark.parametrize('channels_last', [False, True])
def test_blur_f32_bit_identical_to_the_restatement(l, per_sample, channels_last):
    from sradsgan_amd import degrade as G
    x = torch.rand(3, 3, 23, 19, generator=torch.Generator().manual_seed(l)) * 2 - 0.5
    k = torch.from_numpy(_kernels(3, l, 3 * l))
    k = k if per_sample else k[1]
    xd = x.to(DEV)
    if channels_last:
        xd = xd.contiguous(memory_format=torch.channels_last)
    y = G.BatchBlur(l)(xd, k.to(DEV))
    assert y.stride() == xd.stride() and tuple(y.shape) == tuple(x.shape)
    assert _same_bits(y, torch.from_numpy(R.blur_f32(x.numpy(), k.numpy())))


@pytest.mark.parametrize('channels_last', [False, True])
def test_blur_f32_more_channels_than_one_launch_takes(channels_last):
    """Six channels: the kernel stages four planes per launch, so this runs one launch of four and one of two."""
    from sradsgan_amd import degrade as G
    x = torch.rand(2, 6, 13, 35, generator=torch.Generator().manual_seed(6))
    k = torch.from_numpy(_kernels(2, 11, 4))
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last) if channels_last else x.to(DEV)
    y = G.BatchBlur(11)(xd, k.to(DEV))
    assert y.stride() == xd.stride() and _same_bits(y, torch.from_numpy(R.blur_f32(x.numpy(), k.numpy())))


@pytest.mark.parametrize('l', [4, 21])
def test_blur_f32_nan_poisons_exactly_its_footprint(l):
    from sradsgan_amd import degrade as G
    n, c, h, w = 2, 3, 23, 19
    x = torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(2))
    y0, x0 = 1, 17                                                                 # near two edges: the reflection doubles back
    x[1, 2, y0, x0] = float('nan')
    k = _kernels(n, l, 9)
    y = G.BatchBlur(l)(x.to(DEV), torch.from_numpy(k).to(DEV)).cpu().numpy()
    lo = l // 2
    want = np.zeros((n, c, h, w), bool)
    for yy in range(h):
        for xx in range(w):
            rows = {R.reflect_index(yy - lo + i, h) for i in range(l)}
            cols = {R.reflect_index(xx - lo + j, w) for j in range(l)}
            want[1, 2, yy, xx] = y0 in rows and x0 in cols
    assert 0 < want.sum() < h * w
    assert np.array_equal(np.isnan(y), want)
    ref = R.blur_f32(x.numpy(), k)
    assert np.array_equal(y[~want].view(np.int32), ref[~want].view(np.int32))


# --------------------------------------------------------------------------------------------- #
# the reference's recorded outputs
# --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_device_bytes_equal_the_reference(l, scale, h, w):
    from sradsgan_amd import degrade as G
    g = _case(l)
    assert np.array_equal(_blur_u8(g['src'], g['kernels']), g['blur_u8'])
    pre = G.SRMDPreprocessing(scale, True, kernel=l, noise=False, rate_iso=0.5, seed=1)
    lr, code, used = pre(torch.from_numpy(g['src']).to(DEV), kernel=True, kernels=torch.from_numpy(g['kernels']))
    assert code is None and _same_bits(used, torch.from_numpy(g['kernels']))
    assert np.array_equal(pre.last_lr_u8.cpu().numpy(), g['lr_u8'])
    assert _same_bits(lr, torch.from_numpy(R.to_float(g['lr_u8'])).permute(0, 3, 1, 2))
    assert torch.equal(pre.last_kernels, torch.from_numpy(g['kernels'])) and pre.last_levels is None and pre.last_step == 0


@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_device_fp32_blur_within_the_summation_bound_of_the_reference(l, scale, h, w):
    from sradsgan_amd import degrade as G
    g = _case(l)
    x = R.to_float(g['src']).transpose(0, 3, 1, 2)
    y = G.BatchBlur(l)(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(g['kernels']).to(DEV)).cpu().numpy()
    err = np.abs(y.astype(np.float64) - g['blur_f32'].astype(np.float64))
    bound = R.blur_bound(x, g['kernels'])
    print('l %d: max |device - reference| %.3e, largest share of the bound %.3f' % (l, err.max(), (err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_device_noise_tail_equals_the_reference(l, scale, h, w):
    from sradsgan_amd import degrade as G
    g = _case(l)
    z = torch.from_numpy(np.ascontiguousarray(g['noise_z'].transpose(0, 2, 3, 1))).to(DEV)          # the kernel's layout: [N, H, W, C]
    out = G.degrade_noise_u8(torch.from_numpy(g['lr_u8']).to(DEV), torch.from_numpy(g['noise_levels']).to(DEV), z)
    assert _same_bits(out, torch.from_numpy(g['noise_out']))


# --------------------------------------------------------------------------------------------- #
# srhip_degrade_noise_u8
# --------------------------------------------------------------------------------------------- #

def test_noise_kernel_levels_draws_and_clamps():
    from sradsgan_amd import data as D
    from sradsgan_amd import degrade as G
    from sradsgan_amd.model import gdp_kernels as K
    n, h, w, c = 3, 7, 5, 3                                                        # 105 elements per sample: Philox groups straddle samples
    lr = np.random.RandomState(3).randint(0, 256, (n, h, w, c)).astype(np.uint8)
    lr[0, 0, 0], lr[0, 0, 1], lr[2, 6, 4] = 0, 255, (0, 255, 128)
    lrd = torch.from_numpy(lr).to(DEV)
    zero = G.degrade_noise_u8(lrd, torch.zeros(n, device=DEV), seed=5, step=2)
    assert _same_bits(zero, D.to_tensor(lrd)) and zero.stride() == D.to_tensor(lrd).stride()       # level 0: to_tensor's bits
    levels = np.array([0.05, 0.0, 0.3], np.float32)                                # per-sample levels within one launch
    z = K.randn_rows(torch.empty(n, h, w, c, device=DEV), 5, 2)
    drawn = G.degrade_noise_u8(lrd, torch.from_numpy(levels).to(DEV), seed=5, step=2)
    given = G.degrade_noise_u8(lrd, torch.from_numpy(levels).to(DEV), z=z)
    assert _same_bits(drawn, given)
    want = R.noise_tail(lr, levels, z.cpu().numpy())
    assert _same_bits(given, torch.from_numpy(want).permute(0, 3, 1, 2))
    assert _same_bits(given[1], D.to_tensor(lrd)[1]) and not _same_bits(given[0], D.to_tensor(lrd)[0])
    assert not _same_bits(drawn, G.degrade_noise_u8(lrd, torch.from_numpy(levels).to(DEV), seed=5, step=3))
    big = torch.full((n, h, w, c), 50.0, device=DEV)                               # |level z| far past the range: both ends clamp
    up = G.degrade_noise_u8(lrd, torch.ones(n, device=DEV), z=big)
    down = G.degrade_noise_u8(lrd, torch.ones(n, device=DEV), z=-big)
    assert bool((up == 1.0).all()) and bool((down == 0.0).all())


# --------------------------------------------------------------------------------------------- #
# end to end
# --------------------------------------------------------------------------------------------- #

def test_degraded_training_batch_is_reproducible_and_keeps_hr():
    from sradsgan_amd import data as D
    from sradsgan_amd import degrade as G
    hr = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (3, 24, 30, 3)).astype(np.uint8)).to(DEV)
    runs = []
    for _ in range(2):
        pre = G.SRMDPreprocessing(3, True, kernel=11, noise=True, rate_iso=0.5, noise_high=0.1, rate_cln=0.3, seed=8,
                                  pca_matrix=torch.ones(121, 4))
        runs.append([G.degraded_training_batch(hr, 3, pre) for _ in range(2)] + [pre])
    for call in range(2):
        for a, b in zip(runs[0][call], runs[1][call]):
            assert _same_bits(a, b)
    lr, hr_f, bc = runs[0][1]
    pre = runs[0][2]
    plain_lr, plain_hr, _ = D.training_batch(hr, 3)
    assert _same_bits(hr_f, plain_hr) and tuple(lr.shape) == tuple(plain_lr.shape) and not _same_bits(lr, plain_lr)
    assert not _same_bits(runs[0][0][0], lr)                                       # the second call drew anew
    assert pre.last_step == 1 and tuple(pre.last_kernels.shape) == (3, 11, 11) and tuple(pre.last_levels.shape) == (3,)
    assert _same_bits(bc, D.to_tensor(D.resize_u8(pre.last_lr_u8, 24, 30, 'bicubic')))
    # the recorded draws replay the call: blur, resample and noise from the host tables alone
    k = pre.last_kernels.numpy()
    lr_u8 = R.pil_resize(R.blur_u8(hr.cpu().numpy(), k), 8, 10)
    assert np.array_equal(pre.last_lr_u8.cpu().numpy(), lr_u8)
    from sradsgan_amd.model import gdp_kernels as K
    z = K.randn_rows(torch.empty(3, 8, 10, 3, device=DEV), pre.seed, pre.last_step).cpu().numpy()
    assert _same_bits(lr, torch.from_numpy(R.noise_tail(lr_u8, pre.last_levels.numpy(), z)).permute(0, 3, 1, 2))
    out = pre(hr, kernel=True)
    assert len(out) == 3 and tuple(out[1].shape) == (3, 5) and tuple(out[2].shape) == (3, 11, 11)
    want_code = torch.cat([pre.last_kernels.reshape(3, 121).sum(1, keepdim=True).expand(3, 4), pre.last_levels.reshape(3, 1) * 10], 1)
    assert torch.allclose(out[1].cpu(), want_code, rtol=1e-5, atol=1e-6)
    blurred = G.BlurPreprocessing(3, True, kernel=11, seed=8)(hr)
    assert tuple(blurred.shape) == (3, 3, 24, 30) and blurred.dtype == torch.float32


def _trainer(tmp_path, tag, **switches):
    from sradsgan_amd import trainer as T
    g = torch.Generator().manual_seed(6)
    hr = torch.rand(2, 3, 12, 12, generator=g)
    test = [(torch.nn.functional.avg_pool2d(hr, 2), hr, hr.clamp(0, 1), ['a', 'b'])]
    src = [torch.from_numpy(np.random.RandomState(12 + i).randint(0, 256, (2, 12, 12, 3)).astype(np.uint8)) for i in range(2)]
    args = T.default_args(scale_factor=2, num_epochs=1, batch_size=2, save_dir=str(tmp_path / tag), crop_size=12, hr_height=12,
                          hr_width=12, sample_interval=1, n_residual_blocks=1, n_basic_blocks=1, **switches)
    return T.SRADSGAN(args, train_loader=src, test_loader=test), src


def test_trainer_switches(tmp_path):
    from sradsgan_amd import data as D
    from sradsgan_amd import degrade as G
    off, src = _trainer(tmp_path, 'off')
    assert off.degrade is None and off.degrade_test is None
    plain = D.training_batch(src[0].to(DEV), 2)
    for a, b in zip(off._batch(src[0]), plain):
        assert _same_bits(a, b)                                                    # switches off: training_batch's bits
    on, _ = _trainer(tmp_path, 'on', degrade_blur=True, degrade_kernel=7, degrade_rate_iso=0.5, degrade_seed=3)
    assert isinstance(on.degrade, G.SRMDPreprocessing) and on.degrade_test is None and not on.degrade.noise
    lr, hr, bc = on._batch(src[0])
    assert _same_bits(hr, plain[1]) and tuple(lr.shape) == tuple(plain[0].shape) and not _same_bits(lr, plain[0])
    want = R.pil_resize(R.blur_u8(src[0].numpy(), on.degrade.last_kernels.numpy()), 6, 6)
    assert _same_bits(lr, torch.from_numpy(R.to_float(want)).permute(0, 3, 1, 2))
    for a, b in zip(on._batch(src[0], test=True), D.test_batch(src[0].to(DEV), 2)):
        assert _same_bits(a, b)                                                    # training tiles only
    ev, _ = _trainer(tmp_path, 'eval', degrade_blur=True, degrade_kernel=7, degrade_eval=True, degrade_noise_high=0.1, degrade_seed=3)
    assert ev.degrade.noise and not ev.degrade_test.noise and not ev.degrade_test.random
    first, second = ev._batch(src[1], test=True), ev._batch(src[1], test=True)
    for a, b in zip(first, second):
        assert _same_bits(a, b)                                                    # a reproducible evaluation
    assert not _same_bits(first[0], D.test_batch(src[1].to(DEV), 2)[0])
    assert not _same_bits(ev._batch(src[1])[0], ev._batch(src[1])[0])              # training draws anew each call


def test_two_training_steps_on_degraded_batches(tmp_path):
    net, _ = _trainer(tmp_path, 'train', degrade_blur=True, degrade_kernel=7, degrade_rate_iso=0.5, degrade_noise_high=0.08,
                      degrade_seed=3)
    torch.manual_seed(31)
    np.random.seed(31)
    hist = net.train()
    assert len(hist) == 1 and net.degrade.last_step == 1                            # two iterations of batch 2
    assert all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
