"""Host side of the blur-and-noise degradation: the numpy restatement (tests/degrade_ref.py) against the reference's recorded
outputs (tests/golden/degrade.npz, tools/make_golden_degrade.py), the kernel generators, the noise levels, the draws, the refusals
and the trainer's switches."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import degrade_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sradsgan_hip.h')
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'degrade.npz'))
CASES = [tuple(int(v) for v in row) for row in GOLDEN['cases']]                    # (l, scale, H, W)


def _case(l):
    return {k[len('l%d_' % l):]: GOLDEN[k] for k in GOLDEN.files if k.startswith('l%d_' % l)}


def test_fixture_holds_the_cases_the_recorder_states():
    assert CASES == [(21, 3, 24, 21), (11, 2, 24, 22), (4, 4, 24, 20)]
    for l, scale, h, w in CASES:
        g = _case(l)
        assert g['src'].shape == (2, h, w, 3) and g['src'].dtype == np.uint8 and g['kernels'].shape == (2, l, l)
        assert g['lr_u8'].shape == (2, int(h / scale), int(w / scale), 3)
        assert sorted(g['params'][:, 3]) == [0.0, 1.0]                            # one isotropic, one anisotropic kernel


# --------------------------------------------------------------------------------------------- #
# the restatement against the reference
# --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_restated_bytes_equal_the_reference(l, scale, h, w):
    g = _case(l)
    blurred = R.blur_u8(g['src'], g['kernels'])
    assert np.array_equal(blurred, g['blur_u8'])
    assert np.array_equal(R.pil_resize(blurred, int(h / scale), int(w / scale)), g['lr_u8'])


@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_restated_fp32_blur_within_the_summation_bound(l, scale, h, w):
    g = _case(l)
    x = R.to_float(g['src']).transpose(0, 3, 1, 2)
    mine, bound = R.blur_f32(x, g['kernels']), R.blur_bound(x, g['kernels'])
    err = np.abs(mine.astype(np.float64) - g['blur_f32'].astype(np.float64))
    print('l %d: max |restated - reference| %.3e, largest share of the bound %.3f' % (l, err.max(), (err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_restated_noise_tail_equals_the_reference(l, scale, h, w):
    g = _case(l)
    out = R.noise_tail(g['lr_u8'].transpose(0, 3, 1, 2), g['noise_levels'], g['noise_z'])
    assert np.array_equal(out.view(np.int32), g['noise_out'].view(np.int32))
    assert np.array_equal(out[1], R.to_float(g['lr_u8'][1]).transpose(2, 0, 1))    # the level-0 sample is untouched


def test_reflection_indices():
    assert [R.reflect_index(i, 5) for i in range(-4, 9)] == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0]
    assert R.pads(21) == (10, 10) and R.pads(4) == (2, 1) and R.pads(1) == (0, 0)
    x = np.arange(12, dtype=np.float32).reshape(1, 1, 3, 4)
    assert np.array_equal(R.reflect_pad(x, 4)[0, 0], np.pad(x[0, 0], ((2, 1), (2, 1)), mode='reflect'))


# --------------------------------------------------------------------------------------------- #
# kernel generators
# --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('l,scale,h,w', CASES)
def test_generators_reproduce_the_recorded_kernels(l, scale, h, w):
    from sradsgan_amd import degrade as G
    g = _case(l)
    made = G.kernels_from_params(g['params'], l)
    assert made.dtype == torch.float32 and tuple(made.shape) == (2, l, l)
    assert R.ulp_distance(made.numpy(), g['kernels']).max() <= 1                    # both sides: float64 formulas cast to fp32
    for b, (sx, sy, theta, iso) in enumerate(g['params']):
        one = G.isotropic_gaussian_kernel(l, sx, tensor=True) if iso else \
            G.anisotropic_gaussian_kernel(l, G.cal_sigma(sx, sy, theta), tensor=True)
        assert R.ulp_distance(one.numpy(), g['kernels'][b]).max() <= 1
        mine = R.isotropic_kernel(l, sx) if iso else R.gaussian_kernel(l, sx, sy, theta)
        assert R.ulp_distance(mine.astype(np.float32), g['kernels'][b]).max() <= 1   # the independent formula agrees too


@pytest.mark.parametrize('l', [1, 4, 11, 15, 21])
def test_every_kernel_sums_to_one(l):
    from sradsgan_amd import degrade as G
    gen = torch.Generator().manual_seed(l)
    k = G.random_batch_kernel(16, l=l, rate_iso=0.5, generator=gen)
    s = G.stable_batch_kernel(3, l=l, sig=2.6)
    assert k.dtype == s.dtype == torch.float32 and tuple(k.shape) == (16, l, l) and tuple(s.shape) == (3, l, l)
    for t in (k, s):
        assert (t >= 0).all()
        assert (t.double().sum((1, 2)) - 1.0).abs().max() <= l * l * 2.0 ** -24
    assert torch.equal(s[0], s[2]) and torch.equal(s[0], G.isotropic_gaussian_kernel(l, 2.6, tensor=True))
    assert isinstance(G.random_batch_kernel(2, l=l, tensor=False, generator=gen), np.ndarray)


def test_random_kernel_parameters_follow_the_reference_ranges():
    from sradsgan_amd import degrade as G
    p = G.random_kernel_params(400, sig_min=0.2, sig_max=4.0, rate_iso=0.5, scaling=3, generator=torch.Generator().manual_seed(9))
    iso = p[:, 3] == 1.0
    assert 120 < iso.sum() < 280
    assert (p[iso, 0] == p[iso, 1]).all() and (p[iso, 2] == 0).all()
    assert (p[:, :2] >= 0.2).all() and (p[:, :2] <= 4.0).all()
    assert (p[~iso, 2] >= -np.pi).all() and (p[~iso, 2] < np.pi).all() and len(set(p[~iso, 2])) == (~iso).sum()
    assert (G.random_kernel_params(50, rate_iso=1.0, generator=torch.Generator().manual_seed(1))[:, 3] == 1).all()
    assert (G.random_kernel_params(50, rate_iso=0.0, generator=torch.Generator().manual_seed(1))[:, 3] == 0).all()


# --------------------------------------------------------------------------------------------- #
# noise levels and draws
# --------------------------------------------------------------------------------------------- #

def test_random_batch_noise_levels_and_mask():
    from sradsgan_amd import degrade as G
    n, high, rate = 64, 0.08, 0.3
    lv = G.random_batch_noise(n, high, rate, generator=torch.Generator().manual_seed(4))
    assert lv.shape == (n, 1) and lv.dtype == np.float64
    assert (lv >= 0).all() and (lv < high).all()
    replay = torch.Generator().manual_seed(4)                                     # the documented order: n levels, then n mask draws
    level = torch.rand(n, generator=replay, dtype=torch.float64).numpy() * high
    mask = torch.rand(n, generator=replay, dtype=torch.float64).numpy()
    clean = mask < rate
    assert 0 < clean.sum() < n
    assert np.array_equal(lv[:, 0] == 0, clean | (level == 0))
    assert np.array_equal(lv[~clean, 0], level[~clean])
    assert (G.random_batch_noise(n, high, 1.0, generator=torch.Generator().manual_seed(4)) == 0).all()
    assert (G.random_batch_noise(n, high, 0.0, generator=torch.Generator().manual_seed(4))[:, 0] == level).all()


def test_same_seed_same_draws_and_rank_changes_them():
    from sradsgan_amd import degrade as G
    mk = lambda seed, rank: G.SRMDPreprocessing(3, True, kernel=11, noise=True, rate_iso=0.5, noise_high=0.1, seed=seed, rank=rank)
    a, b, c = mk(5, 0), mk(5, 0), mk(5, 1)
    assert a.seed == 5 and c.seed == 6 and mk(4, 1).seed == 5
    for _ in range(2):
        ka, kb, kc = a.draw_kernels(4), b.draw_kernels(4), c.draw_kernels(4)
        la, lb, lc = a.draw_levels(4), b.draw_levels(4), c.draw_levels(4)
        assert torch.equal(ka, kb) and torch.equal(la, lb)
        assert not torch.equal(ka, kc) and not torch.equal(la, lc)
        assert la.dtype == torch.float32 and tuple(la.shape) == (4,)
    assert torch.equal(mk(4, 1).draw_kernels(4), mk(5, 0).draw_kernels(4))          # the stream is keyed by seed + rank
    stable = G.SRMDPreprocessing(3, False, kernel=11, sig=1.5, seed=1)
    assert torch.equal(stable.draw_kernels(2), G.stable_batch_kernel(2, 11, 1.5))
    assert G.SRMDPreprocessing(3, True).seed != G.SRMDPreprocessing(3, True).seed   # unseeded: fresh entropy


# --------------------------------------------------------------------------------------------- #
# refusals
# --------------------------------------------------------------------------------------------- #

def test_refusals_before_touching_the_device():
    from sradsgan_amd import degrade as G
    for bad in (0, 22, -1, 2.5):
        with pytest.raises(ValueError, match=r'1\.\.21'):
            G.BatchBlur(bad)
        with pytest.raises(ValueError, match=r'1\.\.21'):
            G.SRMDPreprocessing(3, True, kernel=bad)
        with pytest.raises(ValueError, match=r'1\.\.21'):
            G.BlurPreprocessing(3, True, kernel=bad)
    blur = G.BatchBlur(5)
    x, k = torch.zeros(2, 3, 8, 9), torch.zeros(2, 5, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        blur(x, k)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        blur(x, k[0])
    with pytest.raises(TypeError):
        blur(x, torch.zeros(3, 5, 5))                                             # neither [l, l] nor [B, l, l]
    with pytest.raises(TypeError):
        blur(x.double(), k)
    with pytest.raises(ValueError, match='reflection padding'):
        G.BatchBlur(21)(torch.zeros(1, 3, 10, 30), torch.zeros(21, 21))            # lo = 10 >= H = 10: torch raises there too
    with pytest.raises(ValueError, match='reflection padding'):
        G.BatchBlur(4)(torch.zeros(1, 3, 9, 2), torch.zeros(4, 4))                 # lo = 2 >= W = 2
    u8 = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.blur_u8(u8, k)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.SRMDPreprocessing(2, True, kernel=5)(u8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.BlurPreprocessing(2, True, kernel=5)(u8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.degrade_noise_u8(u8, torch.zeros(2))
    with pytest.raises(NotImplementedError):
        G.BlurPreprocessing(2, True, kernel=5)(u8, noise=True)
    with pytest.raises(TypeError):
        G.SRMDPreprocessing(2, True, kernel=5, pca_matrix=torch.zeros(24, 4))


def test_grad_requiring_inputs_are_refused():
    from sradsgan_amd import degrade as G
    with pytest.raises(RuntimeError, match='no backward'):
        G.BatchBlur(3)(torch.zeros(1, 3, 8, 8, requires_grad=True), torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match='no backward'):
        G.BatchBlur(3)(torch.zeros(1, 3, 8, 8), torch.zeros(3, 3, requires_grad=True))
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):      # nothing records a graph here: the next check
        G.BatchBlur(3)(torch.zeros(1, 3, 8, 8, requires_grad=True), torch.zeros(3, 3))


# --------------------------------------------------------------------------------------------- #
# trainer switches
# --------------------------------------------------------------------------------------------- #

def test_trainer_switches_default_off_and_build_nothing():
    import argparse
    from sradsgan_amd import degrade as G
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import drcan
    want = dict(degrade_blur=False, degrade_kernel=21, degrade_random=True, degrade_sig=2.6, degrade_sig_min=0.2, degrade_sig_max=4.0,
                degrade_rate_iso=1.0, degrade_scaling=3, degrade_noise_high=0.0, degrade_rate_cln=0.2, degrade_seed=None,
                degrade_eval=False)
    for args in (T.default_args(), drcan.default_args()):
        for name, value in want.items():
            assert getattr(args, name) == value and type(getattr(args, name)) is type(value), name
        assert T.training_degrade(args) is None and T.training_degrade(args, test=True) is None
    assert T.training_degrade(argparse.Namespace(crop_size=216, scale_factor=8)) is None            # a reference Namespace: no fields
    assert T.training_degrade(T.default_args(degrade_eval=True), test=True) is None                 # degrade_eval alone builds nothing
    d = T.training_degrade(T.default_args(degrade_blur=True, degrade_kernel=11, degrade_seed=5, scale_factor=4), rank=2)
    assert isinstance(d, G.SRMDPreprocessing) and d.l == 11 and d.scale == 4 and d.seed == 7 and d.random and not d.noise
    assert T.training_degrade(T.default_args(degrade_blur=True), test=True) is None                 # training tiles only
    d = T.training_degrade(T.default_args(degrade_blur=True, degrade_noise_high=0.05, degrade_rate_cln=0.5))
    assert d.noise and d.noise_high == 0.05 and d.rate_cln == 0.5
    e = T.training_degrade(T.default_args(degrade_blur=True, degrade_eval=True, degrade_noise_high=0.05, degrade_sig=1.7), test=True)
    assert isinstance(e, G.SRMDPreprocessing) and not e.random and not e.noise and e.sig == 1.7
    assert torch.equal(e.draw_kernels(2), G.stable_batch_kernel(2, 21, 1.7))


# --------------------------------------------------------------------------------------------- #
# ABI: the new entry points are declared alike in the header and the ctypes table, and refuse bad arguments on the host
# --------------------------------------------------------------------------------------------- #

_CTYPES = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
           'unsigned long long': ctypes.c_ulonglong}


def _header_signature(name):
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, name
    args = []
    for a in m.group(1).split(','):
        a = ' '.join(a.replace('const', '').split())
        args.append(ctypes.c_void_p if '*' in a else _CTYPES[a.rsplit(' ', 1)[0]])
    return ctypes.c_int, args


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


@pytest.mark.parametrize('name', ['srhip_blur_u8', 'srhip_blur_f32', 'srhip_degrade_noise_u8'])
def test_new_entry_points_are_declared_alike(lib, name):
    from sradsgan_amd import _hip
    assert _hip.SIGNATURES[name] == _header_signature(name)
    assert getattr(lib, name) is not None
    assert lib.srhip_abi_version() == 14                                             # additive: the version does not move


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)                              # never dereferenced: refused before any launch
    err = lib.srhip_last_error
    assert lib.srhip_blur_u8(None, one, two, 1, 8, 8, 3, 3, None) == -1 and b'null tensor' in err()
    assert lib.srhip_blur_u8(one, two, one, 1, 8, 8, 3, 3, None) == -1 and b'not in place' in err()
    assert lib.srhip_blur_u8(one, one, two, 1, 8, 8, 5, 3, None) == -1 and b'bad size' in err()
    assert lib.srhip_blur_u8(one, one, two, 0, 8, 8, 3, 3, None) == -1 and b'bad size' in err()
    for l in (0, 22, -3):
        assert lib.srhip_blur_u8(one, one, two, 1, 30, 30, 3, l, None) == -1 and b'outside 1..21' in err()
    assert lib.srhip_blur_u8(one, one, two, 1, 10, 30, 3, 21, None) == -1 and b'reflection padding' in err()   # lo = 10 >= h
    assert lib.srhip_blur_u8(one, one, two, 1, 30, 2, 3, 4, None) == -1 and b'reflection padding' in err()     # lo = 2 >= w
    strides = (ctypes.c_long * 4)(192, 64, 8, 1)
    neg = (ctypes.c_long * 4)(192, 64, -8, 1)
    assert lib.srhip_blur_f32(one, strides, one, 1, two, None, 1, 3, 8, 8, 3, None) == -1 and b'null tensor' in err()
    assert lib.srhip_blur_f32(one, strides, one, 1, one, strides, 1, 3, 8, 8, 3, None) == -1 and b'not in place' in err()
    assert lib.srhip_blur_f32(one, neg, one, 1, two, strides, 1, 3, 8, 8, 3, None) == -1 and b'negative stride' in err()
    assert lib.srhip_blur_f32(one, strides, one, 1, two, strides, 1, 3, 8, 8, 22, None) == -1 and b'outside 1..21' in err()
    assert lib.srhip_blur_f32(one, strides, one, 0, two, strides, 1, 3, 8, 5, 11, None) == -1 and b'reflection padding' in err()
    assert lib.srhip_degrade_noise_u8(None, one, None, two, 1, 8, 8, 3, 1, 0, 0, None) == -1 and b'null tensor' in err()
    assert lib.srhip_degrade_noise_u8(one, one, one, two, 1, 8, 8, 3, 1, 0, 0, None) == -1 and b'not both' in err()
    assert lib.srhip_degrade_noise_u8(one, one, None, two, 1, 8, 8, 3, 0, 0, 0, None) == -1 and b'needs z or drawn' in err()
    assert lib.srhip_degrade_noise_u8(one, one, None, two, 1, 8, 8, 5, 1, 0, 0, None) == -1 and b'bad size' in err()
