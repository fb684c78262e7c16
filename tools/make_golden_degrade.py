"""Generate tests/golden/degrade.npz by running the REFERENCE's degradation (model/util.py: random_batch_kernel, BatchBlur,
to_pil_image, SRMDPreprocessing(noise=False), b_GaussianNoising), imported at run time through oracle/make_golden.py's stub import
(build container only); nothing of its text is copied.  util.py needs a few more absent modules stubbed (h5py, skimage.io,
skimage.transform, matplotlib; accimage is NOT stubbed, the reference handles its absence), `collections.Iterable` (removed from
Python 3.10) and contiguous NCHW inputs (BatchBlur uses .view).

Cases (l, scale, H x W), B = 2, rate_iso = 0.5 so that both kernel kinds occur: (21, 3, 24 x 21), (11, 2, 24 x 22), (4, 4, 24 x 20).
Recorded per case: the uint8 source, the drawn kernels with their (sig_x, sig_y, theta, isotropic) -- recovered by reseeding numpy
and replaying the draws -- BatchBlur's fp32 output, its to_pil_image bytes, the LR bytes of SRMDPreprocessing(noise=False) for the
same kernels, and one b_GaussianNoising call on that LR with its z (recovered the same way), levels and output.

The recorder also checks that the float32 restatement tests/degrade_ref.py reproduces the reference's blurred bytes and LR bytes
EXACTLY for every case; a seed at which a case fails that (a product within an fp32 rounding of a byte boundary, summed in another
order by the reference's convolution) is passed over for the next one.  The fixture therefore needs no byte tolerance."""
import collections
import collections.abc
import importlib
import importlib.machinery as mach
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle.make_golden import import_reference  # noqa: E402
from tests import degrade_ref as R  # noqa: E402

CASES = ((21, 3, 24, 21), (11, 2, 24, 22), (4, 4, 24, 20))
B, C, RATE_ISO, SIG_MIN, SIG_MAX, SCALING = 2, 3, 0.5, 0.2, 4.0, 3


def import_util():
    import_reference()

    class _Any:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return _Any()

        def __getattr__(self, k):
            return _Any()

    for name in ('h5py', 'skimage.io', 'skimage.transform', 'matplotlib', 'matplotlib.pyplot'):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            m.__spec__ = mach.ModuleSpec(name, None)
            m.__getattr__ = lambda k: _Any()
            sys.modules[name] = m
    if not hasattr(collections, 'Iterable'):
        collections.Iterable = collections.abc.Iterable
    return importlib.import_module('model.util')


def replay_kernel_draws(seed):
    """(sig_x, sig_y, theta, isotropic) per sample from numpy's stream at `seed`, in the order random_batch_kernel consumes it."""
    np.random.seed(seed)
    out = np.zeros((B, 4), np.float64)
    for b in range(B):
        if np.random.random() < RATE_ISO:
            sig = np.random.random() * (SIG_MAX - SIG_MIN) + SIG_MIN
            out[b] = (sig, sig, 0.0, 1.0)
        else:
            theta = np.random.random() * math.pi * 2 - math.pi
            sx = np.random.random() * (SIG_MAX - SIG_MIN) + SIG_MIN
            sy = np.clip(np.random.random() * SCALING * sx, SIG_MIN, SIG_MAX)
            out[b] = (sx, sy, theta, 0.0)
    return out


def record_case(U, l, scale, H, W, seed):
    rng = np.random.RandomState(1000 + seed)
    src = rng.randint(0, 256, (B, H, W, C)).astype(np.uint8)
    x = torch.from_numpy(src).permute(0, 3, 1, 2).contiguous().float().div(255)
    # the reference draws inside SRMDPreprocessing; seeding numpy before each use gives the same kernels to every stage
    np.random.seed(seed)
    kernels = U.random_batch_kernel(B, l=l, sig_min=SIG_MIN, sig_max=SIG_MAX, rate_iso=RATE_ISO, scaling=SCALING, tensor=True)
    params = replay_kernel_draws(seed)
    if len(set(params[:, 3])) != 2:
        return None                                                    # both kernel kinds must occur
    blurred = U.BatchBlur(l=l)(x, kernels)
    blurred_u8 = np.stack([np.stack([np.asarray(U.to_pil_image(blurred[b, c:c + 1])) for c in range(C)], -1) for b in range(B)])
    pre = U.SRMDPreprocessing(scale, random=True, pca_matrix=torch.zeros(l * l, 4), kernel=l, noise=False, sig_min=SIG_MIN,
                              sig_max=SIG_MAX, rate_iso=RATE_ISO, scaling=SCALING)
    np.random.seed(seed)
    lr, _, used = pre(x, kernel=True)
    assert torch.equal(used, kernels)
    lr_u8 = (lr * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    assert torch.equal(torch.from_numpy(lr_u8).permute(0, 3, 1, 2).float().div(255), lr)     # to_tensor of bytes: nothing lost
    # the restatement must give the reference's bytes exactly, or this seed is passed over
    k = kernels.numpy()
    mine_u8 = R.blur_u8(src, k)
    mine_lr = R.pil_resize(mine_u8, int(H / scale), int(W / scale))
    if not (np.array_equal(mine_u8, blurred_u8) and np.array_equal(mine_lr, lr_u8)):
        return None
    levels = np.array([[0.05], [0.0]], np.float32)                     # one noisy, one clean sample
    np.random.seed(seed + 7)
    noisy = U.b_GaussianNoising(lr, torch.from_numpy(levels))
    np.random.seed(seed + 7)
    z = np.random.normal(loc=0.0, scale=1.0, size=tuple(lr.shape)).astype(np.float32)
    return {'src': src, 'kernels': k, 'params': params, 'blur_f32': blurred.numpy(), 'blur_u8': blurred_u8, 'lr_u8': lr_u8,
            'noise_levels': levels.reshape(B), 'noise_z': z, 'noise_out': noisy.numpy(), 'seed': np.int64(seed)}


def main():
    torch.set_num_threads(4)
    U = import_util()
    out = {'cases': np.array(CASES, np.int32)}
    for l, scale, H, W in CASES:
        for seed in range(l, l + 200):                                  # a different stream per case
            rec = record_case(U, l, scale, H, W, seed)
            if rec is not None:
                break
        else:
            raise SystemExit('no seed found for l = %d' % l)
        print('l %2d x%d %dx%d: seed %d, params %s' % (l, scale, H, W, seed, np.round(rec['params'], 3).tolist()))
        for key, v in rec.items():
            out['l%d_%s' % (l, key)] = v
    path = os.path.join(ROOT, 'tests', 'golden', 'degrade.npz')
    np.savez_compressed(path, **out)
    print('%s: %.1f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
