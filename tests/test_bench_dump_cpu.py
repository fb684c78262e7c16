"""bench.dump_outputs -- what `bench.py --dump-outputs DIR` writes after the timed steps -- on CPU tensors: names, dtypes,
values, and the fixed sample that keeps a large output under 64 MB."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    gen = torch.Generator().manual_seed(0)
    img = torch.rand(2, 3, 8, 8, generator=gen)
    out = {'loss_G': torch.tensor(0.25), 'gen_hr': img, 'sr': {'psnr': torch.tensor([30.5, 31.0], dtype=torch.float64)},
           'half': img.half()}
    bench.dump_outputs(str(tmp_path / 'd'), out)
    names = sorted(os.listdir(tmp_path / 'd'))
    assert names == ['gen_hr.npy', 'half.npy', 'loss_G.npy', 'sr.psnr.npy']
    g = np.load(tmp_path / 'd' / 'gen_hr.npy')
    assert g.dtype == np.float32 and g.shape == (2, 3, 8, 8) and np.array_equal(g, img.numpy())
    assert np.load(tmp_path / 'd' / 'loss_G.npy').dtype == np.float32
    assert float(np.load(tmp_path / 'd' / 'loss_G.npy')) == 0.25
    p = np.load(tmp_path / 'd' / 'sr.psnr.npy')
    assert p.dtype == np.float64 and p.tolist() == [30.5, 31.0]
    assert np.load(tmp_path / 'd' / 'half.npy').dtype == np.float32


def test_large_outputs_are_sampled_at_fixed_indices_under_64_mb(tmp_path):
    n = 5 * 2 ** 20                                           # 5 x 20 MB: over the limit together
    big = {'x%d' % i: torch.arange(n, dtype=torch.float32) + i for i in range(5)}
    big['loss'] = torch.tensor(1.5)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), big)
    total = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
    assert total <= bench.DUMP_LIMIT_BYTES
    a0 = np.load(tmp_path / 'a' / 'x0.npy')
    assert a0.shape == (bench.DUMP_SAMPLE_ELEMS,) and a0.dtype == np.float32
    assert np.all(np.diff(a0) > 0)                            # sorted distinct indices of the flattened array
    for i in range(5):                                        # the same indices for every array and every run
        ai = np.load(tmp_path / 'a' / ('x%d.npy' % i))
        assert np.array_equal(ai, a0 + i)
        assert np.array_equal(ai, np.load(tmp_path / 'b' / ('x%d.npy' % i)))
    assert float(np.load(tmp_path / 'a' / 'loss.npy')) == 1.5
