"""Generate tests/golden/drcan_x{2,3,4,8,9}.npz by running the REFERENCE model/drcan.py RCAN (build container only; the stub import
of oracle/make_golden.py, as tools/make_golden_amssrn.py).  Shortened depth: 2 residual groups x 2 RCABs, reduction 16 (the trainer's
value) at every scale, and at x2 also reduction 4 (RCAN's constructor default; keys prefixed 'r4_').  Parameters from the
deterministic filler keyed by state_dict name (prefix 'R.'): the channel-attention biases are non-zero.  Input (2, 3, 13, 14).
Stored: an output digest, the L1 and MSE losses, digests of the L1 loss's gradients in named_parameters() order, the sorted key
list and the parameter names, and the parameter count of the trainer's full configuration (10 groups x 20 RCABs, reduction 16)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import sradsgan_ref as O  # noqa: E402

SHAPE = (2, 3, 13, 14)
GROUPS, BLOCKS = 2, 2


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def out_digest(t):
    return O.digest(t, full_max=4096, nsample=4096)


def inputs(scale):
    x = O.det_fill('drcan.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('drcan.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
    return x, t


def import_drcan():
    import importlib
    from make_golden_amssrn import import_amssrn
    import_amssrn()                                   # the same stubs (skimage, utils, data) serve model/drcan.py
    return importlib.import_module('model.drcan')


def record(dr, scale, reduction):
    G = O.det_init_(dr.RCAN(n_colors=3, n_resgroups=GROUPS, n_resblocks=BLOCKS, reduction=reduction, scale=scale), prefix='R.')
    x, t = inputs(scale)
    y = G(x)
    l1 = torch.nn.functional.l1_loss(y, t)
    mse = torch.nn.functional.mse_loss(y, t)
    l1.backward()
    named = list(G.named_parameters())
    return y, {'y': out_digest(y), 'l1': np.float32(l1.item()), 'mse': np.float32(mse.item()),
               'keys': np.array(sorted(G.state_dict().keys())), 'names': np.array([k for k, _ in named]),
               'grads': np.concatenate([digest(p.grad) for _, p in named])}


def main():
    torch.set_num_threads(8)
    dr = import_drcan()
    for scale in (2, 3, 4, 8, 9):
        y, out = record(dr, scale, 16)
        full = dr.RCAN(n_colors=3, n_resgroups=10, n_resblocks=20, reduction=16, scale=scale)
        out['full_params'] = np.int64(sum(p.numel() for p in full.parameters()))
        out['full_keys'] = np.array(sorted(full.state_dict().keys()))
        if scale == 2:
            _, r4 = record(dr, scale, 4)
            out.update({'r4_' + k: v for k, v in r4.items()})
        path = os.path.join(ROOT, 'tests', 'golden', 'drcan_x%d.npz' % scale)
        np.savez_compressed(path, **out)
        print('x%d: y %s l1 %.6f mse %.6f, %d keys, full %d params, %.1f KB' % (
            scale, tuple(y.shape), float(out['l1']), float(out['mse']), len(out['keys']), int(out['full_params']),
            os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
