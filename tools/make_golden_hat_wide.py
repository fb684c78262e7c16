"""Generate tests/golden/hat180_*.npz and hat144_*.npz by running the REFERENCE model/hat.py GeneratorResNet on the CPU at the
published widths (build container only; the import stubs are tools/make_golden_hat.py's).  The layout is that of hat_*.npz: an
output digest, the L1 and MSE losses against a target of the output's shape, digests of the L1 loss's gradients in
named_parameters() order (tied parameters once), the sorted key list and the parameter names, the index buffers and the shift mask,
and the parameter count and key list of the FULL configuration (HAT: depths (6,) * 6 at 180 channels; HAT-S: the same at 144).
All cases use depths (2, 2), eval mode (drop path off) and parameters from tests/hat_ref.init_.  Fixtures hold arrays and name
lists only.

    hat180_x4     180 / 6 heads / window 16 / (compress 3, squeeze 30, mlp 2), x4, input (2, 3, 32, 48): 2 x 3 windows, every mask region
    hat144_x2     144 / 6 / 16 / (24, 24, 2), x2, input (1, 3, 32, 32): HAT-S, with CAB's 144 -> 6 -> 144 convs
    hat180_x4pad  as hat180_x4 on (1, 3, 20, 37): reflect padding to 32 x 48
    hat180_x3     180 / 6 / 16 / (3, 30, 2), x3, input (1, 3, 16, 32): one window row, no vertical neighbour"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden_hat import digest, import_hat, out_digest, unique_params  # noqa: E402
from tests import hat_ref as R  # noqa: E402
from tests import hat_wide_ref as W  # noqa: E402


def main():
    torch.set_num_threads(8)
    hat = import_hat()
    for name in W.CASES:
        scale, shape = W.CASES[name][1], W.CASES[name][2]
        kw = W.model_kwargs(name)
        ws = kw['window_size']
        G = R.init_(hat.GeneratorResNet(depths=W.DEPTHS, num_heads=(6,) * len(W.DEPTHS), **kw))
        G.eval()
        x, t = R.inputs(name, shape, scale, ws)
        y = G(x)
        l1 = torch.nn.functional.l1_loss(y, t)
        mse = torch.nn.functional.mse_loss(y, t)
        l1.backward()
        ups = unique_params(G)
        full = hat.GeneratorResNet(depths=(6,) * 6, num_heads=(6,) * 6, **kw)
        out = {'y': out_digest(y), 'y_shape': np.array(y.shape), 'l1': np.float32(l1.item()), 'mse': np.float32(mse.item()),
               'keys': np.array(sorted(G.state_dict().keys())), 'names': np.array([k for k, _ in ups]),
               'grads': np.concatenate([digest(p.grad) for _, p in ups]),
               'rpi_sa': G.relative_position_index_SA.numpy().astype(np.int16),
               'rpi_oca': G.relative_position_index_OCA.numpy().astype(np.int16),
               'mask': G.calculate_mask((shape[2] + (-shape[2]) % ws, shape[3] + (-shape[3]) % ws)).numpy().astype(np.int8),
               'full_params': np.int64(sum(p.numel() for _, p in unique_params(full))),
               'full_keys': np.array(sorted(full.state_dict().keys()))}
        path = os.path.join(ROOT, 'tests', 'golden', '%s.npz' % name)
        np.savez_compressed(path, **out)
        print('%s: y %s l1 %.6f mse %.6f, %d keys, full %d params, %.1f KB' % (
            name, tuple(y.shape), float(out['l1']), float(out['mse']), len(out['keys']), int(out['full_params']),
            os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
