"""Generate tests/golden/hat_*.npz by running the REFERENCE model/hat.py GeneratorResNet on the CPU (build container only; the stub
import of tools/make_golden_amssrn.py plus a basicsr.archs.arch_util stub with to_2tuple / trunc_normal_, and Tensor / Variable types
on the stubbed tensorflow module so that einops picks its torch backend).  Configuration: the real width (96 channels, 6 heads) with
depths (2, 2), eval mode (drop path off), parameters from tests/hat_ref.init_ (the deterministic filler keyed by state_dict name).
Cases: x2 / x3 / x4 / x8 at window 9 on a (2, 3, 18, 27) input (shifted windows and every mask region), x3 / x9 at window 8 on
(2, 3, 16, 24), and x4 at window 9 on (1, 3, 13, 14) (reflect padding to 18 x 18).  Stored: an output digest, the L1 and MSE losses
against a target of the output's shape, digests of the L1 loss's gradients in named_parameters() order (tied parameters once), the
sorted key list and the parameter names, and the parameter count and key list of the full configuration (depths (6,) * 6) at the
case's scale and window."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import hat_ref as R  # noqa: E402

DEPTHS = (2, 2)
# name -> (scale, window, input shape)
CASES = {
    'x2': (2, 9, (2, 3, 18, 27)),
    'x3': (3, 9, (2, 3, 18, 27)),
    'x4': (4, 9, (2, 3, 18, 27)),
    'x8': (8, 9, (2, 3, 18, 27)),
    'x3w8': (3, 8, (2, 3, 16, 24)),
    'x9w8': (9, 8, (2, 3, 16, 24)),
    'x4pad': (4, 9, (1, 3, 13, 14)),
}


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def out_digest(t):
    return O.digest(t, full_max=4096, nsample=4096)


def import_hat():
    from make_golden_amssrn import import_amssrn
    import_amssrn()
    tf = sys.modules.get('tensorflow')
    if tf is not None:
        for n in ('Tensor', 'Variable'):
            if not hasattr(tf, n):
                setattr(tf, n, type(n, (), {}))
    for name in ('basicsr', 'basicsr.archs', 'basicsr.archs.arch_util'):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    au = sys.modules['basicsr.archs.arch_util']
    au.to_2tuple = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    au.trunc_normal_ = lambda t, mean=0., std=1., a=-2., b=2.: torch.nn.init.trunc_normal_(t, mean, std, a, b)
    return importlib.import_module('model.hat')


def unique_params(net):
    seen, out = set(), []
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append((k, p))
    return out


def main():
    torch.set_num_threads(8)
    hat = import_hat()
    for name, (scale, ws, shape) in CASES.items():
        G = R.init_(hat.GeneratorResNet(upscale=scale, window_size=ws, depths=DEPTHS, num_heads=(6,) * len(DEPTHS)))
        G.eval()
        x, t = R.inputs(name, shape, scale, ws)
        y = G(x)
        l1 = torch.nn.functional.l1_loss(y, t)
        mse = torch.nn.functional.mse_loss(y, t)
        l1.backward()
        ups = unique_params(G)
        full = hat.GeneratorResNet(upscale=scale, window_size=ws)
        out = {'y': out_digest(y), 'y_shape': np.array(y.shape), 'l1': np.float32(l1.item()), 'mse': np.float32(mse.item()),
               'keys': np.array(sorted(G.state_dict().keys())), 'names': np.array([k for k, _ in ups]),
               'grads': np.concatenate([digest(p.grad) for _, p in ups]),
               'rpi_sa': G.relative_position_index_SA.numpy().astype(np.int16),
               'rpi_oca': G.relative_position_index_OCA.numpy().astype(np.int16),
               'mask': G.calculate_mask((shape[2] + (-shape[2]) % ws, shape[3] + (-shape[3]) % ws)).numpy().astype(np.int8),
               'full_params': np.int64(sum(p.numel() for _, p in unique_params(full))),
               'full_keys': np.array(sorted(full.state_dict().keys()))}
        path = os.path.join(ROOT, 'tests', 'golden', 'hat_%s.npz' % name)
        np.savez_compressed(path, **out)
        print('%s: y %s l1 %.6f mse %.6f, %d keys, full %d params, %.1f KB' % (
            name, tuple(y.shape), float(out['l1']), float(out['mse']), len(out['keys']), int(out['full_params']),
            os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
