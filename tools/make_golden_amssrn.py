"""Generate tests/golden/amssrn_x{2,3,4,8,9}.npz by running the REFERENCE model/amssrn.py GeneratorResNet (build container only; the
stub import of oracle/make_golden.py).  Parameters from the deterministic filler keyed by state_dict name (prefix 'A.'), then four
values set so that every branch is live: one RB PReLU slope negative, one zero, one channel-attention PReLU slope negative, gamma
0.5 (the filler's value, non-zero).  Input (2, 3, 13, 14): odd quadrants at every scale.  Stored: an output digest, the L1 and MSE
losses, digests of the L1 loss's gradients in named_parameters() order (tied parameters once), the sorted key list and the
parameter names, and at x2 two iterations of the reference's step (L1, Adam lr 1e-4, betas (0.9, 0.999)): the loss before each step
and weight digests after it."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from oracle.make_golden import import_reference  # noqa: E402

SHAPE = (2, 3, 13, 14)
STEP_SCALES = (2,)
SLOPES = {'body.0.c1.rb.1.weight': -0.3, 'body.1.c2.rb.1.weight': 0.0, 'body.4.ca.conv_du.1.weight': -0.2,
          'body.5.aspp.act.weight': 0.1}


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def out_digest(t):
    return O.digest(t, full_max=4096, nsample=4096)


def init_(G):
    """the fixtures' parameters (tests/test_amssrn_cpu.py applies the same to the restatement and the HIP model)"""
    O.det_init_(G, prefix='A.')
    params = dict(G.named_parameters())
    with torch.no_grad():
        for k, v in SLOPES.items():
            params[k].fill_(v)
    return G


def import_amssrn():
    import_reference()
    for name in ('skimage', 'skimage.measure', 'utils', 'utils.utils', 'utils.logger'):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                import types
                m = types.ModuleType(name)
                m.__path__ = []
                sys.modules[name] = m
    sm = sys.modules['skimage.measure']
    for n in ('compare_ssim', 'compare_mse', 'compare_psnr', 'compare_nrmse'):
        setattr(sm, n, getattr(sm, n, None))
    lg = sys.modules['utils.logger']
    for n in ('Logger', 'PrintLogger'):
        setattr(lg, n, getattr(lg, n, None))
    data = importlib.import_module('data.data')
    for name in ('get_training_datasets', 'get_test_datasets', 'get_RGB_trainDataset', 'get_RGB_testDataset'):
        if not hasattr(data, name):
            setattr(data, name, None)
    return importlib.import_module('model.amssrn')


def inputs(scale):
    x = O.det_fill('amssrn.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('amssrn.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
    return x, t


def unique_params(net):
    seen, out = set(), []
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append((k, p))
    return out


def main():
    torch.set_num_threads(8)
    am = import_amssrn()
    for scale in (2, 3, 4, 8, 9):
        G = init_(am.GeneratorResNet(scale=scale))
        x, t = inputs(scale)
        y = G(x)
        l1 = torch.nn.functional.l1_loss(y, t)
        mse = torch.nn.functional.mse_loss(y, t)
        l1.backward()
        ups = unique_params(G)
        out = {'y': out_digest(y), 'l1': np.float32(l1.item()), 'mse': np.float32(mse.item()),
               'keys': np.array(sorted(G.state_dict().keys())), 'names': np.array([k for k, _ in ups]),
               'grads': np.concatenate([digest(p.grad) for _, p in ups])}
        if scale in STEP_SCALES:
            G = init_(am.GeneratorResNet(scale=scale))
            opt = torch.optim.Adam(G.parameters(), lr=1e-4, betas=(0.9, 0.999))
            losses = []
            for it in range(2):
                opt.zero_grad()
                lg = torch.nn.functional.l1_loss(G(x), t)
                lg.backward()
                opt.step()
                losses.append(lg.item())
                out['step%d' % it] = np.concatenate([digest(p.detach()) for _, p in unique_params(G)])
            out['steps'] = np.array(losses, dtype=np.float32)
        path = os.path.join(ROOT, 'tests', 'golden', 'amssrn_x%d.npz' % scale)
        np.savez_compressed(path, **out)
        print('x%d: y %s l1 %.6f mse %.6f, %d keys, %.1f KB' % (scale, tuple(y.shape), l1.item(), mse.item(), len(out['keys']),
                                                                 os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
