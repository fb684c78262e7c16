"""Generate tests/golden/dssr_x{2,3,4,8,9}.npz by running the REFERENCE model/dssr.py GeneratorResNet (build container only; the
stub import of oracle/make_golden.py).  Config: 2 residual groups x 2 WABs, input (2, 3, 12, 10); parameters from the deterministic
filler keyed by state_dict name, inputs from det_fill.  Stored: the output, the L1 and MSE losses (dssr.py:266-269), digests of the
parameter gradients of the L1 loss, the sorted key list, and two iterations of the reference's step (loss_G, backward, Adam lr 1e-4,
betas (0.9, 0.999): main_dssr.py defaults) for each loss: the loss before each step and weight digests after it."""
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

GROUPS, BLOCKS, SHAPE = 2, 2, (2, 3, 12, 10)


def step_digest(t):
    """the smaller digest of the post-step weights (tests/dssr_ref.py uses the same)"""
    return O.digest(t, full_max=512, nsample=256)


def import_dssr():
    import_reference()
    data = importlib.import_module('data.data')
    for name in ('get_training_datasets', 'get_test_datasets'):     # imported by dssr.py:34, absent from data/data.py
        if not hasattr(data, name):
            setattr(data, name, None)
    return importlib.import_module('model.dssr')


def build(dssr, scale):
    net = dssr.GeneratorResNet(dssr.ResGroup, n_residual_blocks=GROUPS, n_basic_blocks=BLOCKS, upscale_factor=scale)
    O.det_init_(net, prefix='D.')
    return net


def inputs(scale):
    x = O.det_fill('dssr.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('dssr.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
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
    dssr = import_dssr()
    for scale in (2, 3, 4, 8, 9):
        net = build(dssr, scale)
        x, t = inputs(scale)
        y = net(x)
        l1 = torch.nn.functional.l1_loss(y, t)
        mse = torch.nn.functional.mse_loss(y, t)
        l1.backward()
        out = {'y': y.detach().numpy(), 'loss_l1': np.float32(l1.item()), 'loss_mse': np.float32(mse.item()),
               'keys': np.array(sorted(net.state_dict().keys()))}
        for k, p in unique_params(net):
            out['grad__' + k.replace('.', '__')] = O.digest(p.grad)
        for norm in ('L1', 'L2'):
            net = build(dssr, scale)
            opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.9, 0.999))
            crit = torch.nn.L1Loss() if norm == 'L1' else torch.nn.MSELoss()
            losses = []
            for it in range(2):
                opt.zero_grad()
                loss = crit(net(x), t)
                loss.backward()
                opt.step()
                losses.append(loss.item())
                for k, p in unique_params(net):
                    out['step%d_%s__%s' % (it, norm, k.replace('.', '__'))] = step_digest(p.detach())
            out['steps_%s' % norm] = np.array(losses, dtype=np.float32)
        path = os.path.join(ROOT, 'tests', 'golden', 'dssr_x%d.npz' % scale)
        np.savez_compressed(path, **out)
        print('x%d: y %s l1 %.6f mse %.6f, %d params, %.1f KB' % (scale, tuple(y.shape), l1.item(), mse.item(),
                                                               len(unique_params(net)), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
