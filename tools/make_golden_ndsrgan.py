"""Generate tests/golden/ndsrgan_x{2,3,4,8,9}.npz by running the REFERENCE model/ndsrgan.py GeneratorResNet and Discriminator (build
container only; the stub import of oracle/make_golden.py).  The reference hard-codes 23 DCRDBs, so the full-depth generator runs at
a tiny input (2, 3, 16, 14) (a 10-pixel side would leave D no output at x2); parameters from the deterministic filler keyed by state_dict name, inputs from det_fill.  Stored: the
output, the three SmoothL1 terms of loss_G (pixel, content on the structural VGG stand-in oracle.sradsgan_ref.FeatureExtractor,
GAN on D(gen)), digests of the generator's gradients of loss_G, the sorted key lists, D's output and BatchNorm running statistics
after one call on a (2, 3, 40, 40) input, and two iterations of the reference's step (ndsrgan.py:414-456: SmoothL1 losses, Adam
lr 2e-4, betas (0.9, 0.99)): both losses before each step, weight and BN-buffer digests after it (x2 only).  Fixture size: the output, gradients and weights are stored as digests, the gradient and weight digests
concatenated in named_parameters() order (tied parameters once), the BN buffers in sorted key order."""
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

SHAPE, DSHAPE = (2, 3, 16, 14), (2, 3, 40, 40)      # x2: 32 x 28 -> D's patch is 2 x 1
STEP_SCALES = (2,)


def step_digest(t):
    """the smaller digest of the post-step weights (tests/ndsrgan_ref.py uses the same)"""
    return O.digest(t, full_max=16, nsample=8)


def grad_digest(t):
    return O.digest(t, full_max=16, nsample=8)


def out_digest(t):
    return O.digest(t, full_max=4096, nsample=4096)


def import_ndsrgan():
    import_reference()
    data = importlib.import_module('data.data')
    for name in ('get_training_datasets', 'get_test_datasets', 'get_RGB_trainDataset', 'get_RGB_testDataset'):
        if not hasattr(data, name):
            setattr(data, name, None)
    return importlib.import_module('model.ndsrgan')


def build(nd, scale):
    G = nd.GeneratorResNet(in_channels=3, out_channels=3, nf=64, nc=32, upscale_factor=scale)
    O.det_init_(G, prefix='N.')
    D = nd.Discriminator()
    O.det_init_(D, prefix='ND.')
    Fx = O.FeatureExtractor()
    O.det_init_(Fx, prefix='NF.')
    return G, D, Fx


def inputs(scale):
    x = O.det_fill('ndsrgan.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('ndsrgan.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
    return x, t


def unique_params(net):
    seen, out = set(), []
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append((k, p))
    return out


def k_(k):
    return k.replace('.', '__')


def main():
    torch.set_num_threads(8)
    nd = import_ndsrgan()
    sl1 = torch.nn.SmoothL1Loss()
    for scale in (2, 3, 4, 8, 9):
        G, D, Fx = build(nd, scale)
        x, t = inputs(scale)
        y = G(x)
        v = D(y)
        pixel, content, gan = sl1(y, t), sl1(Fx(y), Fx(t).detach()), sl1(v, torch.ones_like(v))
        loss_G = 1e-2 * pixel + content + 2.5e-3 * gan
        loss_G.backward()
        out = {'y': out_digest(y), 'pixel': np.float32(pixel.item()), 'content': np.float32(content.item()),
               'gan': np.float32(gan.item()), 'keys': np.array(sorted(G.state_dict().keys())),
               'dkeys': np.array(sorted(D.state_dict().keys()))}
        out['grads'] = np.concatenate([grad_digest(p.grad) for _, p in unique_params(G)])
        if scale == 2:
            _, D2, _ = build(nd, scale)
            xd = O.det_fill('ndsrgan.d', DSHAPE, 0.5, 0.5)
            out['d_x_out'] = D2(xd).detach().numpy()
            for k, b in D2.state_dict().items():
                if 'running' in k:
                    out['d_buf__' + k_(k)] = b.numpy()
        if scale in STEP_SCALES:
            G, D, Fx = build(nd, scale)
            opt_G = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.99))
            opt_D = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.99))
            losses = []
            for it in range(2):
                opt_G.zero_grad()
                gen = G(x)
                v = D(gen)
                lg = 1e-2 * sl1(gen, t) + sl1(Fx(gen), Fx(t).detach()) + 2.5e-3 * sl1(v, torch.ones_like(v))
                lg.backward()
                opt_G.step()
                opt_D.zero_grad()
                vr = D(t)
                vf = D(gen.detach())
                ld = (sl1(vr, torch.ones_like(vr)) + sl1(vf, torch.zeros_like(vf))) / 2
                ld.backward()
                opt_D.step()
                losses.append([lg.item(), ld.item()])
                for net, tag in ((G, 'G'), (D, 'D')):
                    out['step%d_%s' % (it, tag)] = np.concatenate([step_digest(p.detach()) for _, p in unique_params(net)])
                out['step%d_Dbuf' % it] = np.concatenate([step_digest(b) for k, b in sorted(D.state_dict().items()) if 'running' in k])
            out['steps'] = np.array(losses, dtype=np.float32)
        path = os.path.join(ROOT, 'tests', 'golden', 'ndsrgan_x%d.npz' % scale)
        np.savez_compressed(path, **out)
        print('x%d: y %s pixel %.6f content %.6f gan %.6f, %.1f KB' % (scale, tuple(y.shape), pixel.item(), content.item(), gan.item(),
                                                                       os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
