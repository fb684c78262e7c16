"""Generate tests/golden/gdp_train.npz by running the REFERENCE GDP_x0/model/gdp_modules (unet.py, diffusion.py) on the CPU, loaded by
path exactly as tools/make_golden_gdp.py loads them: the small net (gdp_ref.SMALL, filled by gdp_ref.init_) through
GaussianDiffusion.p_losses on gdp_train_ref.train_inputs(), with t as torch.randint draws it under
torch.manual_seed(gdp_train_ref.TRAIN_SEED) and the noise that torch.randn_like returned, both stored.

  t, noise      the draws
  loss          p_losses' return value (sum-reduced), float32
  numel         b * c * h * w
  grad.<key>    O.digest(gradient of loss / numel, **gdp_train_ref.DIGEST) for every parameter of the U-Net

Prints the distance of the float64 restatement (tests/gdp_train_ref.py) from these float32 vectors and the float32 restatement's own
gradient score: the CPU test's bars are ten times the former."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import gdp_ref as R  # noqa: E402
from tests import gdp_train_ref as T  # noqa: E402
from make_golden_gdp import import_gdp  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def main():
    torch.set_num_threads(8)
    unet, diffusion = import_gdp()
    net = R.init_(unet.UNet(**R.SMALL)).train()
    G = diffusion.GaussianDiffusion(net, image_size=12, channels=3, loss_type='l2', conditional=True)
    G.set_loss('cpu')
    G.set_new_noise_schedule(T.TRAIN_SCHEDULE, 'cpu')
    hr, sr = T.train_inputs()
    drawn, randint = [], torch.randint

    def recording(*a, **k):
        v = randint(*a, **k)
        drawn.append(v.clone())
        return v

    torch.manual_seed(T.TRAIN_SEED)
    noise = torch.randn_like(hr)
    torch.randint = recording
    try:
        loss = G({'HR': hr, 'SR': sr, 'LR': sr}, noise)
    finally:
        torch.randint = randint
    t, = drawn
    numel = hr.numel()
    (loss / numel).backward()
    out = {'t': t.numpy(), 'noise': noise.numpy(), 'loss': np.float32(loss.item()), 'numel': np.int64(numel)}
    grads = {k: p.grad for k, p in net.named_parameters()}
    for k, g in grads.items():
        out['grad.' + k] = O.digest(g, **T.DIGEST)
    path = os.path.join(GOLD, 'gdp_train.npz')
    np.savez_compressed(path, **out)

    state = R.state(net, torch.float64)
    l64, g64 = T.loss_and_grads(state, hr, sr, t, noise, torch.float64)
    l32, g32 = T.loss_and_grads(state, hr, sr, t, noise, torch.float32)
    print('t = %s, loss / numel: reference %.6f, fp64 restatement %.6f (distance %.3e)' % (t.tolist(), loss.item() / numel, l64,
                                                                                        abs(loss.item() / numel - l64)))
    print('gradient score: reference fp32 vs fp64 restatement %.3e (%s), fp32 restatement vs fp64 %.3e' % (
        *T.grad_score(grads, g64), T.grad_score(g32, g64)[0]))
    print('the same on the stored digests: fp64 restatement vs reference %.3e (%s)' % T.digest_score(g64, out))
    gmax = max(float(g.abs().max()) for g in g64.values())
    small = min(float(g.abs().max()) for g in g64.values())
    print('%d tensors, largest |g| %.3e, smallest per-tensor max |g| %.3e' % (len(g64), gmax, small))
    print('gdp_train.npz: %.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
