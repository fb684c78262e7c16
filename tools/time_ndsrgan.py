"""NDSRGAN throughput on one GPU: the HIP training step (sradsgan_amd.model.ndsrgan.train_step) and generator inference at x4,
B = 16, 54 -> 216, next to an eager ATen restatement (tests/ndsrgan_ref.py) with the same weights.  One JSON line.
Usage: python tools/time_ndsrgan.py [--batch 16] [--steps 10] [--warmup 3] [--no-eager]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import ndsrgan_ref as R  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-eager', action='store_true')
    a = ap.parse_args()
    from sradsgan_amd.model import ndsrgan as H
    dev = torch.device('cuda:0')
    refs = [R.Generator(4), R.Discriminator(), O.FeatureExtractor()]
    for m, p in zip(refs, ('N.', 'ND.', 'NF.')):
        O.det_init_(m, prefix=p)
    x = O.det_fill('time.x', (a.batch, 3, 54, 54), 0.5, 0.5).to(dev)
    t = O.det_fill('time.t', (a.batch, 3, 216, 216), 0.5, 0.5).to(dev)
    G, D, Fx = H.GeneratorResNet(upscale_factor=4), H.Discriminator(), H.FeatureExtractor()
    for m, r in zip((G, D, Fx), refs):
        m.load_state_dict(r.state_dict(), strict=True)
        m.to(dev)
    for p in Fx.parameters():
        p.requires_grad_(False)
    opt_G = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.99))
    opt_D = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.99))
    res = {'batch': a.batch, 'scale': 4, 'hr': 216}
    ms = timed(lambda: H.train_step(G, D, Fx, opt_G, opt_D, x, t), a.steps, a.warmup)
    res['hip_train_ms'], res['hip_train_img_s'] = round(ms, 3), round(a.batch * 1000.0 / ms, 1)
    with torch.no_grad():
        ms = timed(lambda: G(x), a.steps, a.warmup)
    res['hip_infer_ms'], res['hip_infer_img_s'] = round(ms, 3), round(a.batch * 1000.0 / ms, 1)
    if not a.no_eager:
        eG, eD, eF = (m.to(dev) for m in refs)
        for p in eF.parameters():
            p.requires_grad_(False)
        eopt_G = torch.optim.Adam(eG.parameters(), lr=2e-4, betas=(0.9, 0.99))
        eopt_D = torch.optim.Adam(eD.parameters(), lr=2e-4, betas=(0.9, 0.99))
        ms = timed(lambda: R.train_iteration(eG, eD, eF, eopt_G, eopt_D, x, t), a.steps, a.warmup)
        res['eager_train_ms'], res['eager_train_img_s'] = round(ms, 3), round(a.batch * 1000.0 / ms, 1)
        with torch.no_grad():
            ms = timed(lambda: eG(x), a.steps, a.warmup)
        res['eager_infer_ms'], res['eager_infer_img_s'] = round(ms, 3), round(a.batch * 1000.0 / ms, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
