"""AMSSRN throughput on one GPU: the HIP training step (sradsgan_amd.model.amssrn.train_step, L1, Adam lr 1e-4) and generator
inference at x4, B = 16, 54 -> 216, next to an eager ATen run of the restatement (tests/amssrn_ref.py) with the same weights.
One JSON line.  Usage: python tools/time_amssrn.py [--batch 16] [--steps 10] [--warmup 3] [--no-eager]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import amssrn_ref as R  # noqa: E402


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
    from sradsgan_amd.model import amssrn as H
    dev = torch.device('cuda:0')
    ref = R.Generator(4)
    O.det_init_(ref, prefix='A.')
    x = O.det_fill('time.x', (a.batch, 3, 54, 54), 0.5, 0.5).to(dev)
    t = O.det_fill('time.t', (a.batch, 3, 216, 216), 0.5, 0.5).to(dev)
    G = H.GeneratorResNet(scale=4)
    G.load_state_dict(ref.state_dict(), strict=True)
    G.to(dev)
    opt = torch.optim.Adam(G.parameters(), lr=1e-4, betas=(0.9, 0.999))
    train_ms = timed(lambda: H.train_step(G, opt, x, t), a.steps, a.warmup)

    def infer():
        with torch.no_grad():
            G(x)
    infer_ms = timed(infer, a.steps, a.warmup)
    out = {'metric': 'AMSSRN x4 img/s (B=%d, 54->216)' % a.batch, 'train_img_s': round(a.batch * 1000.0 / train_ms, 1),
           'train_ms': round(train_ms, 2), 'infer_img_s': round(a.batch * 1000.0 / infer_ms, 1), 'infer_ms': round(infer_ms, 2)}
    if not a.no_eager:
        E = ref.to(dev).to(memory_format=torch.channels_last)
        eopt = torch.optim.Adam(E.parameters(), lr=1e-4, betas=(0.9, 0.999))

        def estep():
            eopt.zero_grad(set_to_none=True)
            R.loss(E(x), t).backward()
            eopt.step()

        def einfer():
            with torch.no_grad():
                E(x)
        e_train = timed(estep, a.steps, a.warmup)
        e_infer = timed(einfer, a.steps, a.warmup)
        out.update({'eager_train_img_s': round(a.batch * 1000.0 / e_train, 1), 'eager_infer_img_s': round(a.batch * 1000.0 / e_infer, 1),
                    'train_speedup': round(e_train / train_ms, 2), 'infer_speedup': round(e_infer / infer_ms, 2)})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
