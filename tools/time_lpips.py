"""LPIPS timing on one GPU at the validation shape (216 x 216, validation batch 16; SR and bicubic against HR, i.e. 48 images through
the backbone and 32 pairs): (a) the HIP path (sradsgan_amd.lpips.LPIPS.pairs), (b) eager ATen fp32 channels-last on the same GPU with the
same weights (the restatement tests/lpips_ref.py), batched and one image pair at a time as the reference's loop calls it
(sradsgan.py:1326-1332), and (c) validate.evaluate() at x4 with and without LPIPS, eager and replayed from a hipGraph.  Every shape is
warmed up first; each figure is timed with device events over a window of at least --window seconds.  One JSON line.
Usage: python tools/time_lpips.py [--batch 16] [--crop 216] [--window 2] [--no-eager] [--math bf16x3]
(`rocprofv3 --kernel-trace --stats -- python tools/time_lpips.py --no-eager --no-evaluate` for the per-kernel table)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lpips_ref as R  # noqa: E402


def timed(fn, window_s, warmup):
    """ms per call: warm-up calls, then one probe call to size the window, then >= window_s seconds between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    n = max(3, int(window_s * 1000.0 / max(t0.elapsed_time(t1), 1e-3)) + 1)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--crop', type=int, default=216)
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--window', type=float, default=2.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--math', default='bf16x3')
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--no-evaluate', action='store_true')
    a = ap.parse_args()
    from sradsgan_amd import ops, trainer as T, validate as V
    from sradsgan_amd.lpips import LPIPS
    dev = torch.device('cuda:0')
    B, crop = a.batch, a.crop
    G = np.load(R.GOLDEN)
    sd, lin = R.alexnet_state_dict(), R.lin_state_dict(G)
    model = LPIPS()
    model.load_torchvision_alexnet(sd)
    model.load_lin(lin)
    model = model.to(dev)
    cl = torch.channels_last
    hr = R.hash_image((B, 3, crop, crop), 201).to(dev).contiguous(memory_format=cl)
    sr = (0.75 * hr + 0.25 * R.hash_image((B, 3, crop, crop), 202).to(dev)).contiguous(memory_format=cl)
    bc = (0.5 * hr + 0.5 * R.hash_image((B, 3, crop, crop), 203).to(dev)).contiguous(memory_format=cl)
    pairs = [(i, B + i) for i in range(B)] + [(i, 2 * B + i) for i in range(B)]
    ops.set_conv_math(a.math)
    hip_ms, n_hip = timed(lambda: model.pairs([hr, sr, bc], pairs), a.window, a.warmup)
    out = {'metric': 'LPIPS ms per validation batch (B=%d, %dx%d, SR and bicubic vs HR, %s)' % (B, crop, crop, a.math),
           'hip_ms': round(hip_ms, 3), 'hip_calls': n_hip}
    if not a.no_eager:
        sdd = {k: v.to(dev) for k, v in sd.items()}
        for k in list(sdd):
            if sdd[k].dim() == 4:
                sdd[k] = sdd[k].contiguous(memory_format=cl)
        lins = [lin['lin%d.model.1.weight' % k].flatten().to(dev) for k in range(5)]

        def eager_batched():
            with torch.no_grad():
                t = R.taps(torch.cat([hr, sr, bc]), sdd)
                return sum(R.head(torch.cat([f[:B], f[:B]]), f[B:], w) for f, w in zip(t, lins))

        def eager_per_image():
            with torch.no_grad():
                return [R.lpips(x[i:i + 1], hr[i:i + 1], sdd, lins, dtype=torch.float32) for x in (sr, bc) for i in range(B)]
        e_b, _ = timed(eager_batched, a.window, a.warmup)
        e_1, _ = timed(eager_per_image, a.window, a.warmup)
        got = model.pairs([hr, sr, bc], pairs)
        rel = float(((got - eager_batched().double()).abs() / got).max())
        out.update({'eager_batched_ms': round(e_b, 3), 'eager_per_image_ms': round(e_1, 3), 'speedup_vs_batched': round(e_b / hip_ms, 2),
                    'speedup_vs_per_image': round(e_1 / hip_ms, 2), 'hip_vs_eager_rel': float('%.2e' % rel)})
    if not a.no_evaluate:
        args = T.default_args(scale_factor=a.scale)
        net = T.SRADSGAN(args)
        torch.manual_seed(0)
        gen = net._new_generator()
        gen.apply(T.weights_init_normal)
        gen = gen.to(dev).eval()
        lr = torch.nn.functional.avg_pool2d(hr, a.scale)
        ev0, _ = timed(lambda: V.evaluate(gen, lr, hr, a.scale, bicubic=bc), a.window, a.warmup)
        ev1, _ = timed(lambda: V.evaluate(gen, lr, hr, a.scale, bicubic=bc, lpips=model), a.window, a.warmup)
        g0, g1 = V.GraphedEvaluator(gen, a.scale), V.GraphedEvaluator(gen, a.scale, lpips=model)
        gr0, _ = timed(lambda: g0(lr, hr, bc), a.window, a.warmup)
        gr1, _ = timed(lambda: g1(lr, hr, bc), a.window, a.warmup)
        out.update({'evaluate_x%d_ms' % a.scale: round(ev0, 3), 'evaluate_x%d_lpips_ms' % a.scale: round(ev1, 3),
                    'graphed_x%d_ms' % a.scale: round(gr0, 3), 'graphed_x%d_lpips_ms' % a.scale: round(gr1, 3)})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
