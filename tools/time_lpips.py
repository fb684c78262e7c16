"""LPIPS timing on one GPU at the validation shape (216 x 216, validation batch 16; SR and bicubic against HR, i.e. 48 images through
the backbone and 32 pairs): (a) the HIP path (sradsgan_amd.lpips.LPIPS.pairs), (b) eager ATen fp32 channels-last on the same GPU with the
same weights (the restatement tests/lpips_ref.py), batched and one image pair at a time as the reference's loop calls it
(sradsgan.py:1326-1332), and (c) validate.evaluate() at x4 with and without LPIPS, eager and replayed from a hipGraph.  Every shape is
warmed up first; each figure is timed with device events over a window of at least --window seconds.  One JSON line.
--loss runs the loss leg instead (LPIPS.loss, the metric as a training term), at the training batch (--batch 32 there): (d) forward +
backward of LPIPS.loss against eager ATen autograd of the same composition (tests/lpips_loss_ref.py in fp32, channels-last) and (e) the
benchmark's training step (bench.build_networks, B x 54x54 -> 216x216) with weight_lpips 0 against 1 -- both pairs in one process,
alternated over --rounds rounds, every window listed so that drift between the rounds shows.
Usage: python tools/time_lpips.py [--batch 16] [--crop 216] [--window 2] [--no-eager] [--math bf16x3]
       python tools/time_lpips.py --loss [--batch 32] [--rounds 3] [--no-step] [--math bf16x3]
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


def loss_leg(a, model, sd, lin, dev):
    """(d) and (e) of the module docstring -> dict."""
    import statistics
    from sradsgan_amd import ops
    from tests import lpips_loss_ref as L
    B, crop, cl = a.batch, a.crop, torch.channels_last
    hr = R.hash_image((B, 3, crop, crop), 201).to(dev).contiguous(memory_format=cl)
    sr = (0.75 * hr + 0.25 * R.hash_image((B, 3, crop, crop), 202).to(dev)).contiguous(memory_format=cl).requires_grad_(True)
    sdd = {k: (v.to(dev).contiguous(memory_format=cl) if v.dim() == 4 else v.to(dev)) for k, v in sd.items()}
    lins = [lin['lin%d.model.1.weight' % k].flatten().to(dev) for k in range(5)]

    def hip():
        sr.grad = None
        model.loss(sr, hr).backward()

    def eager():
        sr.grad = None
        L.loss(sr, hr, sdd, lins, dtype=torch.float32).backward()

    hip_ms, eager_ms = [], []
    for _ in range(a.rounds):
        hip_ms.append(timed(hip, a.window, a.warmup)[0])
        eager_ms.append(timed(eager, a.window, a.warmup)[0])
    hip()
    g_hip = sr.grad.clone()
    eager()
    rel = float((g_hip - sr.grad).norm() / sr.grad.norm())
    out = {'metric': 'LPIPS.loss forward + backward, ms (B=%d, %dx%d, %s)' % (B, crop, crop, ops.get_conv_math()),
           'hip_ms': [round(v, 3) for v in hip_ms], 'eager_autograd_ms': [round(v, 3) for v in eager_ms],
           'speedup_median': round(statistics.median(eager_ms) / statistics.median(hip_ms), 2), 'grad_rel_2norm_vs_eager': float('%.2e' % rel)}
    if not a.no_step:
        import bench
        from sradsgan_amd.train_step import TrainStep
        steps = []
        for weight in (0.0, 1.0):
            G, D, F = bench.build_networks(dev, seed=20240)
            steps.append(TrainStep(G, D, F, lpips=model if weight else None, weight_lpips=weight))
        gen = torch.Generator().manual_seed(1234)
        hr_s = torch.rand(B, 3, bench.LR_SIDE * bench.SCALE, bench.LR_SIDE * bench.SCALE, generator=gen).to(dev)
        lr_s = torch.rand(B, 3, bench.LR_SIDE, bench.LR_SIDE, generator=gen).to(dev)
        alpha = torch.rand(B, 1, 1, 1, generator=gen).to(dev)
        ms = ([], [])
        for _ in range(a.rounds):
            for k in (0, 1):
                ms[k].append(timed(lambda: steps[k](lr_s, hr_s, alpha), a.window, a.warmup)[0])
        m0, m1 = statistics.median(ms[0]), statistics.median(ms[1])
        out.update({'step_ms_weight0': [round(v, 2) for v in ms[0]], 'step_ms_weight1': [round(v, 2) for v in ms[1]],
                    'step_cost_ms_median': round(m1 - m0, 2), 'step_cost_percent': round(100.0 * (m1 - m0) / m0, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=None, help='default 16, with --loss 32')
    ap.add_argument('--loss', action='store_true', help='the loss leg: LPIPS.loss forward + backward, and the training step with and without it')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--crop', type=int, default=216)
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--window', type=float, default=2.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--math', default='bf16x3')
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--no-evaluate', action='store_true')
    a = ap.parse_args()
    if a.batch is None:
        a.batch = 32 if a.loss else 16
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
    if a.loss:
        ops.set_conv_math(a.math)
        print(json.dumps(loss_leg(a, model, sd, lin, dev)))
        return
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
