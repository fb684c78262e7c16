"""Timing of the contrastive VGG19 losses on one GPU at the training shape (B = 32, 216 x 216, one negative), for both kinds:
(a) forward + backward of contrast.ContrastLoss / ContrastCosineLoss against eager ATen autograd of the same composition
(tests/contrast_ref.py in fp32, channels-last, the positive and the negative under no_grad as the reference's detach leaves them) and
(b) the benchmark's training step (bench.build_networks, B x 54x54 -> 216x216) with weight_contrast 0 against 1 -- each pair in one
process, the legs alternated over --rounds rounds, every window listed so that drift between the rounds shows.  Every shape is warmed up
first; each figure is timed with device events over a window of at least --window seconds.  One JSON line per kind.
Usage: python tools/time_contrast.py [--batch 32] [--crop 216] [--rounds 2] [--window 2] [--no-step] [--no-eager] [--math bf16x3]
(`rocprofv3 --kernel-trace --stats -- python tools/time_contrast.py --no-eager --no-step` for the per-kernel table)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import contrast_ref as R  # noqa: E402
from tools.time_lpips import timed  # noqa: E402


def leg(a, kind, vgg, sdd, dev):
    from sradsgan_amd import contrast as C
    from sradsgan_amd import ops
    B, crop, cl = a.batch, a.crop, torch.channels_last
    hr = R.hash_image((B, 3, crop, crop), 201).to(dev).contiguous(memory_format=cl)
    bc = (0.5 * hr + 0.5 * R.hash_image((B, 3, crop, crop), 203).to(dev)).contiguous(memory_format=cl)
    sr = (0.75 * hr + 0.25 * R.hash_image((B, 3, crop, crop), 202).to(dev)).contiguous(memory_format=cl).requires_grad_(True)
    model = getattr(C, kind)(vgg=vgg)

    def hip():
        sr.grad = None
        model(sr, hr, bc).backward()

    def eager():
        sr.grad = None
        with torch.no_grad():
            fp, fn = R.taps(hr, sdd), [R.taps(bc, sdd)]
        fa = R.taps(sr, sdd)
        (R.cos_from_taps(fa, fp, fn, False) if 'Cosine' in kind else R.l1_from_taps(fa, fp, fn)).backward()

    hip_ms, eager_ms = [], []
    for _ in range(a.rounds):
        hip_ms.append(timed(hip, a.window, a.warmup)[0])
        if not a.no_eager:
            eager_ms.append(timed(eager, a.window, a.warmup)[0])
    out = {'metric': '%s forward + backward, ms (B=%d, %dx%d, N=1, %s)' % (kind, B, crop, crop, ops.get_conv_math()),
           'hip_ms': [round(v, 3) for v in hip_ms]}
    if not a.no_eager:
        hip()
        g_hip = sr.grad.clone()
        eager()
        rel = float((g_hip - sr.grad).norm() / sr.grad.norm())
        out.update({'eager_autograd_ms': [round(v, 3) for v in eager_ms],
                    'speedup_median': round(statistics.median(eager_ms) / statistics.median(hip_ms), 2),
                    'grad_rel_2norm_vs_eager': float('%.2e' % rel)})
    if not a.no_step:
        import bench
        from sradsgan_amd.train_step import TrainStep
        steps = []
        for weight in (0.0, 1.0):
            G, D, F = bench.build_networks(dev, seed=20240)
            steps.append(TrainStep(G, D, F, contrast=model if weight else None, weight_contrast=weight))
        gen = torch.Generator().manual_seed(1234)
        hr_s = torch.rand(B, 3, bench.LR_SIDE * bench.SCALE, bench.LR_SIDE * bench.SCALE, generator=gen).to(dev)
        lr_s = torch.rand(B, 3, bench.LR_SIDE, bench.LR_SIDE, generator=gen).to(dev)
        bc_s = torch.nn.functional.interpolate(lr_s, scale_factor=bench.SCALE, mode='bicubic', align_corners=False)
        alpha = torch.rand(B, 1, 1, 1, generator=gen).to(dev)
        calls = (lambda: steps[0](lr_s, hr_s, alpha), lambda: steps[1](lr_s, hr_s, alpha, negatives=bc_s))
        ms = ([], [])
        for _ in range(a.rounds):
            for k in (0, 1):
                ms[k].append(timed(calls[k], a.window, a.warmup)[0])
        m0, m1 = statistics.median(ms[0]), statistics.median(ms[1])
        out.update({'step_ms_weight0': [round(v, 2) for v in ms[0]], 'step_ms_weight1': [round(v, 2) for v in ms[1]],
                    'step_cost_ms_median': round(m1 - m0, 2), 'step_cost_percent': round(100.0 * (m1 - m0) / m0, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--crop', type=int, default=216)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--window', type=float, default=2.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--math', default='bf16x3')
    ap.add_argument('--kinds', default='ContrastLoss,ContrastCosineLoss')
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('time_contrast: needs a HIP device; a CPU run measures nothing')
    from sradsgan_amd import ops
    from sradsgan_amd.contrast import Vgg19Taps
    dev = torch.device('cuda:0')
    sd = R.vgg19_state_dict()
    vgg = Vgg19Taps()
    vgg.load_torchvision_vgg19(sd)
    vgg = vgg.to(dev)
    sdd = {k: (v.to(dev).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev)) for k, v in sd.items()}
    ops.set_conv_math(a.math)
    for kind in a.kinds.split(','):
        print(json.dumps(leg(a, kind, vgg, sdd, dev)), flush=True)


if __name__ == '__main__':
    main()
