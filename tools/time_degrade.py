"""Timing of the blur-and-noise degradation (sradsgan_amd/degrade.py, csrc/degrade.hip) on one GPU.  Reports figures; sets no
targets beyond the one comparison the blur has to win.

Batch 32 of 216 x 216 x 3 uint8 tiles:
  (a) srhip_blur_u8 alone (fixed kernels on the device, back-to-back launches between two device events) for l = 21 and l = 11,
      against the same blur as eager ATen in the same process: F.conv2d(groups = B * C) on a ReflectionPad2d input, the form the
      reference's BatchBlur runs.  The two legs alternate, --rounds rounds of --calls calls each; the median round of each leg and
      all rounds are reported.  The ATen leg starts from the float tensor (its to_tensor is not timed) and does not quantise: it does
      less than the kernel it is compared with;
  (b) the whole SRMDPreprocessing.__call__ (draws on the host, upload, blur, bicubic x4, noise): ms per call;
  (c) the benchmark training step (bench.py's networks and batch: full-depth SRADSGAN x4, LR 54 -> HR 216, batch 32) fed by
      data.training_batch against the same step fed by degrade.degraded_training_batch, alternated in one process in blocks of
      --block steps, each block between a host clock pair that ends in a device synchronise; the median step time of each leg.

Usage: python tools/time_degrade.py [--calls 50] [--rounds 5] [--blocks 6] [--block 5] [--skip-step] [--out FILE]
One JSON line on stdout; --out appends a readable summary."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SIZE, C, SCALE = 32, 216, 3, 4


def event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, out


def aten_blur(x, kernels, l):
    """BatchBlur.forward's per-sample branch with stock torch ops on the device."""
    b, c, h, w = x.shape
    lo, hi = l // 2, (l // 2 if l % 2 else l // 2 - 1)
    pad = torch.nn.functional.pad(x, (lo, hi, lo, hi), mode='reflect')
    weight = kernels.view(b, 1, l, l).repeat(1, c, 1, 1).view(b * c, 1, l, l)
    return torch.nn.functional.conv2d(pad.view(1, b * c, h + l - 1, w + l - 1), weight, groups=b * c).view(b, c, h, w)


def time_blur(dev, calls, rounds):
    from sradsgan_amd import data as D
    from sradsgan_amd import degrade as G
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (B, SIZE, SIZE, C), generator=g, dtype=torch.uint8).to(dev)
    x = D.to_tensor(src).contiguous()                                     # dense NCHW for the ATen leg
    out = {}
    for l in (21, 11):
        k = G.random_batch_kernel(B, l=l, rate_iso=0.5, generator=g).to(dev)
        legs = {'hip': lambda: G.blur_u8(src, k), 'aten': lambda: aten_blur(x, k, l)}
        times = {'hip': [], 'aten': []}
        for _ in range(rounds):
            for tag in ('hip', 'aten'):
                times[tag].append(event_ms(legs[tag], calls)[0])
        diff = (aten_blur(x, k, l) - D.to_tensor(G.blur_u8(src, k))).abs().max().item()
        taps = B * SIZE * SIZE * C * l * l
        med = {t: statistics.median(v) for t, v in times.items()}
        out['l%d' % l] = {'hip_blur_u8_ms_median': round(med['hip'], 4), 'aten_grouped_conv_ms_median': round(med['aten'], 4),
                          'hip_rounds_ms': [round(v, 4) for v in times['hip']], 'aten_rounds_ms': [round(v, 4) for v in times['aten']],
                          'aten_over_hip': round(med['aten'] / med['hip'], 2),
                          'hip_gtaps_per_s': round(taps / med['hip'] / 1e6, 1),
                          'max_abs_diff_aten_vs_quantised_hip': round(diff, 6)}
    return out


def time_preprocessing(dev, calls):
    from sradsgan_amd import degrade as G
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (B, SIZE, SIZE, C), generator=g, dtype=torch.uint8).to(dev)
    out = {}
    for tag, kw in (('l21_noise', dict(kernel=21, noise=True)), ('l21_plain', dict(kernel=21, noise=False)),
                    ('l11_noise', dict(kernel=11, noise=True))):
        pre = G.SRMDPreprocessing(SCALE, True, rate_iso=0.5, noise_high=0.08, seed=3, **kw)
        out[tag] = {'call_ms': round(event_ms(lambda: pre(src), calls)[0], 4)}
    return out


def time_training_step(dev, blocks, block):
    import bench
    from sradsgan_amd import data as D
    from sradsgan_amd import degrade as G
    from sradsgan_amd.train_step import TrainStep
    Gn, Dn, F = bench.build_networks(dev, seed=20240)
    step = TrainStep(Gn, Dn, F)
    g = torch.Generator().manual_seed(2)
    tiles = torch.randint(0, 256, (B, SIZE, SIZE, C), generator=g, dtype=torch.uint8).to(dev)
    alpha = torch.rand(B, 1, 1, 1, generator=g).to(dev)
    pre = G.SRMDPreprocessing(SCALE, True, kernel=21, noise=True, rate_iso=0.5, noise_high=0.08, seed=3)

    def plain():
        lr, hr, _ = D.training_batch(tiles, SCALE)
        return step(lr, hr, alpha)

    def degraded():
        lr, hr, _ = G.degraded_training_batch(tiles, SCALE, pre)
        return step(lr, hr, alpha)

    for _ in range(25):                                           # bench.py's spin-up: clocks, weight packs, allocator
        plain()
    for _ in range(3):
        degraded()
    torch.cuda.synchronize()
    times = {'plain': [], 'degraded': []}
    for _ in range(blocks):
        for tag, fn in (('plain', plain), ('degraded', degraded)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                out = fn()
            torch.cuda.synchronize()
            times[tag].append((time.perf_counter() - t0) * 1e3 / block)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ('loss_G', 'loss_D'))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {'plain_step_ms_median': round(med['plain'], 3), 'degraded_step_ms_median': round(med['degraded'], 3),
            'plain_step_ms_blocks': [round(v, 3) for v in times['plain']],
            'degraded_step_ms_blocks': [round(v, 3) for v in times['degraded']],
            'degraded_over_plain': round(med['degraded'] / med['plain'], 5), 'steps_per_block': block}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--block', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_degrade: needs the GPU; a CPU run measures nothing')
    dev = torch.device('cuda:0')
    res = {'metric': 'degradation: batch %d, %dx%dx%d uint8, x%d' % (B, SIZE, SIZE, C, SCALE),
           'blur': time_blur(dev, a.calls, a.rounds), 'preprocessing': time_preprocessing(dev, a.calls)}
    if not a.skip_step:
        res['training_step'] = time_training_step(dev, a.blocks, a.block)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('# python tools/time_degrade.py --calls %d --rounds %d --blocks %d --block %d\n' % (a.calls, a.rounds, a.blocks, a.block))
            for section, rows in res.items():
                if isinstance(rows, dict):
                    f.write('%s\n' % section)
                    for k, v in rows.items():
                        f.write('  %-28s %s\n' % (k, json.dumps(v)))
            f.write('\n')


if __name__ == '__main__':
    main()
