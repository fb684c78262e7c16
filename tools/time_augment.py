"""Timing of the dihedral kernels' two users on one GPU.  Reports figures; sets no targets.

Augmentation (data.Augment, csrc/augment.hip), batch 32 of 256 x 256 x 3 uint8 sources -> 216 x 216 crops, all switches on:
  (a) Augment.__call__ (draw on the host, table upload, kernel) with and without Gaussian noise: ms per call over --calls calls
      between two device events, and the kernel alone (fixed table, back-to-back launches) with its achieved bytes/s, counting one
      read and one write of the 32 x 216 x 216 x 3 crop bytes (the gather touches no more of the source than that);
  (b) the benchmark training step (bench.py's networks and batch: full-depth SRADSGAN x4, LR 54 -> HR 216, batch 32) fed by
      data.training_batch on pre-cut 216 tiles against the same step fed by data.augmented_training_batch on the 256 sources,
      alternated in one process in blocks of --block steps, each block between a host clock pair that ends in a device
      synchronise; the median step time of each leg.  The yardstick of the augmented leg is the plain leg of the same process.

Self-ensemble (ensemble.self_ensemble), batch 16, LR 54 x 54 -> 216 x 216 with the same generator:
  (c) one plain inference, self_ensemble (default stacking and chunk=1), and the loop a user would write -- eight generator calls
      on torch.flip / transpose views, mapped back and averaged by torch: ms per call and peak allocated memory of each above what
      was allocated when the leg began; the padded-plane pool (ops.plane_pool, which keeps its buffers per geometry and hands out a
      new one rather than wait for a busy one) is emptied before every leg, so no leg inherits another's buffers.

Usage: python tools/time_augment.py [--calls 200] [--blocks 6] [--block 5] [--reps 3] [--skip-step] [--skip-ensemble] [--out FILE]
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

B, SRC, CROP, SCALE = 32, 256, 216, 4


def event_ms(fn, reps, warmup=3):
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


def time_augment_calls(dev, calls):
    from sradsgan_amd import data as D
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (B, SRC, SRC, 3), generator=g, dtype=torch.uint8).to(dev)
    out, crop_bytes = {}, B * CROP * CROP * 3
    for tag, noise in (('plain', None), ('noise', ['Gaussain', 5.0])):
        aug = D.Augment(CROP, SCALE, random_crop=True, rotate=True, fliplr=True, fliptb=True, noise=noise, seed=3)
        call_ms, _ = event_ms(lambda: aug(src), calls)
        table = aug.draw(B, SRC, SRC).to(dev)
        kernel_ms, _ = event_ms(lambda: D.augment_u8(src, table, CROP, aug.sigma, None, 3, 0), calls)
        out[tag] = {'call_ms': round(call_ms, 4), 'kernel_back_to_back_ms': round(kernel_ms, 4),
                    'kernel_gbytes_per_s': round(2 * crop_bytes / kernel_ms / 1e6, 1)}
    return out


def time_training_step(dev, blocks, block):
    import bench
    from sradsgan_amd import data as D
    from sradsgan_amd.train_step import TrainStep
    G, Dn, F = bench.build_networks(dev, seed=20240)
    step = TrainStep(G, Dn, F)
    g = torch.Generator().manual_seed(2)
    src = torch.randint(0, 256, (B, SRC, SRC, 3), generator=g, dtype=torch.uint8).to(dev)
    tiles = src[:, :CROP, :CROP].contiguous()
    alpha = torch.rand(B, 1, 1, 1, generator=g).to(dev)
    aug = D.Augment(CROP, SCALE, random_crop=True, rotate=True, fliplr=True, fliptb=True, noise=['Gaussain', 5.0], seed=3)

    def plain():
        lr, hr, _ = D.training_batch(tiles, SCALE)
        return step(lr, hr, alpha)

    def augmented():
        lr, hr, _ = D.augmented_training_batch(src, SCALE, aug)
        return step(lr, hr, alpha)

    for _ in range(25):                                           # bench.py's spin-up: clocks, weight packs, allocator
        plain()
    for _ in range(3):
        augmented()
    torch.cuda.synchronize()
    times = {'plain': [], 'augmented': []}
    for _ in range(blocks):
        for tag, fn in (('plain', plain), ('augmented', augmented)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                out = fn()
            torch.cuda.synchronize()
            times[tag].append((time.perf_counter() - t0) * 1e3 / block)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ('loss_G', 'loss_D'))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {'plain_step_ms_median': round(med['plain'], 3), 'augmented_step_ms_median': round(med['augmented'], 3),
            'plain_step_ms_blocks': [round(v, 3) for v in times['plain']],
            'augmented_step_ms_blocks': [round(v, 3) for v in times['augmented']],
            'augmented_over_plain': round(med['augmented'] / med['plain'], 5), 'steps_per_block': block}


def torch_ensemble(gen, lr):
    acc = None
    for op in range(8):
        v = lr
        if op & 1:
            v = v.transpose(2, 3)
        if op & 2:
            v = v.flip(2)
        if op & 4:
            v = v.flip(3)
        y = gen(v.contiguous())
        if op & 4:
            y = y.flip(3)
        if op & 2:
            y = y.flip(2)
        if op & 1:
            y = y.transpose(2, 3)
        acc = y if acc is None else acc + y
    return acc * 0.125


def time_ensemble(dev, reps):
    import bench
    from sradsgan_amd import ensemble as E
    from sradsgan_amd import ops
    gen = bench.build_networks(dev, seed=20240)[0].eval()
    lr = torch.rand(16, 3, 54, 54, generator=torch.Generator().manual_seed(5)).to(dev)
    out = {}
    with torch.no_grad():
        for tag, fn in (('one_inference', lambda: gen(lr)), ('self_ensemble', lambda: E.self_ensemble(gen, lr)),
                        ('self_ensemble_chunk1', lambda: E.self_ensemble(gen, lr, chunk=1)), ('torch_loop', lambda: torch_ensemble(gen, lr))):
            torch.cuda.synchronize()
            ops.plane_pool.release_all()         # every leg starts without the padded-plane buffers the legs before it left (they stay per geometry)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ms, res = event_ms(fn, reps, warmup=2)
            out[tag] = {'ms': round(ms, 2), 'peak_mem_mib_above_resident': round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)}
            if tag == 'self_ensemble_chunk1':
                one = res
            if tag == 'torch_loop':
                out[tag]['max_abs_diff_vs_chunk1'] = float((res - one).abs().max())
    for tag in ('self_ensemble', 'self_ensemble_chunk1', 'torch_loop'):
        out[tag]['over_one_inference'] = round(out[tag]['ms'] / out['one_inference']['ms'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--block', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--skip-ensemble', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_augment: needs the GPU; a CPU run measures nothing')
    dev = torch.device('cuda:0')
    res = {'metric': 'augmentation: batch %d, %dx%d -> %d, all switches on; self-ensemble: batch 16, 54 -> 216, x%d' % (B, SRC, SRC, CROP, SCALE),
           'augment': time_augment_calls(dev, a.calls)}
    if not a.skip_step:
        res['training_step'] = time_training_step(dev, a.blocks, a.block)
        res['training_step']['augment_call_share_of_plain_step'] = round(
            res['augment']['noise']['call_ms'] / res['training_step']['plain_step_ms_median'], 5)
    if not a.skip_ensemble:
        res['self_ensemble'] = time_ensemble(dev, a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('# python tools/time_augment.py --calls %d --blocks %d --block %d --reps %d\n' % (a.calls, a.blocks, a.block, a.reps))
            for section, rows in res.items():
                if isinstance(rows, dict):
                    f.write('%s\n' % section)
                    for k, v in rows.items():
                        f.write('  %-28s %s\n' % (k, json.dumps(v)))
            f.write('\n')


if __name__ == '__main__':
    main()
