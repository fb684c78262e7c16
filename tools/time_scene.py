"""Whole-scene super-resolution timing on one GPU (sradsgan_amd/scene.py): a random uint8 LR scene (default 1024 x 1024 at x4, the
full-depth SRADSGAN generator, tile crop_size // scale = 54, overlap tile // 4) through
  (a) super_resolve_scene: HIP tile extraction, the generator, the HIP feathered blend, banded;
  (b) the eager equivalent on the same GPU with the same generator: a Python loop of slicing, to_tensor in torch, the generator, a
      torch weighted paste into scene-sized fp32 accumulators and torch quantisation;
  (c) the tiling alone: (a) with the generator replaced by a constant SR batch, i.e. the two new kernels with their host calls and
      table uploads -- its share of (a)'s wall time is reported.
Each path is warmed up once on the whole scene and then timed with device events over --reps runs.  HR megapixels per second; one JSON
line.  Usage: python tools/time_scene.py [--height 1024] [--width 1024] [--scale 4] [--tile 54] [--overlap 13] [--tiles-per-batch 16]
[--groups 12] [--blocks 3] [--reps 2] [--no-eager]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()                                                               # warm-up: every batch shape, the weight packs, the allocator
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, out


def eager_scene(gen, scene, plan, tiles_per_batch):
    """The loop a user would write around the generator: same plan, same weights, same blend formula, ATen ops only."""
    dev = scene.device
    wy, wx = torch.from_numpy(plan.ys.weights).to(dev), torch.from_numpy(plan.xs.weights).to(dev)
    acc = torch.zeros(plan.hr_h, plan.hr_w, 3, device=dev)
    wsum = torch.zeros(plan.hr_h, plan.hr_w, 1, device=dev)
    Th, Tw = plan.ys.hr_tile, plan.xs.hr_tile
    with torch.no_grad():
        for j in range(plan.ys.n):
            origins = plan.origins(j)
            for c in range(0, len(origins), tiles_per_batch):
                part = origins[c:c + tiles_per_batch]
                x = torch.stack([scene[y:y + plan.th, xx:xx + plan.tw] for y, xx in part]).permute(0, 3, 1, 2).float().div(255.0)
                sr = gen(x.contiguous(memory_format=torch.channels_last))
                for k in range(len(part)):
                    ya, xa = plan.ys.hr_positions[j], plan.xs.hr_positions[c + k]
                    w2 = (wy[j][:, None] * wx[c + k][None, :])[:, :, None]
                    acc[ya:ya + Th, xa:xa + Tw] += w2 * sr[k].permute(1, 2, 0)
                    wsum[ya:ya + Th, xa:xa + Tw] += w2
    return (acc / wsum * 255.0).clamp(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--tile', type=int, default=None)
    ap.add_argument('--overlap', type=int, default=None)
    ap.add_argument('--tiles-per-batch', type=int, default=16)
    ap.add_argument('--groups', type=int, default=12)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--no-eager', action='store_true')
    a = ap.parse_args()
    from sradsgan_amd import model as M, scene as S, trainer as T
    dev = torch.device('cuda:0')
    tile = 216 // a.scale if a.tile is None else a.tile
    overlap = tile // 4 if a.overlap is None else a.overlap
    torch.manual_seed(0)
    gen = M.GeneratorResNet(M.ResGroup, n_residual_blocks=a.groups, n_basic_blocks=a.blocks, upscale_factor=a.scale)
    gen.apply(T.weights_init_normal)
    gen = gen.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    scene = torch.randint(0, 256, (a.height, a.width, 3), generator=g, dtype=torch.uint8).to(dev)
    plan = S.ScenePlan(a.height, a.width, a.scale, tile, overlap)
    mpx = plan.hr_h * plan.hr_w / 1e6
    hip_ms, hip_out = timed(lambda: S.super_resolve_scene(gen, scene, a.scale, tile, overlap, a.tiles_per_batch), a.reps)
    peak = torch.cuda.max_memory_allocated()
    const = torch.rand(a.tiles_per_batch, 3, plan.ys.hr_tile, plan.xs.hr_tile, device=dev).contiguous(memory_format=torch.channels_last)
    tiling_ms, _ = timed(lambda: S.run_plan(plan, scene, lambda x: const[:x.shape[0]], a.tiles_per_batch).out, a.reps)
    out = {'metric': 'whole-scene SR, %dx%d LR x%d, SRADSGAN %dx%d, tile %d overlap %d, %d x %d tiles in batches of %d, ring %d'
                     % (a.height, a.width, a.scale, a.groups, a.blocks, tile, overlap, plan.ys.n, plan.xs.n, a.tiles_per_batch,
                        plan.ring_depth),
           'hr_megapixels': round(mpx, 3), 'hip_ms': round(hip_ms, 2), 'hip_mpx_per_s': round(mpx / hip_ms * 1e3, 2),
           'tiling_only_ms': round(tiling_ms, 2), 'tiling_share_of_hip': round(tiling_ms / hip_ms, 4),
           'hip_peak_mem_gib': round(peak / 2 ** 30, 2)}
    if not a.no_eager:
        eager_ms, eager_out = timed(lambda: eager_scene(gen, scene, plan, a.tiles_per_batch), a.reps)
        diff = (hip_out.int() - eager_out.int()).abs()
        out.update({'eager_ms': round(eager_ms, 2), 'eager_mpx_per_s': round(mpx / eager_ms * 1e3, 2),
                    'speedup': round(eager_ms / hip_ms, 2), 'max_level_diff_vs_eager': int(diff.max()),
                    'share_differing': float('%.2e' % float((diff > 0).float().mean()))})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
