"""HAT throughput on one GPU at the reference's training configuration (GeneratorResNet defaults: 6 RHAGs x 6 HABs, embed 96, window
9, img_size = crop / scale; main_hat.py: crop 216, B = 16, Adam lr 2e-4, betas (0.9, 0.99)): (a) the L1 training step
(sradsgan_amd.model.hat.train_step, train mode: drop path on), (b) generator inference, (c) the same two in eager ATen fp32 on the same
GPU (the restatement tests/hat_ref.py with the same parameters, torch.optim.Adam; train mode's drop path is not drawn there), and
(d) the peak device memory of the HIP step.  Every shape is warmed up first; each figure is timed with device events over a window
of at least --window seconds.  One JSON line.
--published hat | hat-s times the published networks instead (HAT: embed 180, HAT-S: embed 144 with compress_ratio 24 and
squeeze_factor 24; six heads, window 16, mlp_ratio 2, 6 x 6) at x4, 64 -> 256, the same four figures against the same eager
restatement.  --kernel-share N adds the N kernels with the most device time in one training step and one inference call (torch's
profiler) and the share of the window-attention kernels among them.
Usage: python tools/time_hat.py [--scale 8] [--batch 16] [--window 5] [--no-eager] [--math bf16x3] [--published hat] [--kernel-share 12]
(`rocprofv3 --kernel-trace --stats -- python tools/time_hat.py --no-eager` for the per-kernel table)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import hat_ref as R  # noqa: E402


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


PUBLISHED = {'hat': ('HAT', dict(embed_dim=180, compress_ratio=3, squeeze_factor=30)),
             'hat-s': ('HAT-S', dict(embed_dim=144, compress_ratio=24, squeeze_factor=24))}


def kernel_share(fn, top):
    """device time by kernel name over one call of fn: (total ms, share of the window-attention kernels, the `top` largest)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        t = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0)
        if t:
            rows[e.name] = rows.get(e.name, 0.0) + t
    total = sum(rows.values()) or 1.0
    attn = sum(v for k, v in rows.items() if 'attn' in k and ('hat' in k))
    names = sorted(rows.items(), key=lambda kv: -kv[1])[:top]
    return round(total / 1000.0, 2), round(attn / total, 3), [[k[:90], round(v / total, 3)] for k, v in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scale', type=int, default=8)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--crop', type=int, default=216)
    ap.add_argument('--window', type=float, default=5.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--math', default='bf16x3')
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--published', choices=sorted(PUBLISHED), default=None)
    ap.add_argument('--kernel-share', type=int, default=0)
    a = ap.parse_args()
    if a.published:
        a.scale, a.crop = 4, 256
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    dev = torch.device('cuda:0')
    B, s, lr_size = a.batch, a.scale, a.crop // a.scale
    ws = 9 if s in (2, 4, 8) else 8                        # hat.py:625-626
    label, kw, dim = 'HAT', {}, 96
    if a.published:
        label, kw = PUBLISHED[a.published]
        label, ws, dim = label + ' (published)', 16, kw['embed_dim']
        kw = dict(kw, mlp_ratio=2.)
    G = R.init_(H.GeneratorResNet(upscale=s, window_size=ws, img_size=lr_size, **kw))
    sd_init = {k: v.clone() for k, v in G.state_dict().items()}
    G = G.to(dev).train()
    x = O.det_fill('time.x', (B, 3, lr_size, lr_size), 0.5, 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    t = O.det_fill('time.t', (B, 3, a.crop, a.crop), 0.5, 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    opt = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.99))
    ops.set_conv_math(a.math)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    train_ms, n_train = timed(lambda: H.train_step(G, opt, x, t), a.window, a.warmup)
    peak_train = torch.cuda.max_memory_allocated(dev)

    def infer():
        with torch.no_grad():
            G(x)
    G.eval()
    torch.cuda.reset_peak_memory_stats(dev)
    infer_ms, n_infer = timed(infer, a.window, a.warmup)
    peak_infer = torch.cuda.max_memory_allocated(dev)
    metric = '%s x%d img/s (6x6, window %d, B=%d, %d->%d, %s)' % (label, s, ws, B, lr_size, a.crop, a.math)
    if a.published:
        metric = '%s x%d img/s (6x6, embed %d, window %d, B=%d, %d->%d, %s)' % (label, s, dim, ws, B, lr_size, a.crop, a.math)
    out = {'metric': metric,
           'train_img_s': round(B * 1000.0 / train_ms, 1), 'train_ms': round(train_ms, 2), 'train_calls': n_train,
           'infer_img_s': round(B * 1000.0 / infer_ms, 1), 'infer_ms': round(infer_ms, 2), 'infer_calls': n_infer,
           'peak_mem_train_GiB': round(peak_train / 2.0 ** 30, 2), 'peak_mem_infer_GiB': round(peak_infer / 2.0 ** 30, 2)}
    if a.kernel_share:
        G.train()
        out['train_kernel_ms'], out['train_attn_share'], out['train_top_kernels'] = kernel_share(lambda: H.train_step(G, opt, x, t),
                                                                                                 a.kernel_share)
        G.eval()
        out['infer_kernel_ms'], out['infer_attn_share'], out['infer_top_kernels'] = kernel_share(infer, a.kernel_share)
    if not a.no_eager:
        del G, opt
        torch.cuda.empty_cache()
        sd = {k: (v.to(dev).requires_grad_(True) if v.dtype.is_floating_point else v.to(dev)) for k, v in sd_init.items()}
        cfg = R.config(s, ws, (6,) * 6, lr_size)
        cfg['dim'] = dim
        params = [v for v in sd.values() if v.requires_grad]
        eopt = torch.optim.Adam(params, lr=2e-4, betas=(0.9, 0.99))

        def estep():
            eopt.zero_grad(set_to_none=True)
            loss = F.l1_loss(R.forward(sd, x, cfg), t)
            loss.backward()
            eopt.step()
        torch.cuda.reset_peak_memory_stats(dev)
        e_train, _ = timed(estep, a.window, a.warmup)
        e_peak = torch.cuda.max_memory_allocated(dev)

        def einfer():
            with torch.no_grad():
                R.forward(sd, x, cfg)
        e_infer, _ = timed(einfer, a.window, a.warmup)
        out.update({'eager_train_img_s': round(B * 1000.0 / e_train, 1), 'eager_infer_img_s': round(B * 1000.0 / e_infer, 1),
                    'eager_peak_mem_train_GiB': round(e_peak / 2.0 ** 30, 2),
                    'train_speedup': round(e_train / train_ms, 2), 'infer_speedup': round(e_infer / infer_ms, 2)})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
