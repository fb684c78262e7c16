"""Dilated 3x3 convolutions on one GPU: ASPP's 256 -> 256 convs (x4, B = 16, 54 x 54 LR) through the HIP path
(sradsgan_amd.ops.conv2d_dil_*_raw: forward into a [n, h, w, 768] buffer, data gradient, weight gradient + bias) next to eager
ATen (F.conv2d with dilation, and its autograd backward) on the same tensors.  One JSON line: milliseconds per call and TFLOP/s
(2 n h w cin cout 9 per pass).
Usage: python tools/time_dilated_conv.py [--batch 16] [--size 54] [--steps 20] [--warmup 5] [--mode bf16x3]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402


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
    ap.add_argument('--size', type=int, default=54)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--mode', default='bf16x3', choices=['bf16x3', 'fp32', 'half'])
    a = ap.parse_args()
    from sradsgan_amd import ops
    dev = torch.device('cuda:0')
    n, c, h, w = a.batch, a.channels, a.size, a.size
    cl = torch.channels_last
    x = O.det_fill('tdil.x', (n, c, h, w), 1.0).to(dev).contiguous(memory_format=cl)
    dy = O.det_fill('tdil.dy', (n, c, h, w), 1e-3).to(dev).contiguous(memory_format=cl)
    buf = torch.empty(n, 3 * c, h, w, device=dev).contiguous(memory_format=cl)
    dx = torch.empty(n, c, h, w, device=dev).contiguous(memory_format=cl)
    flop = 2.0 * n * h * w * c * c * 9
    out = {'metric': 'dilated 3x3 conv %d->%d, B=%d, %dx%d' % (c, c, n, h, w), 'mode': a.mode, 'unit': 'ms per call', 'dilation': {}}
    with ops.conv_math(a.mode):
        for d in (1, 2, 3):
            wt = torch.nn.Parameter(O.det_fill('tdil.w%d' % d, (c, c, 3, 3), 0.03).to(dev))
            b = O.det_fill('tdil.b%d' % d, (c,), 0.1).to(dev)
            slot = buf[:, (d - 1) * c:]
            fwd = timed(lambda: ops.conv2d_dil_fwd_raw(x, c, wt, b, slot, 3 * c, n, h, w, d), a.steps, a.warmup)
            dgrad = timed(lambda: ops.conv2d_dil_dgrad_raw(dy, c, wt, dx, c, n, h, w, d), a.steps, a.warmup)
            wgrad = timed(lambda: ops.conv2d_dil_wgrad_raw(x, c, dy, c, tuple(wt.shape), n, h, w, d), a.steps, a.warmup)
            xe = x.clone().requires_grad_()
            we = wt.detach().clone().requires_grad_()
            be = b.clone().requires_grad_()
            e_fwd = timed(lambda: F.conv2d(xe, we, be, 1, d, d), a.steps, a.warmup)
            e_step = timed(lambda: torch.autograd.grad(F.conv2d(xe, we, be, 1, d, d), (xe, we, be), dy), a.steps, a.warmup)
            out['dilation'][str(d)] = {
                'hip_fwd_ms': round(fwd, 4), 'hip_dgrad_ms': round(dgrad, 4), 'hip_wgrad_ms': round(wgrad, 4),
                'hip_fwd_tflops': round(flop / fwd / 1e9, 1), 'hip_dgrad_tflops': round(flop / dgrad / 1e9, 1),
                'hip_wgrad_tflops': round(flop / wgrad / 1e9, 1),
                'hip_fwd_bwd_ms': round(fwd + dgrad + wgrad, 4),
                'eager_fwd_ms': round(e_fwd, 4), 'eager_fwd_bwd_ms': round(e_step, 4)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
