"""Timing of the papers' evaluation protocol on one GPU (sradsgan_amd/metrics.py, csrc/metrics_pub.hip).  A tool, not a test.

Case 1: B = 16 float images 216 x 216 x 3.  validate.quantized_metrics (the reference trainer's protocol, existing kernels) against
  metrics.published_metrics (crop 4, luma), and both against the published protocol written with torch ops on the same GPU (fp64
  F.conv2d with the 11 x 11 window over the five moment planes).  The legs alternate in one process.
Case 2: one 4096 x 4096 x 3 uint8 scene pair.  metrics.published_metrics_u8 against the torch composition, and the share of
  scene.evaluate_scene (full-depth SRADSGAN x4, tile 54, overlap 13) that its two metric calls take.
Every time comes from device events around back-to-back calls after a warm-up; `kernel_us` times the three launches of the library
alone (buffers allocated once), `call_us` the Python entry.  GB/s counts one read of both images' bytes (the cropped region is what the
kernels read; the whole image is counted).  One JSON line per case.
Usage: python tools/time_metrics.py [--reps 50] [--scene 4096] [--no-scene-sr] [--no-torch]"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_us(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def torch_published(a_u8, b_u8, crop, y):
    """The published protocol of uint8 NHWC batches with ATen ops: (psnr, ssim) float64 [N]."""
    n, h, w, c = a_u8.shape
    a = a_u8[:, crop:h - crop, crop:w - crop].permute(0, 3, 1, 2).double()
    b = b_u8[:, crop:h - crop, crop:w - crop].permute(0, 3, 1, 2).double()
    if y:
        coef = torch.tensor([65481.0, 128553.0, 24966.0], device=a.device, dtype=torch.float64).view(1, 3, 1, 1)
        a, b = 16.0 + (a * coef).sum(1, keepdim=True) / 255000.0, 16.0 + (b * coef).sum(1, keepdim=True) / 255000.0
    mse = ((a - b) ** 2).mean(dim=(1, 2, 3))
    g = torch.exp(-((torch.arange(11, device=a.device, dtype=torch.float64) - 5.0) ** 2) / 4.5)
    g = g / g.sum()
    ch = a.shape[1]
    win = (g[:, None] * g[None, :]).expand(ch, 1, 11, 11).contiguous()
    f = lambda p: F.conv2d(p, win, groups=ch)
    mu1, mu2 = f(a), f(b)
    s1, s2, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return 10.0 * torch.log10(255.0 ** 2 / mse), ssim.mean(dim=(1, 2, 3))


def kernel_legs(a, b, n, h, w, c, crop, luma, is_float):
    """The library's three launches on preallocated buffers: a function per launch and one for all three."""
    from sradsgan_amd import _hip, metrics
    lib = _hip.lib()
    nb = metrics.library_config()[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    part = torch.empty(n, nb, 2, device=a.device, dtype=torch.int64)
    spart = torch.empty(n, nb, device=a.device, dtype=torch.float64)
    out = torch.empty(3, n, device=a.device, dtype=torch.float64)
    sse = lambda: _hip.check(lib.srhip_pub_sse(p(a), p(b), p(part), n, h, w, c, crop, luma, is_float, st))
    ssim = lambda: _hip.check(lib.srhip_pub_ssim(p(a), p(b), p(spart), n, h, w, c, crop, luma, is_float, st))
    fin = lambda: _hip.check(lib.srhip_pub_finish(p(part), p(spart), p(out), n, h, w, c, crop, luma, st))
    return sse, ssim, fin, (lambda: (sse(), ssim(), fin()))


def guarded(fn):
    try:
        return fn()
    except Exception as e:                                              # e.g. no fp64 convolution in the installed torch
        return 'failed: %s' % (str(e).splitlines()[0][:120],)


def case1(reps, with_torch):
    from sradsgan_amd import metrics as M, validate as V
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    hr = torch.rand(16, 3, 216, 216, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    sr = (hr + 0.05 * torch.randn(16, 3, 216, 216, generator=g).to(dev)).contiguous(memory_format=torch.channels_last)
    nbytes = 2 * hr.numel() * 4
    sse, ssim, fin, all3 = kernel_legs(sr, hr, 16, 216, 216, 3, 4, 1, 1)
    legs = {'quantized_metrics_call_us': lambda: V.quantized_metrics(sr, hr, 4),
            'published_metrics_call_us': lambda: M.published_metrics(sr, hr, 4, True),
            'published_kernels_us': all3, 'published_sse_kernel_us': sse, 'published_ssim_kernel_us': ssim,
            'published_finish_kernel_us': fin}
    if with_torch:
        qs, qh = M.quantise(sr), M.quantise(hr)
        legs['torch_composition_us'] = lambda: torch_published(qs, qh, 4, True)
    res = {k: [] for k in legs}
    for _ in range(3):                                                  # alternate the legs
        for k, fn in legs.items():
            res[k].append(guarded(lambda: round(timed_us(fn, reps), 2)))
    out = {'case': 'B=16 216x216x3 float, crop 4, luma', 'image_bytes_read': nbytes}
    for k, v in res.items():
        out[k] = v
    best = min(x for x in res['published_kernels_us'] if not isinstance(x, str))
    out['published_kernels_gbytes_per_s'] = round(nbytes / best / 1e3, 1)
    if with_torch and not isinstance(guarded(lambda: torch_published(qs, qh, 4, True)), str):
        ps, ss = torch_published(qs, qh, 4, True)
        m = M.published_metrics(sr, hr, 4, True)
        out['max_abs_ssim_diff_vs_torch'] = float((m['ssim'] - ss).abs().max())
        out['max_rel_psnr_diff_vs_torch'] = float(((m['psnr'] - ps) / ps).abs().max())
    return out


def case2(reps, side, with_torch, with_sr):
    from sradsgan_amd import metrics as M
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1)
    b = torch.randint(0, 256, (1, side, side, 3), generator=g, dtype=torch.uint8).to(dev)
    a = (b.int() + torch.randint(-6, 7, (1, side, side, 3), generator=g).to(dev)).clamp(0, 255).to(torch.uint8)
    nbytes = 2 * a.numel()
    sse, ssim, fin, all3 = kernel_legs(a, b, 1, side, side, 3, 4, 1, 0)
    legs = {'published_metrics_u8_call_us': lambda: M.published_metrics_u8(a, b, 4, True), 'published_kernels_us': all3,
            'published_sse_kernel_us': sse, 'published_ssim_kernel_us': ssim}
    if with_torch:
        legs['torch_composition_us'] = lambda: torch_published(a, b, 4, True)
    res = {k: [] for k in legs}
    for _ in range(2):
        for k, fn in legs.items():
            res[k].append(guarded(lambda: round(timed_us(fn, max(2, reps // 10)), 1)))
    out = {'case': '%dx%dx3 uint8 scene pair, crop 4, luma' % (side, side), 'image_bytes_read': nbytes}
    out.update(res)
    best = min(x for x in res['published_kernels_us'] if not isinstance(x, str))
    out['published_kernels_gbytes_per_s'] = round(nbytes / best / 1e3, 1)
    if with_sr:
        from sradsgan_amd import model as Mo, scene as S, trainer as T
        torch.manual_seed(0)
        gen = Mo.GeneratorResNet(Mo.ResGroup, n_residual_blocks=12, n_basic_blocks=3, upscale_factor=4)
        gen.apply(T.weights_init_normal)
        gen = gen.to(dev).eval()
        whole = timed_us(lambda: S.evaluate_scene(gen, b[0], 4, 54, 13), 2)
        metric = timed_us(lambda: (M.published_metrics_u8(a, b, 4, True), M.published_metrics_u8(a, b, 4, True)), 5)
        out.update({'evaluate_scene_ms': round(whole / 1e3, 1), 'its_two_metric_calls_ms': round(metric / 1e3, 3),
                    'metric_share_of_evaluate_scene': round(metric / whole, 5)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--scene', type=int, default=4096)
    ap.add_argument('--no-scene-sr', action='store_true')
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_metrics: needs a HIP device; there is nothing to time on the CPU')
    print(json.dumps(case1(a.reps, not a.no_torch)))
    print(json.dumps(case2(a.reps, a.scene, not a.no_torch, not a.no_scene_sr)))


if __name__ == '__main__':
    main()
