"""Spectral normalisation on one GPU.

Kernel times: the batched power iteration (srhip_sn_forward_batched: 4 launches) and the batched projection
(srhip_sn_backward_batched: 2 launches) for the 8 wrapped convs of the patch discriminator, beside the same arithmetic written with
torch ops on the same device (per layer: 2 mv, 2 norms, 2 divisions, dot, mv, division, 2 copies into the parameters; projection:
mul-sum, outer, 2 divisions, mul, sub, add).
Step times at the benchmark's shape (B = 32, x4, HR 216 x 216): TrainStep with the spectral discriminator and with the non-spectral
PatchDiscriminator of the same norm_type, both on the plain order (reuse_d_fake=False), beside the default one-walk step of the
non-spectral one; and one D forward pass alone, with and without the spectral layers.
Every figure: warm-up, device events, --trials trials of --iters calls; the median with min .. max.  One box, one JSON line.
Usage: python tools/time_spectral.py [--batch 32] [--norm-type ''] [--trials 5] [--iters 10] [--no-steps]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D_SHAPES = [(64, 27), (64, 576), (128, 576), (128, 1152), (256, 1152), (256, 2304), (512, 2304), (512, 4608)]
DEV = torch.device('cuda:0')


def trials(fn, n_trials, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_trials):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / iters)
    return out


def fig(ms):
    return dict(ms=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def kernel_figures(a):
    from sradsgan_amd import ops
    gen = torch.Generator().manual_seed(1)
    layers = []
    for c, k in D_SHAPES:
        u, v = torch.randn(c, generator=gen), torch.randn(k, generator=gen)
        layers.append(((torch.randn(c, k, generator=gen) * 0.02).to(DEV), (u / u.norm()).to(DEV), (v / v.norm()).to(DEV)))
    grads = [torch.randn(c, k, generator=gen).to(DEV) for c, k in D_SHAPES]
    slots = [torch.zeros(c, k, device=DEV) for c, k in D_SHAPES]
    table = ops.SpectralTable(layers)
    out, _ = table.forward()

    def torch_forward():
        res = []
        for w, u, v in layers:
            t = w.t() @ u
            vn = t / (t.norm() + 1e-12)
            s = w @ vn
            un = s / (s.norm() + 1e-12)
            sigma = torch.dot(un, w @ vn)
            u.copy_(un), v.copy_(vn)
            res.append((w / sigma, sigma))
        return res

    sigmas = [table.snapshot(out, i)[2] for i in range(len(layers))]

    def torch_backward():
        for (w, u, v), g, s, sigma in zip(layers, grads, slots, sigmas):
            s.add_(g / sigma - (g * w).sum() / (sigma * sigma) * torch.outer(u, v))

    return dict(forward_hip=fig(trials(lambda: table.forward(), a.trials, a.iters)),
                forward_torch_ops=fig(trials(torch_forward, a.trials, a.iters)),
                backward_hip=fig(trials(lambda: table.backward(out, grads, slots), a.trials, a.iters)),
                backward_torch_ops=fig(trials(torch_backward, a.trials, a.iters)),
                bytes_weights=4 * sum(c * k for c, k in D_SHAPES))


def step_figures(a):
    from sradsgan_amd import model as M
    from sradsgan_amd.model.spectral import spectral_init_
    from sradsgan_amd.train_step import TrainStep
    from sradsgan_amd.trainer import weights_init_normal
    B, side, scale = a.batch, 54, 4
    gen = torch.Generator().manual_seed(0)
    hr = torch.rand(B, 3, side * scale, side * scale, generator=gen).to(DEV)
    lr = torch.rand(B, 3, side, side, generator=gen).to(DEV)
    alpha = torch.rand(B, 1, 1, 1, generator=gen).to(DEV)
    res = {}
    for name, spectral, reuse in (('spectral_plain_order', True, False), ('patch_plain_order', False, False), ('patch_one_walk', False, True)):
        torch.manual_seed(0)
        G = M.GeneratorResNet(M.ResGroup, n_residual_blocks=12, n_basic_blocks=3, upscale_factor=scale).apply(weights_init_normal)
        if spectral:
            D = spectral_init_(M.SpectralPatchDiscriminator(norm_type=a.norm_type))
        else:
            D = M.PatchDiscriminator(norm_type=a.norm_type).apply(weights_init_normal)
        step = TrainStep(G.to(DEV), D.to(DEV), M.FeatureExtractor().to(DEV), reuse_d_fake=reuse)
        res['step_' + name] = fig(trials(lambda: step(lr, hr, alpha), a.trials, a.iters, warmup=2))
        with torch.no_grad():
            res['d_forward_' + name.split('_')[0]] = fig(trials(lambda: D(hr), a.trials, a.iters))
        del step, G, D
        torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--norm-type', default='')
    p.add_argument('--trials', type=int, default=5)
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--no-steps', action='store_true')
    a = p.parse_args()
    res = dict(kernels=kernel_figures(a))
    if not a.no_steps:
        res['steps'] = step_figures(a)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
