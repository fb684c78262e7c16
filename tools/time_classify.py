"""Scene-classification timing on one GPU (sradsgan_amd/classify.py):
  (a) feature extraction, img/s at 256 x 256, B = 64: uint8 -> preprocess -> VGG19 trunk on the HIP path next to eager ATen fp32
      channels-last VGG19 (tests/classify_ref.vgg19_ref in float32) with the same weights, plus ms and TFLOP/s of every conv layer;
  (b) one head training step at K = 32768, m = 64, 21 classes: the HIP path (SceneClassifier.train_batch), the same step written with
      torch.mm, and its two forward GEMMs through ops.linear;
  (c) a UC-Merced-sized run end to end on synthetic tiles: 21 classes x 100 tiles of 256 x 256, channel means, features, split,
      fit (100 epochs), refit, evaluate -- wall seconds per stage.
Every shape is warmed up first; (a) and (b) are timed with device events over a window of at least --window seconds.  One JSON line.
Usage: python tools/time_classify.py [--batch 64] [--size 256] [--window 2] [--epochs 100] [--per-class 100] [--no-eager] [--no-features] [--no-run]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import classify_ref as C  # noqa: E402


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
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--window', type=float, default=2.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=100)
    ap.add_argument('--per-class', type=int, default=100)
    ap.add_argument('--math', default='bf16x3')
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--no-run', action='store_true')
    ap.add_argument('--no-features', action='store_true')
    a = ap.parse_args()
    from sradsgan_amd import classify as S, ops
    dev = torch.device('cuda:0')
    ops.set_conv_math(a.math)
    B, size = a.batch, a.size
    vgg = S.VGG19Features().to(dev)
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, size, size, 3), generator=g, dtype=torch.uint8).to(dev)
    means = S.channel_means(u8)
    out = {'metric': 'scene classification (B=%d, %dx%d, %s)' % (B, size, size, a.math)}

    # (a) feature extraction
    if not a.no_features:
        ms, _ = timed(lambda: S.features_of(u8, vgg, means), a.window, a.warmup)
        out['features_hip_img_s'] = round(B / ms * 1e3, 1)
        x = S.preprocess(u8, means)
        _, taps = vgg(x, taps=True)
        prev, layers = x.permute(0, 3, 1, 2), {}
        for i, t in taps:
            if i in S.CONVS:
                conv, src = vgg.features[i], prev
                lms, _ = timed(lambda: ops.conv2d_fwd_raw(src, conv.weight, conv.bias, 1, 1, slope=0.0), a.window / 8, a.warmup)
                flop = 2.0 * t.shape[0] * t.shape[2] * t.shape[3] * t.shape[1] * src.shape[1] * 9
                layers['features.%d %d->%d @%d' % (i, src.shape[1], t.shape[1], t.shape[2])] = [round(lms, 4), round(flop / lms * 1e-9, 1)]
            prev = t
        out['conv_layers_ms_tflops'] = layers
        if not a.no_eager:
            cl = torch.channels_last
            state = {k: (v.detach().contiguous(memory_format=cl) if v.dim() == 4 else v.detach()) for k, v in vgg.state_dict().items()}
            m32 = torch.as_tensor(means.astype(np.float32)).to(dev)

            def eager():
                with torch.no_grad():
                    xe = ((u8.float() - m32) * (1.0 / 255.0)).permute(0, 3, 1, 2)      # channels-last memory already
                    f = xe
                    for block in C.BLOCKS:
                        for i in block:
                            f = torch.relu(torch.nn.functional.conv2d(f, state['features.%d.weight' % i], state['features.%d.bias' % i], padding=1))
                        f = torch.nn.functional.max_pool2d(f, 2, 2)
                    return f
            ems, _ = timed(eager, a.window, a.warmup)
            out['features_eager_img_s'] = round(B / ems * 1e3, 1)
            out['features_speedup'] = round(ems / ms, 2)
            got = S.features_of(u8, vgg, means)
            out['features_hip_vs_eager_rel'] = float('%.2e' % C.err(got.reshape(B, size // 32, size // 32, 512), eager().permute(0, 2, 3, 1)))

    # (b) one head training step
    K, m, ncls = 32768, 64, 21
    head = S.SceneClassifier(ncls, (8, 8, 512), dev, seed=1)
    xb = torch.randn(m, K, generator=g).abs().to(dev)
    yb = torch.randint(0, ncls, (m,), generator=g, dtype=torch.int32).to(dev)
    hms, _ = timed(lambda: head.train_batch(xb, yb, 3), a.window, a.warmup)
    out['head_step_hip_ms'] = round(hms, 4)
    for name, fn in (('dense_fwd_ms', lambda: S.dense_fwd(xb, head.w1, head.b1, relu=True, dropout=(3, 0))),
                     ('dense_wgrad_ms', lambda: S.dense_wgrad(xb, torch.ones(m, S.HIDDEN, device=dev), head.gw1, head.gb1))):
        t_ms, _ = timed(fn, a.window / 4, a.warmup)
        out[name] = round(t_ms, 4)
    out['dense_fwd_w_stream_TBs'] = round(K * S.HIDDEN * 4 / out['dense_fwd_ms'] * 1e-9, 3)
    out['dense_wgrad_write_TBs'] = round(K * S.HIDDEN * 4 / out['dense_wgrad_ms'] * 1e-9, 3)
    if not a.no_eager:
        w1, b1, w2, b2 = (t.clone() for t in (head.w1, head.b1, head.w2, head.b2))
        params = [w1, b1, w2, b2]
        for p in params:
            p.grad = torch.zeros_like(p)
        try:                                                         # the baseline at its best: one fused optimiser kernel,
            opt = torch.optim.Adam(params, lr=S.LR, betas=(S.B1, S.B2), eps=S.EPS, fused=True)
            out['head_step_torch_mm_adam'] = 'fused'
        except (RuntimeError, TypeError):
            opt = torch.optim.Adam(params, lr=S.LR, betas=(S.B1, S.B2), eps=S.EPS)
            out['head_step_torch_mm_adam'] = 'default'
        yl = yb.long()
        onehot = torch.nn.functional.one_hot(yl, ncls).float()

        def mm_step():
            with torch.no_grad():
                pre = torch.mm(xb, w1) + b1
                keep = (torch.rand_like(pre) < 0.5).float() * 2.0
                h = pre.clamp_min(0) * keep
                z = torch.mm(h, w2) + b2
                p = torch.softmax(z, 1)
                loss = -torch.log_softmax(z, 1).gather(1, yl[:, None]).mean()
                dz = (p - onehot) / m
                torch.mm(h.t(), dz, out=w2.grad)                     # ... and gradients written where the optimiser reads them
                torch.sum(dz, 0, out=b2.grad)
                dpre = torch.mm(dz, w2.t()) * keep * (pre > 0).float()
                torch.mm(xb.t(), dpre, out=w1.grad)
                torch.sum(dpre, 0, out=b1.grad)
                opt.step()
                return loss
        mms, _ = timed(mm_step, a.window, a.warmup)
        out['head_step_torch_mm_ms'] = round(mms, 4)
        wt1, wt2 = w1.t().contiguous(), w2.t().contiguous()          # ops.linear takes nn.Linear's [out, in] weight
        x4 = xb.view(m, K, 1, 1).contiguous(memory_format=torch.channels_last)

        def linear_fwd():
            with torch.no_grad():
                return ops.linear(ops.linear(x4, wt1, b1).clamp_min(0), wt2, b2)      # the 1x1 conv route on [m, K, 1, 1]
        try:
            lms, _ = timed(linear_fwd, a.window / 4, a.warmup)
            out['head_fwd_ops_linear_ms'] = round(lms, 4)
        except Exception as e:                                       # ops.linear serves the generators' shapes; report, do not hide
            out['head_fwd_ops_linear_ms'] = 'not served: %s' % (str(e)[:120],)
        fms, _ = timed(lambda: head.logits(xb), a.window / 4, a.warmup)
        out['head_fwd_hip_ms'] = round(fms, 4)

    # (c) a UC-Merced-sized run on synthetic tiles
    if not a.no_run:
        ncls, per = 21, a.per_class
        t0 = time.time()
        small, labels = C.synthetic_tiles(classes=ncls, per_class=per, size=32, seed=5)
        tiles = torch.from_numpy(small).to(dev).permute(0, 3, 1, 2).repeat_interleave(size // 32, 2).repeat_interleave(size // 32, 3)
        tiles = tiles.permute(0, 2, 3, 1).contiguous()                # [2100, size, size, 3] uint8
        torch.cuda.synchronize()
        t1 = time.time()
        batches = [tiles[i:i + B] for i in range(0, tiles.shape[0], B)]
        mu = S.channel_means(batches)
        feats = torch.cat([S.features_of(b, vgg, mu) for b in batches])
        torch.cuda.synchronize()
        t2 = time.time()
        tr, va, te = S.split_indices(labels, 0)
        head = S.SceneClassifier(ncls, (size // 32, size // 32, 512), dev)
        hist, best = head.fit(feats[tr], labels[tr], feats[va], labels[va], epochs=a.epochs, batch_size=64, seed=0)
        torch.cuda.synchronize()
        t3 = time.time()
        head.refit(torch.cat([feats[tr], feats[va]]), np.concatenate([labels[tr], labels[va]]), best, seed=0)
        torch.cuda.synchronize()
        t4 = time.time()
        res = head.evaluate(feats[te], labels[te])
        t5 = time.time()
        out['run'] = {'tiles': int(tiles.shape[0]), 'epochs': a.epochs, 'best_epoch': best, 'make_tiles_s': round(t1 - t0, 2),
                      'means_and_features_s': round(t2 - t1, 2), 'fit_s': round(t3 - t2, 2), 'refit_s': round(t4 - t3, 2),
                      'evaluate_s': round(t5 - t4, 3), 'total_s': round(t5 - t1, 2), 'test_accuracy': round(res['accuracy'], 4),
                      'peak_mem_GB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
