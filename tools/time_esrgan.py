"""ESRGAN throughput on one GPU: the HIP training step (esrgan.TrainStep: RRDBNet nb = 23 x4, Discriminator_VGG_*, VGGFeatureExtractor,
vanilla relativistic criterion) and generator inference against the fp32 restatement (tests/esrgan_ref.py) run eagerly with ATen in
the same process -- channels-last, autograd, fused torch.optim.Adam; its step reads its five scalars back to the host, as the
reference's loop does.  Two configurations: ESRGAN's own (B = 16, 32 -> 128, Discriminator_VGG_128) and UC Merced's (64 -> 256,
Discriminator_VGG_256).  The four figures of a configuration are timed in alternating blocks (HIP step, eager step, HIP inference,
eager inference), the whole sequence --runs times, each block with device events over a window of at least --window seconds after a
warm-up.  The shares of the dense head, the GAN criteria and the input normalisation are their own forward + backward launches at the
step's shapes timed in isolation (the count per step is 4 head passes, 2 criterion pairs, 2 + 1 normalisation passes), divided by the
step time.  One JSON line per configuration and run.
Usage: python tools/time_esrgan.py [--batch 16] [--window 2] [--runs 2] [--configs esrgan,ucmerced] [--no-eager]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import esrgan_ref as R  # noqa: E402

CONFIGS = {'esrgan': (32, 128), 'ucmerced': (64, 256)}
WEIGHTS = dict(weight_pixel=1e-2, weight_content=1.0, weight_gan=5e-3)


def timed(fn, window_s, warmup):
    """ms per call: warm-up calls, one probe call to size the window, then >= window_s seconds between two device events."""
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
    return t0.elapsed_time(t1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--window', type=float, default=2.0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--nb', type=int, default=23)
    ap.add_argument('--configs', default='esrgan,ucmerced')
    ap.add_argument('--no-eager', action='store_true')
    a = ap.parse_args()
    from sradsgan_amd.model import esrgan as E
    dev = torch.device('cuda:0')
    B = a.batch
    for name in a.configs.split(','):
        lr_side, hr_side = CONFIGS[name]
        ref_g = R.fill_generator(R.Generator(a.nb, 4), tag='time')
        ref_d = R.fill_discriminator(R.Discriminator(hr_side), hr_side)
        ref_f = R.fill_extractor(R.Vgg())
        x = O.det_fill('time.x', (B, 3, lr_side, lr_side), 0.5, 0.5).to(dev)
        t = O.det_fill('time.t', (B, 3, hr_side, hr_side), 0.5, 0.5).to(dev)
        G, D, F = E.RRDBNet(3, 3, 64, a.nb), E.DISCRIMINATORS[hr_side](3, 64), E.VGGFeatureExtractor()
        for net, ref in ((G, ref_g), (D, ref_d), (F, ref_f)):
            net.load_state_dict(ref.state_dict(), strict=True)
            net.to(dev)
        step = E.TrainStep(G, D, F, lr=1e-4, **WEIGHTS)

        def infer():
            with torch.no_grad():
                G(x)

        if not a.no_eager:
            EG, ED, EF = (m.to(dev).to(memory_format=torch.channels_last) for m in (ref_g, ref_d, ref_f))
            oG = torch.optim.Adam(EG.parameters(), lr=1e-4, betas=(0.9, 0.999), fused=True)
            oD = torch.optim.Adam(ED.parameters(), lr=1e-4, betas=(0.9, 0.999), fused=True)
            xe, te = x.contiguous(memory_format=torch.channels_last), t.contiguous(memory_format=torch.channels_last)

            def eager_step():
                R.train_iteration(EG, ED, EF, oG, oD, xe, te, 'vanilla', True, **WEIGHTS)

            def eager_infer():
                with torch.no_grad():
                    EG(xe)

        # the new kernels at the step's shapes, forward + backward, in isolation
        side = D.side
        feat = O.det_fill('time.feat', (B, 512, side, side), 1.0).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
        c = D.classifier
        logits_a = O.det_fill('time.la', (B, 1), 2.0).to(dev).requires_grad_()
        logits_b = O.det_fill('time.lb', (B, 1), 2.0).to(dev).requires_grad_()
        img = t.clone().requires_grad_()

        def head_pass():
            E.dhead(feat, c[0].weight, c[0].bias, c[2].weight, c[2].bias).sum().backward()

        def criterion_pair():
            E.ragan_pair_d(logits_a, logits_b, 'vanilla').backward()

        def norm_pass():
            E.input_norm(img, F.mean, F.std).backward(t)

        for run in range(a.runs):
            torch.cuda.reset_peak_memory_stats(dev)
            train_ms = timed(lambda: step(x, t), a.window, a.warmup)
            peak = torch.cuda.max_memory_allocated(dev)
            out = {'config': name, 'run': run, 'metric': 'ESRGAN x4 (RRDBNet nb=%d, B=%d, %d->%d, Discriminator_VGG_%d, vanilla RaGAN)'
                   % (a.nb, B, lr_side, hr_side, hr_side), 'train_ms': round(train_ms, 2), 'train_img_s': round(B * 1000.0 / train_ms, 1),
                   'peak_mem_train_GiB': round(peak / 2.0 ** 30, 2)}
            if not a.no_eager:
                torch.cuda.reset_peak_memory_stats(dev)
                e_train = timed(eager_step, a.window, a.warmup)
                out.update({'eager_train_ms': round(e_train, 2), 'eager_train_img_s': round(B * 1000.0 / e_train, 1),
                            'eager_peak_mem_train_GiB': round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 2),
                            'train_speedup': round(e_train / train_ms, 2)})
            G.eval()
            infer_ms = timed(infer, a.window, a.warmup)
            G.train()
            out.update({'infer_ms': round(infer_ms, 2), 'infer_img_s': round(B * 1000.0 / infer_ms, 1)})
            if not a.no_eager:
                e_infer = timed(eager_infer, a.window, a.warmup)
                out.update({'eager_infer_img_s': round(B * 1000.0 / e_infer, 1), 'infer_speedup': round(e_infer / infer_ms, 2)})
            head_ms, crit_ms, norm_ms = (timed(fn, 0.2, 3) for fn in (head_pass, criterion_pair, norm_pass))
            out.update({'head_share': round(4 * head_ms / train_ms, 4), 'criteria_share': round(2 * crit_ms / train_ms, 4),
                        'input_norm_share': round(3 * norm_ms / train_ms, 4), 'head_pass_ms': round(head_ms, 3),
                        'criterion_pair_ms': round(crit_ms, 3), 'input_norm_pass_ms': round(norm_ms, 3)})
            print(json.dumps(out), flush=True)
        del step, G, D, F
        if not a.no_eager:
            del EG, ED, EF, oG, oD
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
