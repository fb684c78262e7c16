"""GDP diffusion sampling on one GPU at the reference's configuration (tests/golden/gdp_test_54_216.json: 128 base channels,
multipliers (1, 2, 4, 8), 2 ResBlocks per level, six attention blocks of 16 heads x 64 on 27 x 27 tokens, 216 x 216 images,
1000-step linear schedule), at B = 4 (the config's batch size) and B = 16:
  (a) ms per U-Net forward and per sampler step (forward + the update kernel) on the HIP path, in --math and in the other mode,
  (b) the six attention launches and the GroupNorm launches of one forward timed on their own, as a share of the forward,
  (c) seconds per 1000-step sample (1000 x the step time: the steps are identical), (d) peak device memory,
  (e) the same forward for the float32 restatement (tests/gdp_ref.py) run eagerly with ATen on the same GPU, same parameters: timed and
      its peak memory read BEFORE the first HIP forward, while no packed weight image exists yet; the bytes of the packed images the
      HIP path then holds beside the parameters are reported on their own,
  (f) PSNR between a 50-step sample in fp32 and in bf16x3 conv arithmetic with the same seed (B = 4).
Parameters are tests/gdp_ref.init_'s deterministic filler.  Every shape is warmed up first; each figure is timed with device events
over a window of at least --window seconds, all in one process.  One JSON line.
Usage: python tools/time_gdp.py [--batches 4,16] [--window 3] [--no-eager] [--no-psnr] [--math bf16x3]"""
import argparse
import json
import math
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import gdp_ref as R  # noqa: E402


def timed(fn, window_s, warmup):
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
    ap.add_argument('--batches', default='4,16')
    ap.add_argument('--window', type=float, default=3.0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--math', default='bf16x3')
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--no-psnr', action='store_true')
    ap.add_argument('--psnr-steps', type=int, default=50)
    a = ap.parse_args()
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp
    dev = torch.device('cuda:0')
    opt = json.loads(re.sub(r'//.*', '', open(os.path.join(ROOT, 'tests', 'golden', 'gdp_test_54_216.json')).read()))
    size = opt['model']['diffusion']['image_size']
    G = gdp.define_G(opt)
    R.init_(G.denoise_fn)
    G = G.to(dev)
    G.set_new_noise_schedule(opt['model']['beta_schedule']['val'], dev)
    net = G.denoise_fn
    other = 'fp32' if a.math == 'bf16x3' else 'bf16x3'
    out = {'metric': 'GDP sampling, %dx%d, %d steps, %s' % (size, size, G.num_timesteps, a.math),
           'params_M': round(sum(p.numel() for p in net.parameters()) / 1e6, 1)}
    batches = [int(v) for v in a.batches.split(',')]
    cfg = dict(model_channels=128, channel_mults=tuple(opt['model']['unet']['channel_multiplier']),
               res_blocks=opt['model']['unet']['res_blocks'])
    out['param_GiB'] = round(sum(p.numel() for p in net.parameters()) * 4 / 2.0 ** 30, 2)
    eager_rows, eager_out = {}, {}
    if not a.no_eager:                                   # first: nothing of the HIP path is resident yet
        sd = {k: v.detach() for k, v in net.state_dict().items()}
        for B in batches:
            x = O.det_fill('time.gdp.x%d' % B, (B, size, size, 6), 1.0).to(dev).permute(0, 3, 1, 2).contiguous()
            t = torch.full((B,), 500, device=dev, dtype=torch.long)

            def eager():
                with torch.no_grad():
                    return R.unet_forward(sd, x, t, cfg)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            ms = timed(eager, a.window, a.warmup)
            eager_rows[B] = {'eager_unet_ms': round(ms, 2), 'eager_peak_mem_GiB': round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 2)}
            eager_out[B] = eager().cpu()
            del x, t
        del sd
        torch.cuda.empty_cache()
    for B in batches:
        buf = O.det_fill('time.gdp.x%d' % B, (B, size, size, 6), 1.0).to(dev)
        emb = G._emb_rows(500, B, dev)
        row = {}
        for mode in (a.math, other):
            ops.set_conv_math(mode)
            torch.cuda.reset_peak_memory_stats(dev)
            row['unet_ms_' + mode] = round(timed(lambda: net.forward_embedded(buf.permute(0, 3, 1, 2), emb), a.window, a.warmup), 2)
            row['step_ms_' + mode] = round(timed(lambda: G._step(buf, 3, 500, None, 1, 1), a.window, a.warmup), 2)
            row['peak_mem_GiB_' + mode] = round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 2)
            row['sample_1000_steps_s_' + mode] = round(row['step_ms_' + mode] * G.num_timesteps / 1000.0, 1)
            buf.copy_(O.det_fill('time.gdp.x%d' % B, (B, size, size, 6), 1.0))
        ops.set_conv_math(a.math)
        qkv = O.det_fill('time.gdp.qkv', (B, 729, 3072), 1.0).to(dev)
        attn = 6 * timed(lambda: gdp.qkv_attention(qkv, 16), min(a.window, 1.0), a.warmup)
        gn_ms = 0.0
        for c, hw, count in gn_census(net, size):
            x = torch.empty(B, hw, c, device=dev).normal_()
            g = torch.ones(c, device=dev)
            gn_ms += count * timed(lambda: gdp.group_norm_act(x, g, g, silu=True), 0.2, 1)
        row['attention_ms_per_forward'] = round(attn, 2)
        row['attention_share_of_forward'] = round(attn / row['unet_ms_' + a.math], 3)
        row['group_norm_ms_per_forward'] = round(gn_ms, 2)
        row['group_norm_share_of_forward'] = round(gn_ms / row['unet_ms_' + a.math], 3)
        if not a.no_eager:
            row.update(eager_rows[B])
            row['unet_speedup_vs_eager'] = round(row['eager_unet_ms'] / row['unet_ms_' + a.math], 2)
            row['peak_mem_vs_eager'] = round(row['peak_mem_GiB_' + a.math] / row['eager_peak_mem_GiB'], 2)
            with torch.no_grad(), ops.conv_math('fp32'):
                y = net.forward_embedded(buf.permute(0, 3, 1, 2), emb).cpu()
            row['hip_fp32_vs_eager_rel'] = float((y - eager_out[B]).abs().max() / eager_out[B].abs().max())
        out['B%d' % B] = row
        del buf
        torch.cuda.empty_cache()
    packed = 0
    for p in net.parameters():                           # the persistent GEMM operands ops.packed_weight keeps per parameter
        for ent in getattr(p, '_srhip_packed', {}).values():
            packed += ent[2].numel() * 4
    out['packed_weight_GiB'] = round(packed / 2.0 ** 30, 2)
    if not a.no_psnr:
        B = 4
        sched = dict(opt['model']['beta_schedule']['val'], n_timestep=a.psnr_steps)
        G.set_new_noise_schedule(sched, dev)
        cond = O.det_fill('time.gdp.cond', (B, 3, size, size), 1.0).to(dev)
        imgs = {}
        for mode in ('fp32', 'bf16x3'):
            with ops.conv_math(mode):
                imgs[mode] = gdp.quantize_u8(G.super_resolution_batch(cond, seed=7).permute(0, 2, 3, 1)).double()
        mse = float(((imgs['fp32'] - imgs['bf16x3']) ** 2).mean())
        out['psnr_fp32_vs_bf16x3_%d_steps_dB' % a.psnr_steps] = round(10 * math.log10(255.0 ** 2 / mse), 2) if mse > 0 else 'identical'
        out['bytes_differing'] = float((imgs['fp32'] != imgs['bf16x3']).double().mean())
    print(json.dumps(out))


def gn_census(net, size):
    """(channels, pixels, count) of every GroupNorm launch of one forward."""
    import collections
    seen = collections.Counter()
    # walk the blocks as forward does: resolution halves after each `down` ResBlock and doubles after each `up`
    from sradsgan_amd.model.gdp import AttentionBlock, ResBlock
    hw = size * size
    for group in (net.input_blocks, [net.middle_block], net.output_blocks):
        for block in group:
            for layer in block:
                if isinstance(layer, ResBlock):
                    seen[(layer.channels, hw)] += 1
                    if layer.updown:
                        hw = hw * 4 if layer.h_upd.up else hw // 4
                    seen[(layer.out_channel, hw)] += 1
                elif isinstance(layer, AttentionBlock):
                    seen[(layer.channels, hw)] += 1
    seen[(net.out[0].num_channels, hw)] += 1
    return [(c, p, n) for (c, p), n in sorted(seen.items())]


if __name__ == '__main__':
    main()
