"""GDP diffusion training on one GPU at the reference's configuration (tests/golden/gdp_test_54_216.json: the full U-Net, 216 x 216,
1000-step linear schedule, Adam at the config's learning rate), at B = 4 and B = 16: one DDPM.optimize_parameters() per measurement.
  (a) ms per step on the HIP path in bf16x3 and in fp32 conv arithmetic, and its peak device memory,
  (b) the same step for the float32 restatement (tests/gdp_ref.py) run eagerly with ATen autograd and fused torch.optim.Adam on the
      same GPU, same parameters: timed, and its peak memory read, BEFORE the HIP path has allocated anything,
  (c) the attention backward launches and the GroupNorm backward launches of one step timed on their own (as tools/time_gdp.py times
      the forward ones), as a share of the bf16x3 step.
Peak memory is torch.cuda.max_memory_allocated on both sides: the peak of torch's caching allocator (every buffer of either path comes
from it), not the device's own figure, which also holds the allocator's cached blocks, the code objects and the runtime's pools.  The
`fp32` peak is read with the `bf16x3` run's packed images still resident.
Parameters are tests/gdp_ref.init_'s deterministic filler.  Each figure is timed with device events over a window of at least --window
seconds after a warm-up, all in one process.  Every finished row is also written to --out as it is measured.  One JSON line.
Usage: python tools/time_gdp_train.py [--batches 4,16] [--window 1] [--no-eager] [--out FILE]"""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import sradsgan_ref as O  # noqa: E402
from tests import gdp_ref as R  # noqa: E402
from time_gdp import gn_census, timed  # noqa: E402


def batch(B, size, dev):
    hr = O.det_fill('time.gdp.train.hr%d' % B, (B, 3, size, size), 1.0).to(dev)
    sr = O.det_fill('time.gdp.train.sr%d' % B, (B, 3, size, size), 1.0).to(dev)
    noise = O.det_fill('time.gdp.train.z%d' % B, (B, 3, size, size), 1.7).to(dev)
    t = (torch.arange(B, device=dev) * 997 % 1000).long()
    return hr, sr, noise, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='4,16')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-eager', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp_train
    dev = torch.device('cuda:0')
    opt = json.loads(re.sub(r'//.*', '', open(os.path.join(ROOT, 'tests', 'golden', 'gdp_test_54_216.json')).read()))
    opt['phase'] = 'train'
    opt['path']['resume_state'] = None
    size = opt['model']['diffusion']['image_size']
    lr = opt['train']['optimizer']['lr']
    G = gdp_train.define_G(opt)
    R.init_(G.denoise_fn)
    net = G.denoise_fn
    batches = [int(v) for v in a.batches.split(',')]
    out = {'metric': 'GDP training step, %dx%d, Adam lr %g' % (size, size, lr),
           'params_M': round(sum(p.numel() for p in net.parameters()) / 1e6, 1)}

    def emit():
        if a.out:
            with open(a.out, 'w') as f:
                f.write(json.dumps(out) + '\n')

    cfg = dict(model_channels=128, channel_mults=tuple(opt['model']['unet']['channel_multiplier']), res_blocks=opt['model']['unet']['res_blocks'])
    eager_rows = {}
    if not a.no_eager:                                   # first: nothing of the HIP path is resident yet
        sd = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in net.state_dict().items()}
        adam = torch.optim.Adam(list(sd.values()), lr=lr, fused=True)
        for B in batches:
            hr, sr, noise, t = batch(B, size, dev)
            x = torch.cat([0.6 * hr + 0.8 * noise, sr], dim=1)

            def eager():
                adam.zero_grad(set_to_none=False)
                loss = ((R.unet_forward(sd, x, t, cfg) - hr) ** 2).sum() / hr.numel()
                loss.backward()
                adam.step()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            ms = timed(eager, a.window, a.warmup)
            eager_rows[B] = {'eager_step_ms': round(ms, 1), 'eager_peak_mem_GiB': round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 2)}
            out['eager_B%d' % B] = eager_rows[B]
            emit()
            del hr, sr, noise, t, x
        del sd, adam
        torch.cuda.empty_cache()
    model = gdp_train.DDPM(opt, netG=G)
    for B in batches:
        hr, sr, noise, t = batch(B, size, dev)
        model.feed_data({'HR': hr, 'SR': sr, 'LR': sr})
        row = {}
        for mode in ('bf16x3', 'fp32'):
            ops.set_conv_math(mode)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            row['step_ms_' + mode] = round(timed(lambda: model.optimize_parameters(noise, t=t), a.window, a.warmup), 1)
            row['peak_mem_GiB_' + mode] = round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 2)
            out['B%d' % B] = row
            emit()
        ops.set_conv_math('bf16x3')
        row['loss_after'] = float(model.log_dict['l_pix'])
        qkv = O.det_fill('time.gdp.qkv', (B, 729, 3072), 1.0).to(dev)
        dout = O.det_fill('time.gdp.dout', (B, 729, 1024), 1.0).to(dev)
        qkv, o, lse = gdp_train.attention_fwd_lse(qkv, 16)
        attn = 6 * timed(lambda: gdp_train.attention_bwd_raw(qkv, o, lse, dout, 16), min(a.window, 1.0), a.warmup)
        attn_fwd = 6 * timed(lambda: gdp_train.attention_fwd_lse(qkv, 16), min(a.window, 1.0), a.warmup)
        gn_ms = 0.0
        for c, hw, count in gn_census(net, size):
            x = torch.empty(B, hw, c, device=dev).normal_()
            dy = torch.empty(B, hw, c, device=dev).normal_()
            g = torch.ones(c, device=dev)
            _, stats = gdp_train.group_norm_fwd_raw(x, g, g, None, True)
            gn_ms += count * timed(lambda: gdp_train.group_norm_bwd_raw(dy, x, stats, g, g, None, True), 0.2, 1)
            del x, dy
        step = row['step_ms_bf16x3']
        row.update({'attention_bwd_ms_per_step': round(attn, 2), 'attention_bwd_share_of_step': round(attn / step, 3),
                    'attention_fwd_lse_ms_per_step': round(attn_fwd, 2), 'group_norm_bwd_ms_per_step': round(gn_ms, 2),
                    'group_norm_bwd_share_of_step': round(gn_ms / step, 3)})
        if B in eager_rows:
            row.update(eager_rows[B])
            row['step_speedup_vs_eager'] = round(eager_rows[B]['eager_step_ms'] / step, 2)
            row['peak_mem_vs_eager'] = round(row['peak_mem_GiB_bf16x3'] / eager_rows[B]['eager_peak_mem_GiB'], 2)
        out['B%d' % B] = row
        emit()
        del hr, sr, noise, t, qkv, dout, o, lse
        torch.cuda.empty_cache()
    packed = 0
    for p in net.parameters():
        for ent in getattr(p, '_srhip_packed', {}).values():
            packed += ent[2].numel() * 4
    out['packed_weight_GiB'] = round(packed / 2.0 ** 30, 2)
    out['arena_GiB'] = round(model.arena.numel * 16 / 2.0 ** 30, 2)
    emit()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
