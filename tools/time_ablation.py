"""Attention ablations of the generator at the benchmark configuration (12 groups x 3 blocks, x4, 54 -> 216, split-bf16 convs) on one GPU.

Per configuration of tests/attn_variants_ref.GEN_CONFIGS and for the default:
  inference (B = 16, grad mode off)   the variant tails on csrc/attn_variants.hip, and the same with that route forced to the
                                      composition of srhip_cbam_* primitives (the predicate ops.attention_variant_supported is
                                      patched here: no debug key).  The two are alternated call by call in one process after a warm-up,
                                      --calls calls each; median with min .. max, img/s, and the peak memory of one call of each
                                      (peak_MB everywhere: the high-water mark above what was allocated when the measurement began).
  training step (B = 32)              TrainStep with the variant generator, the same two routes alternated step by step, --steps
                                      each.  --no-train skips it.
For --aten configurations also the oracle's generator (oracle/sradsgan_ref.py) run eagerly with ATen on the same GPU, fp32,
channels-last, grad mode off.  The bytes each tail form reads and writes are computed from the shapes.
Run the same command twice to see the run-to-run spread.  Prints one JSON line per configuration; --table FILE ... (no GPU) prints
the files of such lines, one per run, as the table of profiles/ablation_timing.txt.
Usage: python tools/time_ablation.py [--calls 20] [--steps 20] [--no-train] [--aten 2] [--only TAG ...]
       python tools/time_ablation.py --table profiles/ablation_timing_run1.jsonl profiles/ablation_timing_run2.jsonl"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attn_variants_ref as V  # noqa: E402

DEV = torch.device('cuda:0')
GROUPS, BLOCKS, SCALE, LR = 12, 3, 4, 54
DEFAULT = ('CA-SA', 'CA-SA', 'CA-SA', 'Avg|Max', True)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def fig(ms, batch):
    med = statistics.median(ms)
    return dict(ms=round(med, 3), min=round(min(ms), 3), max=round(max(ms), 3), img_s=round(batch * 1000.0 / med, 1))


def tail_bytes(mode, pool, addconv, n, hw):
    """HBM bytes of one tail + skip add (activations only; the gates and pooled maps are n * hw * 4-byte rows and smaller):
    fused = the passes of csrc/attn_variants.hip and the closing kernel / conv; composed = the primitive chain, every gated
    activation written and read back."""
    t = n * hw * 64 * 4
    gates = ('CA' in mode) + ('SA' in mode)
    fused = gates * t                                   # one pooling pass over u per gate
    composed = gates * (t + 2 * t)                      # pool (read) + scale (read, write) per gate
    if mode == 'CA|SA':
        fused += t + 2 * t + 2 * t + t + t              # gated cat: read u, write 2t; conv reads 2t + skip, writes t
        composed += 2 * t + 2 * t + 2 * t + t + t       # cat: read 2t, write 2t; the same conv
    elif '-' in mode and addconv:
        fused += t + t + t                              # conv reads u (gates folded) + skip, writes out
        composed += t + t + t                           # conv reads z + skip, writes out
    else:
        fused += t + t + t                              # gate-and-add: u, skip -> out ('': the plain 1x1 conv, the same bytes)
        composed += t + t + t                           # z + skip -> out
    return dict(fused_MB=round(fused / 2 ** 20, 1), composed_MB=round(composed / 2 ** 20, 1))


def build(cfg):
    from sradsgan_amd import model as M
    rla, bla, ga, pool, addconv = cfg
    torch.manual_seed(0)
    g = M.GeneratorResNet(M.ResGroup, n_residual_blocks=GROUPS, n_basic_blocks=BLOCKS, rla_mode=rla, bla_mode=bla, ga_mode=ga,
                          pool_mode=pool, addconv=addconv, upscale_factor=SCALE)
    for m in g.modules():
        if hasattr(m, 'gamma'):
            torch.nn.init.constant_(m.gamma, 0.5)
    return g.to(DEV)


def inference(g, a, cfg):
    from sradsgan_amd import ops
    x = torch.rand(16, 3, LR, LR, device=DEV)
    real = ops.attention_variant_supported
    routes = {'fused': real, 'composed': lambda *args: False}
    if cfg == DEFAULT:
        routes = {'fused': real}                        # the default tail has routes of its own (attn_tail.hip); nothing to force
    ms, peak = {k: [] for k in routes}, {}
    g.eval()
    with torch.no_grad(), ops.conv_math('bf16x3'):
        try:
            for k, pred in routes.items():
                ops.attention_variant_supported = pred
                for _ in range(3):
                    g(x)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()         # weights, x and whatever earlier configurations left cached in the package
                g(x)
                torch.cuda.synchronize()
                peak[k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            for _ in range(a.calls):
                for k, pred in routes.items():
                    ops.attention_variant_supported = pred
                    ms[k].append(timed(lambda: g(x)))
        finally:
            ops.attention_variant_supported = real
    out = {k: dict(fig(v, 16), peak_MB=peak[k]) for k, v in ms.items()}
    if 'composed' in ms:
        out['fused_over_composed'] = round(statistics.median(ms['fused']) / statistics.median(ms['composed']), 4)
    return out


def training(g, a, cfg):
    from sradsgan_amd import model as M, ops
    from sradsgan_amd.train_step import TrainStep
    torch.manual_seed(1)
    step = TrainStep(g, M.Discriminator().to(DEV), M.FeatureExtractor().to(DEV))
    lr, hr = torch.rand(32, 3, LR, LR, device=DEV), torch.rand(32, 3, LR * SCALE, LR * SCALE, device=DEV)
    alpha = torch.rand(32, 1, 1, 1, device=DEV)
    real = ops.attention_variant_supported
    routes = {'fused': real} if cfg == DEFAULT else {'fused': real, 'composed': lambda *args: False}
    ms, peak = {k: [] for k in routes}, {}
    g.train()
    with ops.conv_math('bf16x3'):
        try:
            for k, pred in routes.items():
                ops.attention_variant_supported = pred
                for _ in range(3):
                    step(lr, hr, alpha)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step(lr, hr, alpha)
                torch.cuda.synchronize()
                peak[k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            for _ in range(a.steps):
                for k, pred in routes.items():
                    ops.attention_variant_supported = pred
                    ms[k].append(timed(lambda: step(lr, hr, alpha)))
        finally:
            ops.attention_variant_supported = real
    out = {k: dict(fig(v, 32), peak_MB=peak[k]) for k, v in ms.items()}
    if 'composed' in ms:
        out['fused_over_composed'] = round(statistics.median(ms['fused']) / statistics.median(ms['composed']), 4)
    return out


def aten(cfg, a):
    from oracle import sradsgan_ref as O
    rla, bla, ga, pool, addconv = cfg
    g = O.GeneratorResNet(O.ResGroup, n_residual_blocks=GROUPS, n_basic_blocks=BLOCKS, rla_mode=rla, bla_mode=bla, ga_mode=ga, pool_mode=pool,
                          addconv=addconv, upscale_factor=SCALE).to(DEV).to(memory_format=torch.channels_last).eval()
    x = torch.rand(16, 3, LR, LR, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        for _ in range(3):
            g(x)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = [timed(lambda: g(x)) for _ in range(a.calls)]
    return dict(fig(ms, 16), peak_MB=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))


TABLE_HEAD = """tools/time_ablation.py, one file of JSON lines per run (named below), on one MI355X: the generator's attention ablations at the
benchmark configuration -- 12 groups x 3 blocks, x4, LR 54 x 54 -> 216 x 216, split-bf16 convs.  config = rla_bla_ga_pool_addconv
(m = '-', p = '|', none = '').  Times are medians of the run's calls / steps with min .. max; peak MB is the high-water mark of one
call / step above what was allocated when the measurement began.

"fused" = the variant tails as one autograd node on csrc/attn_variants.hip; "composed" = the same tails forced to the srhip_cbam_*
composition (ops.attention_variant_supported patched in the tool), alternated call by call with "fused" in the same process.
The default's tail is attn_tail.hip's own fusion (no composed leg).  inference: B = 16, grad mode off.  training: TrainStep, B = 32.
aten: the oracle's generator run eagerly with ATen on the same GPU, fp32, channels-last, grad mode off, B = 16.
"""


def table(files):
    """The JSON lines of one or more runs as text: per run a row per configuration, then the bytes per tail form."""
    def leg(d, k):
        x = d.get(k) if d else None
        return ('%6.2f [%6.2f..%6.2f] %7.1f %6.0f' % (x['ms'], x['min'], x['max'], x['img_s'], x['peak_MB'])) if x else '%-38s' % 'n/a'

    def ratio(d):
        return ('%.3f' % d['fused_over_composed']) if d and 'fused_over_composed' in d else ''
    print(TABLE_HEAD)
    rows = []
    for path in files:
        rows = [json.loads(line) for line in open(path) if line.strip()]
        print('%s          columns per leg: ms [min..max] img/s peakMB' % os.path.basename(path))
        print('%-36s | %-38s | %-38s | %-5s | %-38s | %-38s | %-5s | %s' % ('config', 'inference fused', 'inference composed', 'f/c',
                                                                            'train fused', 'train composed', 'f/c', 'aten ms'))
        for r in rows:
            i, t, at = r['inference_b16'], r.get('train_b32'), r.get('aten_eager_fp32_b16')
            print('%-36s | %s | %s | %-5s | %s | %s | %-5s | %s' % (r['config'], leg(i, 'fused'), leg(i, 'composed'), ratio(i), leg(t, 'fused'),
                                                                    leg(t, 'composed'), ratio(t), ('%.2f' % at['ms']) if at else ''))
        print()
    print('HBM bytes of ONE tail forward + skip add at B = 16 (activations only, from the shapes; tail_bytes), MB: fused / composed')
    for r in rows:
        b = r['tail_bytes_b16']
        print('%-36s group tail %6.1f / %6.1f    block tail %6.1f / %6.1f' % (r['config'], b['group']['fused_MB'], b['group']['composed_MB'],
                                                                              b['block']['fused_MB'], b['block']['composed_MB']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--aten', type=int, default=2, help='how many of the configurations also run the oracle eagerly with ATen')
    ap.add_argument('--only', nargs='*', default=None)
    ap.add_argument('--table', nargs='+', default=None, help='print these files of JSON lines as a table and exit')
    a = ap.parse_args()
    if a.table:
        return table(a.table)
    for i, cfg in enumerate([DEFAULT] + V.GEN_CONFIGS):
        tag = 'default' if cfg == DEFAULT else V.gen_tag(cfg)
        if a.only and tag not in a.only:
            continue
        g = build(cfg)
        row = dict(config=tag, inference_b16=inference(g, a, cfg))
        row['tail_bytes_b16'] = {'group': tail_bytes(cfg[0], cfg[3], cfg[4], 16, LR * LR), 'block': tail_bytes(cfg[1], cfg[3], cfg[4], 16, LR * LR)}
        if not a.no_train:
            row['train_b32'] = training(g, a, cfg)
        del g
        torch.cuda.empty_cache()
        if 0 < i <= a.aten:
            row['aten_eager_fp32_b16'] = aten(cfg, a)
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
