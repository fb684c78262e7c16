"""The discriminator's normalisations on one GPU.

Kernel times: at B = 32 with a 216 x 216 input, over the seven normalised layers of the patch discriminator (64@108^2, 128@108^2,
128@54^2, 256@54^2, 256@27^2, 512@27^2, 512@14^2), the three gn.hip entry points (forward, backward, second-order backward; group
norm: 32 groups, unbiased, affine; instance norm: groups = C, no affine) beside the matching bn.hip entry points (train_fwd,
train_bwd_acc_x, train_bwd_bwd_acc_x) on the same shapes in the same run, with the achieved bytes/s of each under the traffic both
families are designed to: forward 2 reads + 1 write, backward 4 + 1, second order 6 + 2 tensor passes.
Step times: the D phase (D(real), D(fake), the gradient penalty and their backward) and the whole TrainStep for norm_type 'batch',
'', 'instance' and 'group', each against eager ATen fp32 channels-last running tests/disc_norms_ref.py's discriminator.
Every figure: warm-up, device events, --trials trials of --iters calls; the median with min .. max.  One box, one JSON line.
Usage: python tools/time_d_norms.py [--batch 32] [--trials 5] [--iters 10] [--no-steps] [--no-eager]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from tests import disc_norms_ref as DR  # noqa: E402

LAYERS = [(64, 108), (128, 108), (128, 54), (256, 54), (256, 27), (512, 27), (512, 14)]
PASSES = {'fwd': 3, 'bwd': 5, 'bwd2': 8}          # tensor passes over HBM


def trials(fn, n_trials, iters, warmup=3):
    """[ms per call] over n_trials windows of `iters` calls between two device events."""
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


def fig(ms, nbytes=None):
    d = dict(ms=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))
    if nbytes is not None:
        d['TBps'] = round(nbytes / (statistics.median(ms) * 1e-3) / 1e12, 3)
    return d


def kernel_table(B, a):
    from sradsgan_amd import _hip
    lib, dev = _hip.lib(), torch.device('cuda:0')
    p_ = lambda t: t.data_ptr() if t is not None else None                       # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for c, side in LAYERS:
        p = side * side
        x, dy, u = (torch.randn(B, p, c, device=dev) for _ in range(3))
        y, o1, o2 = (torch.empty_like(x) for _ in range(3))
        gamma, beta = 1 + 0.1 * torch.randn(c, device=dev), 0.1 * torch.randn(c, device=dev)
        dg, db = torch.empty_like(gamma), torch.empty_like(gamma)
        nbytes = B * p * c * 4
        row = dict(layer='%d@%d^2' % (c, side))
        # bn.hip
        rows_ = B * p
        ws = torch.empty(max(lib.srhip_bn_workspace(rows_, c), lib.srhip_bn_bwd2_workspace(rows_, c)) // 4 + 2, device=dev)
        mean, invstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
        tail = (p_(ws), ws.numel() * 4, rows_, c)
        bn = dict(
            fwd=lambda: _hip.check(lib.srhip_bn_train_fwd(p_(x), p_(gamma), p_(beta), None, None, p_(y), p_(mean), p_(invstd), *tail, 1e-5, 0.1, 0.2, 1, st)),
            bwd=lambda: _hip.check(lib.srhip_bn_train_bwd_acc_x(p_(dy), p_(x), p_(gamma), p_(beta), p_(mean), p_(invstd), p_(o1), p_(dg), p_(db), None, None,
                                                                *tail, 0.2, 1, st)),
            bwd2=lambda: _hip.check(lib.srhip_bn_train_bwd_bwd_acc_x(p_(u), p_(dy), p_(x), p_(gamma), p_(beta), p_(mean), p_(invstd), p_(o1), p_(o2), p_(dg),
                                                                     None, *tail, 0.2, 1, st)))
        for k in PASSES:
            row['bn_' + k] = fig(trials(bn[k], a.trials, a.iters), PASSES[k] * nbytes)
        # gn.hip: the group kind and the instance kind
        gws = torch.empty(lib.srhip_gn_workspace(B, p, c) // 4, device=dev)
        for kind, groups, unb, ga, be in (('group', 32, 1, gamma, beta), ('instance', c, 0, None, None)):
            gm, gi = torch.empty(B * groups, device=dev), torch.empty(B * groups, device=dev)
            dims = (p_(gws), gws.numel() * 4, B, p, c, groups, unb)
            has = ga is not None
            gn = dict(
                fwd=lambda: _hip.check(lib.srhip_gn_fwd(p_(x), p_(ga), p_(be), p_(y), p_(gm), p_(gi), *dims, 1e-5, 0.2, 1, st)),
                bwd=lambda: _hip.check(lib.srhip_gn_bwd(p_(dy), p_(x), p_(ga), p_(be), p_(gm), p_(gi), None, p_(o1), p_(dg) if has else None,
                                                        p_(db) if has else None, None, None, *dims, 0.2, 1, st)),
                bwd2=lambda: _hip.check(lib.srhip_gn_bwd_bwd(p_(u), p_(dy), p_(x), p_(ga), p_(be), p_(gm), p_(gi), p_(o1), p_(o2),
                                                             p_(dg) if has else None, None, *dims, 0.2, 1, st)))
            for k in PASSES:
                row['%s_%s' % (kind, k)] = fig(trials(gn[k], a.trials, a.iters), PASSES[k] * nbytes)
                row['%s_%s' % (kind, k)]['vs_bn'] = round(row['%s_%s' % (kind, k)]['ms'] / row['bn_' + k]['ms'], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def step_table(B, a):
    from sradsgan_amd import model as M
    from sradsgan_amd.train_step import TrainStep
    dev = torch.device('cuda:0')
    og = O.det_init_(O.GeneratorResNet(O.ResGroup, n_residual_blocks=12, n_basic_blocks=3, upscale_factor=8), prefix='G.')
    of = O.det_init_(O.FeatureExtractor(), prefix='F.')
    lr_img = O.det_fill('time.lr', (B, 3, 27, 27), 0.5, 0.5).to(dev)
    hr_img = O.det_fill('time.hr', (B, 3, 216, 216), 0.5, 0.5).to(dev)
    alpha = O.det_fill('time.alpha', (B, 1, 1, 1), 0.5, 0.5).to(dev)
    out = {}
    for nt in ('batch', '', 'instance', 'group'):
        od = DR.fill_(DR.Discriminator(norm_type=nt, attention=True), 0, 1.0)
        hd = M.PatchDiscriminator(norm_type=nt, attention=True)
        hd.load_state_dict(od.state_dict(), strict=True)
        hg, hf = M.GeneratorResNet(M.ResGroup, upscale_factor=8), M.FeatureExtractor()
        hg.load_state_dict(og.state_dict()), hf.load_state_dict(of.state_dict())
        step = TrainStep(hg.to(dev), hd.to(dev), hf.to(dev))
        row = dict(step=fig(trials(lambda: step(lr_img, hr_img, alpha), a.trials, max(2, a.iters // 3), warmup=2)))
        fake = torch.rand_like(hr_img)

        def d_phase(D, penalty):
            D.zero_grad(set_to_none=False) if hasattr(D, 'zero_grad') else None
            loss = -D(hr_img).mean() + D(fake).mean()
            (loss + 11.0 * penalty(D)).backward()

        row['d_phase'] = fig(trials(lambda: d_phase(hd, lambda D: step.gradient_penalty(hr_img, fake, alpha)), a.trials, max(2, a.iters // 2), warmup=2))
        if not a.no_eager:
            ed = od.to(dev).to(memory_format=torch.channels_last)
            hr_cl, fake_cl = hr_img.contiguous(memory_format=torch.channels_last), fake.contiguous(memory_format=torch.channels_last)

            def eager_phase():
                ed.zero_grad(set_to_none=False)
                loss = -ed(hr_cl).mean() + ed(fake_cl).mean()
                interp = (alpha * hr_cl + (1 - alpha) * fake_cl).requires_grad_(True)
                d_out = ed(interp)
                grads = torch.autograd.grad(d_out, interp, torch.ones_like(d_out), create_graph=True)[0]
                (loss + 11.0 * (grads.norm(2, 1) - 1).pow(2).mean()).backward()

            row['d_phase_eager'] = fig(trials(eager_phase, a.trials, max(2, a.iters // 2), warmup=2))
        out[nt or 'none'] = row
        print(json.dumps({nt or 'none': row}), file=sys.stderr, flush=True)
        del step, hg, hd, hf
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--step-batch', type=int, default=16)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-steps', action='store_true')
    ap.add_argument('--no-eager', action='store_true')
    a = ap.parse_args()
    res = dict(tool='time_d_norms', device=torch.cuda.get_device_name(0), batch=a.batch, kernels=kernel_table(a.batch, a))
    if not a.no_steps:
        res['step_batch'] = a.step_batch
        res['steps'] = step_table(a.step_batch, a)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
