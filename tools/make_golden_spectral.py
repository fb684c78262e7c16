"""Generate tests/golden/disc_spectral.npz by running the REFERENCE model/base_networks.py Discriminator(..., use_spectralnorm=True, ...)
(build container only; the stub import of oracle/make_golden.py) with the filler, inputs and pass sequence of tests/spectral_ref.py at
(2, 3, 32, 32).

  1. keys, shapes and requires_grad flags of all 8 variants (norm_type '' | 'instance' | 'group' | 'batch' x attention);
  2. for ('', plain), ('', att), ('instance', plain), ('batch', plain): digests of D(img), of d img and of every trainable parameter's
     gradient for the cotangent det_fill('D.dy'); the reference's own SRADSGAN.gradient_penalty(..., 'L2', 'LS') under
     np.random.seed(123) and digests of its parameter gradients; u, v (strided entries) and sigma of every layer after passes 1-4;
  3. one training iteration at train_small's shapes with the '' + attention discriminator, relative False and True (the restatement
     gan_options_ref.train_step on the REFERENCE's modules): the six logged scalars, gradient digests of G and D, and weight_u /
     weight_v of every layer AFTER the step, i.e. after the clamp to +- clip_value that the reference applies to every D parameter.

Established on the CPU here and recorded:
  signal     as tools/make_golden_disc_norms.py: the conv factor (it reaches the plain last conv only: W = weight_bar / sigma does not
             see it) is chosen so that the per-sample L2 norm of the penalty's d D / d interpolate lies in [1, 10] -- the upper decade of
             that tool's [0.1, 10]: at its lower edge D's outputs are too small for the `passes` condition below
  stability  the restatement in fp64 against itself with the operands of every 3 x 3 conv's forward rounded to a split-bf16 pair: the
             first filler tag suffix in 0 .. 15 for which every recorded tensor agrees within HALF the bars of the GPU test is taken
  passes     mean D(fake) of the D phase differs from mean D(gen_hr) of the G phase by more than 10 x the scalar bar (a port that
             reuses a pass cannot meet the scalars), and the recorded post-step u after the step's 4 (relative: 5) power iterations
             differs from what one iteration fewer and one more would leave by more than 100 x the u bar (a port that miscounts the
             iterations cannot meet the recorded u)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402
from tests import disc_norms_ref as DR  # noqa: E402
from tests import gan_options_ref as GR  # noqa: E402
from tests import spectral_ref as SR  # noqa: E402
from tests.conv_emulation import split_bf16  # noqa: E402

BARS = dict(y=1e-3, dx=2e-3, grads=2e-3, gp=1e-4, gp_grads=5e-3)       # tests/test_spectral_gpu.py
SCALAR_BAR, UV_BAR, CLIP = 1e-3, 1e-5, 0.01
FLOOR = 1e-4


def rel(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), FLOOR)


def hilo(t):
    hi, lo = split_bf16(t.detach().float())
    return (hi + lo).to(t.dtype)


def straight_through(t):
    return t + (hilo(t) - t).detach()


def rounded_twin(d):
    """The restatement `d` (fp64) with split-bf16 operands in the forward of every 3 x 3 conv (values rounded, gradients straight through)."""
    for w in SR.wrappers(d):
        w.operand = straight_through
    last = d.model[len(d.model) - 1]
    with torch.no_grad():
        last.weight.copy_(hilo(last.weight))
    last.register_forward_pre_hook(lambda mod, args: (straight_through(args[0]),))
    return d


def power_iteration(w_bar, u, v):
    wm = w_bar.flatten(1)
    v = SR.l2normalize(wm.t() @ u)
    return SR.l2normalize(wm @ v), v


def main():
    torch.set_num_threads(8)
    ref = MG.import_reference()
    bn = importlib.import_module('model.base_networks')
    me = types.SimpleNamespace(gpu_mode=False)

    def ref_penalty(d, real, fake, alpha):
        np.random.seed(123)
        old = torch.get_default_dtype()
        torch.set_default_dtype(real.dtype)             # the reference builds alpha with torch.FloatTensor(...)
        try:
            if real.dtype == torch.float64:
                return SR.restated_penalty(d, real, fake, alpha)
            return ref.SRADSGAN.gradient_penalty(me, d, real, fake, 'L2', 'LS').detach()
        finally:
            torch.set_default_dtype(old)

    np.random.seed(123)
    alpha = torch.from_numpy(np.random.random((SR.IMG_SHAPE[0], 1, 1, 1)).astype(np.float32))
    out = {'alpha': alpha.numpy(), 'variants': np.array([SR.tag(*v) for v in SR.VARIANTS]), 'numbered': np.array([SR.tag(*v) for v in SR.NUMBERED])}
    for nt, att in SR.VARIANTS:
        name = SR.tag(nt, att)
        d = bn.Discriminator(norm_type=nt, use_spectralnorm=True, attention=att)
        sd = d.state_dict()
        flags = dict(d.named_parameters())
        out.update({name + '.keys': np.array(list(sd.keys())), name + '.shapes': np.array([','.join(map(str, v.shape)) for v in sd.values()]),
                    name + '.requires_grad': np.array([bool(flags[k].requires_grad) if k in flags else False for k in sd], dtype=np.bool_)})
    for nt, att in SR.NUMBERED:
        name, chosen = SR.tag(nt, att), None
        for suffix in range(16):
            t = SR.inputs(suffix)
            scale, norms = 1.0, None
            for _ in range(400):                         # signal: per-sample norm of d D / d interpolate into [1, 10] (see `passes`)
                d = SR.fill_(SR.Discriminator(norm_type=nt, attention=att), suffix, scale)
                x = (alpha * t['real'] + (1 - alpha) * t['fake']).requires_grad_(True)
                g = torch.autograd.grad(d(x).sum(), x)[0]
                norms = g.flatten(1).norm(dim=1)
                if float(norms.min()) >= 1.0 and float(norms.max()) <= 10:
                    break
                scale *= 1.1 if float(norms.min()) < 1.0 else 1 / 1.1
            else:
                raise SystemExit('%s: no conv scale gives a per-sample gradient norm in [1, 10] (last %s)' % (name, norms))
            fresh64 = lambda: SR.fill_(SR.Discriminator(norm_type=nt, attention=att), suffix, scale).double()      # noqa: E731
            a, b = SR.run(fresh64(), t, alpha.double(), ref_penalty), SR.run(rounded_twin(fresh64()), t, alpha.double(), ref_penalty)
            figs = dict(y=rel(b['y'], a['y']), dx=rel(b['dx'], a['dx']), gp=abs(b['gp'] - a['gp']),
                        grads=max(rel(b['grads'][k], a['grads'][k]) for k in a['grads']),
                        gp_grads=max(rel(b['gp_grads'][k], a['gp_grads'][k]) for k in a['gp_grads']))
            ok = all(figs[k] <= 0.5 * BARS[k] for k in BARS)
            print('%-14s suffix %2d scale %.4g norms %s  %s  %s' % (name, suffix, scale, [round(float(v), 4) for v in norms],
                                                                   ' '.join('%s %.2e' % kv for kv in figs.items()), 'ok' if ok else 'unstable'))
            if ok:
                chosen = (suffix, scale, norms, figs)
                break
        if chosen is None:
            raise SystemExit('%s: no stable filler tag among 16' % name)
        suffix, scale, norms, figs = chosen
        d = SR.fill_(bn.Discriminator(norm_type=nt, use_spectralnorm=True, attention=att), suffix, scale)
        r = SR.run(d, t, alpha, ref_penalty)             # the reference itself, fp32, its own penalty method
        out.update({name + '.suffix': np.int64(suffix), name + '.conv_scale': np.float64(scale), name + '.signal': norms.numpy(),
                    name + '.stability': np.array([figs[k] for k in BARS]), name + '.y': r['y'].numpy().ravel(), name + '.dx': MG.O.digest(r['dx']),
                    name + '.gp': np.float32(r['gp']), name + '.names': np.array(list(r['grads'].keys())),
                    name + '.grads': np.concatenate([DR.digest(v) for v in r['grads'].values()]),
                    name + '.gp_grads': np.concatenate([DR.digest(v) for v in r['gp_grads'].values()])})
        for i, (u, v, s) in enumerate(r['states'], start=1):
            out['%s.u%d' % (name, i)], out['%s.v%d' % (name, i)], out['%s.sigma%d' % (name, i)] = u, v, s
        print('%-14s sigma after pass 1 %s ... pass 4 %s' % (name, np.array2string(r['states'][0][2], precision=4),
                                                             np.array2string(r['states'][3][2], precision=4)))
    # ---- one training iteration (sradsgan.py:829-892) per case, '' + attention: gan_options_ref.train_step on the REFERENCE's modules
    small = np.load(os.path.join(ROOT, 'tests', 'golden', 'train_small.npz'))
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    out['train_alpha'] = small['alpha0']
    sh = GR.TRAIN_SHAPE
    name = SR.tag('', True)
    for case, opts in SR.TRAIN_CASES.items():
        G = MG.O.det_init_(ref.GeneratorResNet(ref.ResGroup, n_residual_blocks=sh['n_groups'], n_basic_blocks=sh['n_blocks'],
                                               upscale_factor=sh['scale']), prefix='G.')
        Fx = MG.O.det_init_(MG.vgg_standin(), prefix='F.')
        D = SR.fill_(bn.Discriminator(norm_type='', use_spectralnorm=True, attention=True), int(out[name + '.suffix']), float(out[name + '.conv_scale']))
        w_bars = [w.module.weight_bar.detach().clone() for w in SR.wrappers(D)]
        passes = []                                      # per D pass: (mean of the output, [(u, v) of every layer])
        D.register_forward_hook(lambda mod, args, y: passes.append(
            (float(y.detach().mean()), [(w.module.weight_u.detach().clone(), w.module.weight_v.detach().clone()) for w in SR.wrappers(mod)])))
        sc = GR.train_step(G, D, Fx, torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999)),
                           torch.optim.Adam([p for p in D.parameters()], lr=2e-4, betas=(0.9, 0.999)), lr_img, hr_img,
                           torch.from_numpy(small['alpha0']), clip_value=CLIP, **opts)
        key = '%s.it_%s' % (name, case)
        npass = 5 if opts['relative'] else 4
        assert len(passes) == npass, len(passes)
        out[key + '_scalars'] = np.array([sc[k] for k in GR.SCALARS], dtype=np.float64)
        for net_tag, net in (('G', G), ('D', D)):
            names, samples, counts, maxabs = GR.grad_digest(net)
            out['%s_%s_names' % (key, net_tag)], out['%s_%s_grads' % (key, net_tag)] = names, samples
            out['%s_%s_counts' % (key, net_tag)], out['%s_%s_maxabs' % (key, net_tag)] = counts, maxabs
        out[key + '_u'], out[key + '_v'] = SR.clamp_uv(D, CLIP)
        # passes: D(gen_hr) is the first pass, D(fake) the one before the last (the last is D(interp))
        gap = abs(passes[npass - 2][0] - passes[0][0])
        assert gap > 10 * SCALAR_BAR, (case, gap)
        # iterations: what one power iteration fewer / one more (with the step's weight_bar) would leave after the clamp
        dig = lambda ts: np.concatenate([SR.uv_digest(t.clamp(-CLIP, CLIP)) for t in ts])      # noqa: E731
        fewer = dig([u for u, _ in passes[npass - 2][1]])
        more = dig([power_iteration(w, u, v)[0] for w, (u, v) in zip(w_bars, passes[npass - 1][1])])
        d_fewer, d_more = float(np.abs(out[key + '_u'] - fewer).max()), float(np.abs(out[key + '_u'] - more).max())
        assert d_fewer > 100 * UV_BAR and d_more > 100 * UV_BAR, (case, d_fewer, d_more)
        out[key + '_conditions'] = np.array([gap, d_fewer, d_more])
        assert all(p.grad is None for k, p in D.named_parameters() if k.endswith(('weight_u', 'weight_v')))
        print('%-14s %-9s scalars %s  pass means %s  |D(fake) - D(gen)| %.3e  post-step u vs one fewer %.3e, one more %.3e'
              % (name, case, np.array2string(out[key + '_scalars'], precision=6), [round(p[0], 5) for p in passes], gap, d_fewer, d_more))
    path = os.path.join(ROOT, 'tests', 'golden', 'disc_spectral.npz')
    np.savez_compressed(path, **out)
    print('%s: %.1f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
