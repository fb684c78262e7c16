"""Generate tests/golden/disc_norms.npz by running the REFERENCE model/base_networks.py Discriminator (build container only; the
stub import of oracle/make_golden.py) for norm_type in ('', 'instance', 'group') x attention in (False, True), with the filler and
inputs of tests/disc_norms_ref.py at (2, 3, 32, 32).

Per variant: the state_dict keys (in order) and shapes; digests of D(img), of d img and of every parameter gradient for the
cotangent det_fill('D.dy'); the value of the reference's own SRADSGAN.gradient_penalty(..., 'L2', 'LS') under np.random.seed(123),
its alpha, and digests of the penalty's parameter gradients.  Per norm_type, with the attention pair: one training iteration at
train_small's shapes (the six logged scalars, digests of G's and D's gradients), as gan_options.npz records its cases.

Two properties of the inputs are established on the CPU here and recorded:
  signal     the 3 x 3 conv weights are multiplied by a factor (stored) chosen so that the per-sample L2 norm of the penalty's
             d D / d interpolate lies in [0.1, 10] (the plain filler gives the norm-free D 3e-5 and gp = 0.99994: a test of nothing)
  stability  the reference in fp64 against itself in fp64 with the operands of the 3 x 3 convs' forward rounded to a split-bf16
             pair (tests/conv_emulation.split_bf16, hi + lo): the first filler tag suffix in 0 .. 15 for which every recorded tensor
             agrees within HALF the bars of tests/test_disc_norms_gpu.py is taken (a LeakyReLU or max-pool input on its kink decides)."""
import copy
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
from tests.conv_emulation import split_bf16  # noqa: E402

BARS = dict(y=1e-3, dx=2e-3, grads=2e-3, gp=1e-4, gp_grads=5e-3)       # tests/test_disc_norms_gpu.py
FLOOR = 1e-4


def rel(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), FLOOR)


def hilo(t):
    hi, lo = split_bf16(t.detach().float())
    return (hi + lo).to(t.dtype)


def rounded_twin(d64):
    """fp64 copy whose 3 x 3 convs see split-bf16 operands in the forward (values rounded, gradients straight through)."""
    d = copy.deepcopy(d64)
    for m in d.modules():
        if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3):
            with torch.no_grad():
                m.weight.copy_(hilo(m.weight))
            m.register_forward_pre_hook(lambda mod, args: (args[0] + (hilo(args[0]) - args[0]).detach(),))
    return d


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
                return DR.restated_penalty(d, real, fake, alpha)
            return ref.SRADSGAN.gradient_penalty(me, d, real, fake, 'L2', 'LS').detach()
        finally:
            torch.set_default_dtype(old)

    np.random.seed(123)
    alpha = torch.from_numpy(np.random.random((DR.IMG_SHAPE[0], 1, 1, 1)).astype(np.float32))
    out = {'alpha': alpha.numpy(), 'variants': np.array([DR.tag(*v) for v in DR.VARIANTS])}
    for nt, att in DR.VARIANTS:
        name, chosen = DR.tag(nt, att), None
        for suffix in range(16):
            t = DR.inputs(suffix)
            scale, norms = 1.0, None
            for _ in range(400):                         # signal: per-sample norm of d D / d interpolate into [0.1, 10]
                d = DR.fill_(bn.Discriminator(norm_type=nt, attention=att), suffix, scale)
                x = (alpha * t['real'] + (1 - alpha) * t['fake']).requires_grad_(True)
                g = torch.autograd.grad(d(x).sum(), x)[0]
                norms = g.flatten(1).norm(dim=1)
                if float(norms.min()) >= 0.1 and float(norms.max()) <= 10:
                    break
                scale *= 1.1 if float(norms.min()) < 0.1 else 1 / 1.1
            else:
                raise SystemExit('%s: no conv scale gives a per-sample gradient norm in [0.1, 10] (last %s)' % (name, norms))
            d64 = copy.deepcopy(d).double()
            a, b = DR.run(d64, t, alpha.double(), ref_penalty), DR.run(rounded_twin(d64), t, alpha.double(), ref_penalty)
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
        r = DR.run(d, t, alpha, ref_penalty)             # the reference itself, fp32, its own penalty method
        sd = d.state_dict()
        out.update({name + '.keys': np.array(list(sd.keys())), name + '.shapes': np.array([','.join(map(str, v.shape)) for v in sd.values()]),
                    name + '.suffix': np.int64(suffix), name + '.conv_scale': np.float64(scale), name + '.signal': norms.numpy(),
                    name + '.stability': np.array([figs[k] for k in BARS]), name + '.y': r['y'].numpy().ravel(), name + '.dx': MG.O.digest(r['dx']),
                    name + '.gp': np.float32(r['gp']), name + '.names': np.array(list(r['grads'].keys())),
                    name + '.grads': np.concatenate([DR.digest(v) for v in r['grads'].values()]),
                    name + '.gp_grads': np.concatenate([DR.digest(v) for v in r['gp_grads'].values()])})
    # ---- one training iteration per variant (sradsgan.py:829-892), as tools/make_golden_gan_options.py records its cases: the
    # restatement gan_options_ref.train_step (which that tool holds to train_small.npz) on the REFERENCE's modules -- its generator
    # at train_small's configuration, base_networks.Discriminator(norm_type, attention=True) with the variant's filler, the VGG stand-in
    small = np.load(os.path.join(ROOT, 'tests', 'golden', 'train_small.npz'))
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    out['train_alpha'] = small['alpha0']
    sh = GR.TRAIN_SHAPE
    for nt in DR.NORM_TYPES:
        name = DR.tag(nt, True)
        G = MG.O.det_init_(ref.GeneratorResNet(ref.ResGroup, n_residual_blocks=sh['n_groups'], n_basic_blocks=sh['n_blocks'],
                                               upscale_factor=sh['scale']), prefix='G.')
        Fx = MG.O.det_init_(MG.vgg_standin(), prefix='F.')
        D = DR.fill_(bn.Discriminator(norm_type=nt, attention=True), int(out[name + '.suffix']), float(out[name + '.conv_scale']))
        sc = GR.train_step(G, D, Fx, torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999)),
                           torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.999)), lr_img, hr_img, torch.from_numpy(small['alpha0']))
        out[name + '.it_scalars'] = np.array([sc[k] for k in GR.SCALARS], dtype=np.float64)
        for tag, net in (('G', G), ('D', D)):
            names, samples, counts, maxabs = GR.grad_digest(net)
            out['%s.it_%s_names' % (name, tag)], out['%s.it_%s_grads' % (name, tag)] = names, samples
            out['%s.it_%s_counts' % (name, tag)], out['%s.it_%s_maxabs' % (name, tag)] = counts, maxabs
        print('%-14s iteration %s' % (name, np.array2string(out[name + '.it_scalars'], precision=6)))
    path = os.path.join(ROOT, 'tests', 'golden', 'disc_norms.npz')
    np.savez_compressed(path, **out)
    print('%s: %.1f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
