"""Generate tests/golden/gan_options.npz (build container only; the stub import of oracle/make_golden.py, as tools/make_golden_drcan.py).

1. The REFERENCE's SRADSGAN.gradient_penalty (sradsgan.py:595-641, np.random alpha under a fixed seed) for the five non-default
   (grad_penalty_Lp_norm, penalty_type) pairs, on the inputs of gradient_penalty.npz and a discriminator whose conv weights come from
   the deterministic filler with GP_GAIN times the std (tests/gan_options_ref.scaled_discriminator_init_): with clip-sized weights the
   per-pixel norms are ~0.2 and hinge is identically zero.  Per norm kind the share of pixels above 1, the share within 1e-3 of 1, the
   share of Linf near-ties and the smallest margin are asserted (gan_options_ref.shares_ok) and stored.
2. One training iteration at train_small's shapes and depth for the four cases of gan_options_ref.CASES, run by the restatement
   gan_options_ref.train_step on the reference's modules (the reference's train() is one monolithic loop) -- after asserting that the
   restatement with default options reproduces train_small.npz.  The cases use the scaled discriminator (TRAIN_GAIN, clip_value GP_CLIP).  Stored
   per case: the six logged scalars and mean(D(real)), the penalty, digests of G's and D's gradients, D's BatchNorm buffers after the
   step, and the shares of the interpolate's gradient for the case's norm kind."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from oracle import sradsgan_ref as O  # noqa: E402
from tests import gan_options_ref as GR  # noqa: E402

GP_KEYS = ['model.0.weight', 'model.3.weight', 'model.3.bias', 'model.11.weight', 'model.17.fc2.weight', 'model.18.conv1.weight',
           'model.25.weight']


class _Self:
    gpu_mode = False


def build(R, MG, scaled):
    s = GR.TRAIN_SHAPE
    G = R.GeneratorResNet(R.ResGroup, n_residual_blocks=s['n_groups'], n_basic_blocks=s['n_blocks'], upscale_factor=s['scale'])
    D, Fx = R.Discriminator(), MG.vgg_standin()
    O.det_init_(G, prefix='G.'), O.det_init_(Fx, prefix='F.')
    GR.scaled_discriminator_init_(D, gain=GR.TRAIN_GAIN) if scaled else O.det_init_(D, prefix='D.')
    return G, D, Fx


def adams(G, D):
    return (torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999)), torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.999)))


def main():
    torch.set_num_threads(8)
    argv, sys.argv = sys.argv, sys.argv[:1]
    import make_golden as MG
    sys.argv = argv
    R = MG.import_reference()
    out = {'gain': np.float64(GR.GP_GAIN), 'train_gain': np.float64(GR.TRAIN_GAIN), 'clip': np.float64(GR.GP_CLIP), 'band': np.float64(GR.BAND), 'band_cap': np.float64(GR.BAND_CAP)}

    # ---- 1. the penalty through the reference's own method ----------------------------------------------------------------
    real = O.det_fill('gp.real', (2, 3, 32, 32), 0.5, 0.5)
    fake = O.det_fill('gp.fake', (2, 3, 32, 32), 0.5, 0.5)
    np.random.seed(123)
    alpha = np.random.random((2, 1, 1, 1))
    out['gp_alpha'] = alpha.astype(np.float32)
    d = GR.scaled_discriminator_init_(R.Discriminator())
    grads = GR.input_gradient(d, real, fake, torch.from_numpy(alpha).float())
    for norm in GR.NORMS:
        sh = GR.pixel_norm_shares(grads, norm)
        print('penalty golden, %-4s: share above 1 %.4f, within %.0e of 1 %.4f, Linf near-ties %.4f, smallest margin %.2e' % ((norm,) + sh[:1] + (GR.BAND,) + sh[1:]))
        assert GR.shares_ok(*sh[:3]), (norm, sh)
        out['gp_shares_' + norm] = np.array(sh, dtype=np.float64)
    for norm, pen in GR.NON_DEFAULT_PAIRS:
        d = GR.scaled_discriminator_init_(R.Discriminator())
        np.random.seed(123)
        gp = R.SRADSGAN.gradient_penalty(_Self(), d, real, fake, norm, pen)
        sd = dict(d.named_parameters())
        tag = 'gp_%s_%s' % (norm, pen)
        out[tag] = np.float64(gp.item())
        for k in GP_KEYS:
            out[tag + '__grad__' + k.replace('.', '__')] = O.digest(sd[k].grad)
        print('%-14s gp %.6f' % (tag, gp.item()))

    # ---- 2. training iterations by the restatement -------------------------------------------------------------------------
    small = np.load(os.path.join(ROOT, 'tests', 'golden', 'train_small.npz'))
    G, D, Fx = build(R, MG, scaled=False)
    oG, oD = adams(G, D)
    for it in range(2):
        lr_img, hr_img = GR.case_inputs('train_small', it)
        s = GR.train_step(G, D, Fx, oG, oD, lr_img, hr_img, torch.from_numpy(small['alpha%d' % it]))
        got = np.array([s[k] for k in GR.SCALARS])
        np.testing.assert_allclose(got, small['scalars%d' % it], rtol=2e-4, atol=2e-5, err_msg='default options, it %d' % it)
        if it == 0:
            for k in ['model.0.weight', 'model.25.weight']:
                want = small['it0_D_grad__' + k.replace('.', '__')]
                np.testing.assert_allclose(O.digest(dict(D.named_parameters())[k].grad), want, rtol=1e-3, atol=1e-3 * np.abs(want).max())
    print('default options reproduce train_small.npz')

    lr_img, hr_img = GR.case_inputs('train_small', 0)
    alpha = torch.from_numpy(small['alpha0'])
    out['train_alpha'] = small['alpha0']
    for name, opts in GR.CASES.items():
        G, D, Fx = build(R, MG, scaled=True)
        with torch.no_grad():
            gen = G(lr_img)
        norm = opts.get('grad_penalty_Lp_norm', 'L2')
        sh = GR.pixel_norm_shares(GR.input_gradient(copy.deepcopy(D), hr_img, gen, alpha), norm)
        assert GR.shares_ok(*sh[:3]), (name, norm, sh)
        oG, oD = adams(G, D)
        s = GR.train_step(G, D, Fx, oG, oD, lr_img, hr_img, alpha, clip_value=GR.GP_CLIP, **opts)
        out[name + '__scalars'] = np.array([s[k] for k in GR.SCALARS] + [s['d_real_mean']], dtype=np.float64)
        out[name + '__shares'] = np.array(sh, dtype=np.float64)
        for tag, net in (('G', G), ('D', D)):
            names, samples, counts, maxabs = GR.grad_digest(net)
            out['%s__%s_names' % (name, tag)], out['%s__%s_grads' % (name, tag)] = names, samples
            out['%s__%s_counts' % (name, tag)], out['%s__%s_maxabs' % (name, tag)] = counts, maxabs
        names, vals, nbt = GR.bn_buffers(D)
        out[name + '__bn_names'], out[name + '__bn'], out[name + '__nbt'] = names, vals, nbt
        print('%-11s %s  shares(%s) %s  nbt %s' % (name, np.array2string(out[name + '__scalars'], precision=6), norm,
                                                   np.array2string(np.array(sh), precision=4), nbt[:1]))
    path = os.path.join(ROOT, 'tests', 'golden', 'gan_options.npz')
    np.savez_compressed(path, **out)
    print('gan_options.npz %.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
