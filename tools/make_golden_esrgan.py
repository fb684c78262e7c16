"""Generate tests/golden/esrgan_*.npz by running the REFERENCE model/architecture.py and model/block.py (RRDBNet, Discriminator_VGG_96 /
128 / 192 / 256) and the reference's GANLoss (model/sradsgan.py:35-67) -- build container only; the stub import of
oracle/make_golden.py supplies the absent torchvision.  VGGFeatureExtractor cannot be constructed there (it asks torchvision for a
pretrained file), so its structure comes from tests/esrgan_ref.py, filled by the deterministic filler, like
oracle.sradsgan_ref.FeatureExtractor.  Parameters come from the filler keyed by state_dict name, inputs from det_fill.

  esrgan_keys.npz   the sorted key lists of RRDBNet(nb = 2) for x2, x3, x4, x8 and of the four discriminators
  esrgan_gen.npz    RRDBNet(nb = 2) at LR (2, 3, 12, 10) for the four scales: the output and the gradients of a fixed linear functional
                    of it, as digests; RRDBNet(nb = 23, x4) at (1, 3, 8, 8): the output
  esrgan_disc.npz   each discriminator at B = 2: output, digest of the input gradient of sum(output), BatchNorm buffers after the call
  esrgan_step.npz   two iterations of sradsgan.py:829-892 (gp off) composed from the reference's classes with torch.optim.Adam
                    (lr 2e-6): RRDBNet(nb = 2), Discriminator_VGG_96, GANLoss, x4, LR 24 x 24, B = 2, L1, weights 1e-2 / 1 / 5e-3,
                    for {vanilla, lsgan} x {relativistic, plain}: the five scalars before each step, digests of the weights and of the
                    BatchNorm buffers after it."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle.make_golden import import_reference  # noqa: E402
from tests import esrgan_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')


def k_(k):
    return k.replace('.', '__')


def save(name, arrays):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('%s: %d arrays, %.1f KB' % (name, len(arrays), os.path.getsize(path) / 1024.0))


def main():
    torch.set_num_threads(8)
    sr = import_reference()
    arch = importlib.import_module('model.architecture')
    d_cls = {s: getattr(arch, 'Discriminator_VGG_%d' % s) for s in R.D_SIZES}

    keys, gen = {}, {}
    for scale in R.SCALES:
        G = R.fill_generator(arch.RRDBNet(3, 3, 64, 2, upscale=scale))
        keys['g_x%d' % scale] = np.array(sorted(G.state_dict().keys()))
        x = R.gen_input(scale)
        y = G(x)
        (y * R.gen_functional(scale)).sum().backward()
        gen['y_x%d' % scale] = R.out_digest(y)
        gen['grads_x%d' % scale] = np.concatenate([R.small_digest(p.grad) for _, p in G.named_parameters()])
    G = R.fill_generator(arch.RRDBNet(3, 3, 64, 23, upscale=4), tag='23')
    from oracle import sradsgan_ref as O
    with torch.no_grad():
        gen['y_deep'] = R.out_digest(G(O.det_fill('esrgan.deep.x', R.DEEP_SHAPE, 0.5, 0.5)))
    assert sum(p.numel() for p in G.parameters()) == 16697987

    disc = {}
    for size in R.D_SIZES:
        D = R.fill_discriminator(d_cls[size](3, 64), size)
        keys['d_%d' % size] = np.array(sorted(D.state_dict().keys()))
        x = R.d_input(size).requires_grad_()
        out = D(x)
        out.sum().backward()
        disc['out_%d' % size] = out.detach().numpy()
        disc['dx_%d' % size] = R.out_digest(x.grad)
        for k, b in R.bn_buffers(D):
            disc['buf_%d__%s' % (size, k_(k))] = b.numpy()
    save('esrgan_keys', keys)
    save('esrgan_gen', gen)
    save('esrgan_disc', disc)

    step = {}
    lr_img, hr_img = R.step_inputs()
    l1 = torch.nn.L1Loss()
    w = R.WEIGHTS
    for gan_type, relative in R.STEP_CASES:
        tag = '%s_%s' % (gan_type, 'rel' if relative else 'plain')
        G = R.fill_generator(arch.RRDBNet(3, 3, 64, 2, upscale=R.STEP_SCALE))
        D = R.fill_discriminator(d_cls[R.STEP_D](3, 64), R.STEP_D)
        Fx = R.fill_extractor(R.Vgg())
        crit = sr.GANLoss(gan_type)
        opt_G = torch.optim.Adam(G.parameters(), lr=R.ADAM_LR, betas=(0.9, 0.999))
        opt_D = torch.optim.Adam(D.parameters(), lr=R.ADAM_LR, betas=(0.9, 0.999))
        rows = []
        for it in range(2):
            opt_G.zero_grad()
            gen_hr = G(lr_img)
            pixel = l1(gen_hr, hr_img)
            content = l1(Fx(gen_hr), Fx(hr_img).detach())
            if relative:
                pred_g_fake = D(gen_hr)
                pred_d_real = D(hr_img).detach()
                loss_gan = (crit(pred_d_real - torch.mean(pred_g_fake), False) + crit(pred_g_fake - torch.mean(pred_d_real), True)) / 2
            else:
                loss_gan = crit(D(gen_hr), True)
            loss_G = w['weight_pixel'] * pixel + w['weight_content'] * content + w['weight_gan'] * loss_gan
            loss_G.backward()
            opt_G.step()
            opt_D.zero_grad()
            if relative:
                pred_d_real = D(hr_img)
                pred_d_fake = D(gen_hr.detach())
                loss_D = (crit(pred_d_real - torch.mean(pred_d_fake), True) + crit(pred_d_fake - torch.mean(pred_d_real), False)) / 2
            else:
                loss_D = crit(D(hr_img), True) + crit(D(gen_hr.detach()), False)
            loss_D.backward()
            opt_D.step()
            rows.append([loss_G.item(), loss_D.item(), pixel.item(), content.item(), loss_gan.item()])
            for net, name in ((G, 'G'), (D, 'D')):
                step['%s_step%d_%s' % (tag, it, name)] = np.concatenate([R.small_digest(p.detach()) for _, p in net.named_parameters()])
            step['%s_step%d_Dbuf' % (tag, it)] = np.concatenate([R.small_digest(b) for _, b in R.bn_buffers(D)])
        step[tag] = np.array(rows, dtype=np.float64)
        print(tag, rows)
    save('esrgan_step', step)


if __name__ == '__main__':
    main()
