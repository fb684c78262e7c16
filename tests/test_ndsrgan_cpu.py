"""NDSRGAN without a GPU: the CPU restatement (tests/ndsrgan_ref.py) against vectors recorded from the reference's model/ndsrgan.py
(tools/make_golden_ndsrgan.py), and the HIP model's parameter layout against the reference's."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O
from tests import ndsrgan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [2, 3, 4, 8, 9]
SHAPE, DSHAPE = (2, 3, 16, 14), (2, 3, 40, 40)
LR = 2e-4


def golden(scale):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'ndsrgan_x%d.npz' % scale))


def build_ref(scale, dtype=torch.float32):
    G, D, Fx = R.Generator(scale), R.Discriminator(), O.FeatureExtractor()
    O.det_init_(G, prefix='N.')
    O.det_init_(D, prefix='ND.')
    O.det_init_(Fx, prefix='NF.')
    return G.to(dtype), D.to(dtype), Fx.to(dtype)


def inputs(scale):
    x = O.det_fill('ndsrgan.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('ndsrgan.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
    return x, t


def loss_terms(G, D, Fx, x, t):
    y = G(x)
    v = D(y)
    pixel = F.smooth_l1_loss(y, t)
    content = F.smooth_l1_loss(Fx(y), Fx(t).detach())
    gan = F.smooth_l1_loss(v, torch.ones_like(v))
    return y, pixel, content, gan


@pytest.mark.parametrize('scale', SCALES)
def test_restatement_matches_reference_vectors(scale):
    g = golden(scale)
    G, D, Fx = build_ref(scale)
    assert sorted(G.state_dict().keys()) == list(g['keys'])
    assert sorted(D.state_dict().keys()) == list(g['dkeys'])
    x, t = inputs(scale)
    y, pixel, content, gan = loss_terms(G, D, Fx, x, t)
    assert np.abs(R.out_digest(y) - g['y']).max() < 2e-5
    for name, v in (('pixel', pixel), ('content', content), ('gan', gan)):
        assert abs(float(v) - float(g[name])) < 2e-6, name
    (1e-2 * pixel + content + 2.5e-3 * gan).backward()
    dig = np.concatenate([R.grad_digest(p.grad) for _, p in R.unique_params(G)])
    ref = g['grads']
    assert dig.shape == ref.shape
    assert np.abs(dig - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_restatement_discriminator_and_running_stats_match_reference():
    g = golden(2)
    _, D, _ = build_ref(2)
    out = D(O.det_fill('ndsrgan.d', DSHAPE, 0.5, 0.5))
    assert out.shape == (2, 1, 3, 3)                   # 40 / 8 - 2
    assert np.abs(out.detach().numpy() - g['d_x_out']).max() < 2e-5
    for k, b in D.state_dict().items():
        if 'running' in k:
            assert np.abs(b.numpy() - g['d_buf__' + k.replace('.', '__')]).max() < 1e-5, k


def test_restatement_two_adam_steps_match_reference():
    g = golden(2)
    G, D, Fx = build_ref(2)
    x, t = inputs(2)
    opt_G = torch.optim.Adam(G.parameters(), lr=LR, betas=(0.9, 0.99))
    opt_D = torch.optim.Adam(D.parameters(), lr=LR, betas=(0.9, 0.99))
    for it in range(2):
        lg, ld = R.train_iteration(G, D, Fx, opt_G, opt_D, x, t)
        assert abs(lg - float(g['steps'][it][0])) < 1e-5 and abs(ld - float(g['steps'][it][1])) < 1e-5, (it, lg, ld)
        for net, tag in ((G, 'G'), (D, 'D')):
            d = np.abs(np.concatenate([R.step_digest(p.detach()) for _, p in R.unique_params(net)]) - g['step%d_%s' % (it, tag)])
            # sampled elements: Adam turns a roundoff-signed gradient into a full lr step; sums / norms: a few such elements each
            assert np.median(d) <= 1e-6 and d.max() <= 2 * LR * (it + 1) * 64, (it, tag, d.max())
        bufs = np.concatenate([R.step_digest(b) for k, b in sorted(D.state_dict().items()) if 'running' in k])
        assert np.abs(bufs - g['step%d_Dbuf' % it]).max() < 1e-4


@pytest.mark.parametrize('scale', SCALES)
def test_hip_model_state_dict_keys_match_reference(scale):
    from sradsgan_amd.model import ndsrgan as H
    g = golden(scale)
    G = H.GeneratorResNet(in_channels=3, out_channels=3, nf=64, nc=32, upscale_factor=scale)    # built on the CPU
    assert sorted(G.state_dict().keys()) == list(g['keys'])
    assert len(G.state_dict()) == {2: 746, 3: 746, 4: 748, 8: 750, 9: 748}[scale]
    ref, D, _ = build_ref(scale)
    G.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(G.state_dict(), strict=True)
    hd = H.Discriminator()
    assert sorted(hd.state_dict().keys()) == list(g['dkeys'])
    hd.load_state_dict(D.state_dict(), strict=True)
    if scale in (4, 8, 9):                             # one conv shared by every upsampling stage
        assert G.upsampling[1].weight is G.upsampling[4].weight


def test_hip_model_parameter_counts():
    from sradsgan_amd.model import ndsrgan as H
    assert sum(p.numel() for p in H.GeneratorResNet(upscale_factor=4).parameters()) == 17510403
    assert sum(p.numel() for p in R.Generator(4).parameters()) == 17510403
    assert sum(p.numel() for p in H.Discriminator().parameters()) == 2766529
    assert sum(p.numel() for p in R.Discriminator().parameters()) == 2766529


def test_hip_model_refuses_other_widths_and_the_cpu():
    from sradsgan_amd.model import ndsrgan as H
    with pytest.raises(NotImplementedError):
        H.GeneratorResNet(nf=32)
    with pytest.raises(NotImplementedError):
        H.DenseBlock(64, 16)
    G = H.GeneratorResNet(upscale_factor=2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        H.Discriminator()(torch.zeros(1, 3, 32, 32))
