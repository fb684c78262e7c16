"""DSSR without a GPU: the CPU restatement (tests/dssr_ref.py) against vectors recorded from the reference's model/dssr.py
(tools/make_golden_dssr.py), and the HIP model's parameter layout against the reference's."""
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import dssr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [2, 3, 4, 8, 9]
LR = 1e-4


def golden(scale):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'dssr_x%d.npz' % scale))


def build_ref(scale, dtype=torch.float32):
    net = R.Generator(groups=2, blocks=2, scale=scale)
    O.det_init_(net, prefix='D.')
    return net.to(dtype)


def inputs(scale):
    x = O.det_fill('dssr.x.%d' % scale, (2, 3, 12, 10), 0.5, 0.5)
    t = O.det_fill('dssr.t.%d' % scale, (2, 3, 12 * scale, 10 * scale), 0.5, 0.5)
    return x, t


def gkey(prefix, k):
    return prefix + k.replace('.', '__')


@pytest.mark.parametrize('scale', SCALES)
def test_restatement_matches_reference_vectors(scale):
    g = golden(scale)
    net = build_ref(scale)
    assert sorted(net.state_dict().keys()) == list(g['keys'])
    x, t = inputs(scale)
    y = net(x)
    l1 = torch.nn.functional.l1_loss(y, t)
    mse = torch.nn.functional.mse_loss(y, t)
    assert np.abs(y.detach().numpy() - g['y']).max() < 2e-6
    l1v, msev = float(l1.detach()), float(mse.detach())
    assert abs(l1v - float(g['loss_l1'])) < 1e-6 and abs(msev - float(g['loss_mse'])) < 1e-6
    l1.backward()
    params = R.unique_params(net)
    assert len(params) == sum(1 for k in g.files if k.startswith('grad__'))
    for k, p in params:
        ref = g[gkey('grad__', k)]
        assert np.abs(O.digest(p.grad) - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k


@pytest.mark.parametrize('norm', ['L1', 'L2'])
@pytest.mark.parametrize('scale', [2, 3, 4])
def test_restatement_two_adam_steps_match_reference(scale, norm):
    g = golden(scale)
    net = build_ref(scale)
    x, t = inputs(scale)
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999))
    crit = torch.nn.L1Loss() if norm == 'L1' else torch.nn.MSELoss()
    for it in range(2):
        opt.zero_grad()
        loss = crit(net(x), t)
        loss.backward()
        opt.step()
        assert abs(float(loss) - float(g['steps_' + norm][it])) < (2e-6 if it == 0 else 5e-6), (it, float(loss))
        for k, p in R.unique_params(net):
            ref = g['step%d_%s__%s' % (it, norm, k.replace('.', '__'))]
            d = np.abs(R.step_digest(p.detach()) - ref)
            # Adam turns a gradient whose sign is roundoff into a full +-lr step: each element may be off by 2 lr per step taken
            assert d[:-2].max() <= 2 * LR * (it + 1) + 1e-6, (it, k)
            if len(ref) > 512:
                assert d[-2] <= 2 * LR * (it + 1) * p.numel() and d[-1] <= 2 * LR * (it + 1) * np.sqrt(p.numel()) + 1e-5, (it, k)


@pytest.mark.parametrize('scale', SCALES)
def test_hip_model_state_dict_keys_match_reference(scale):
    from sradsgan_amd.model import dssr as H
    g = golden(scale)
    net = H.GeneratorResNet(H.ResGroup, n_residual_blocks=2, n_basic_blocks=2, upscale_factor=scale)   # built on the CPU
    assert sorted(net.state_dict().keys()) == list(g['keys'])
    ref = build_ref(scale)
    net.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(net.state_dict(), strict=True)
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters())
    assert net.UP.is_affine()


def test_hip_model_default_config_parameter_count():
    from sradsgan_amd.model import dssr as H
    net = H.GeneratorResNet(H.ResGroup, n_residual_blocks=3, n_basic_blocks=10, upscale_factor=4)
    assert sum(p.numel() for p in net.parameters()) == 9134339          # the reference's default x4 generator
    assert sum(p.numel() for p in R.Generator(3, 10, 4).parameters()) == 9134339


def test_hip_model_refuses_the_cpu():
    from sradsgan_amd.model import dssr as H
    net = H.GeneratorResNet(H.ResGroup, n_residual_blocks=1, n_basic_blocks=1, upscale_factor=2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(1, 3, 8, 8))
