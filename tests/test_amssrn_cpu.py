"""AMSSRN on the host: the fp64 restatement (tests/amssrn_ref.py) against the reference's vectors (tests/golden/amssrn_x*.npz, made
by tools/make_golden_amssrn.py from the reference's GeneratorResNet), and the HIP model's state_dict keys and shapes, including the
tied x9 upsampler.  No GPU call is made here."""
import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import amssrn_ref as R

SCALES = (2, 3, 4, 8, 9)
SHAPE = (2, 3, 13, 14)
SLOPES = {'body.0.c1.rb.1.weight': -0.3, 'body.1.c2.rb.1.weight': 0.0, 'body.4.ca.conv_du.1.weight': -0.2,
          'body.5.aspp.act.weight': 0.1}


def golden(scale):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'amssrn_x%d.npz' % scale))


def init_(G):
    O.det_init_(G, prefix='A.')
    params = dict(G.named_parameters())
    with torch.no_grad():
        for k, v in SLOPES.items():
            params[k].fill_(v)
    return G


def inputs(scale):
    x = O.det_fill('amssrn.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('amssrn.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
    return x, t


def unique_params(net):
    seen, out = set(), []
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append((k, p))
    return out


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize('scale', SCALES)
def test_restatement_matches_reference_vectors(scale):
    g = golden(scale)
    G = init_(R.Generator(scale)).double()
    x, t = inputs(scale)
    y = G(x.double())
    l1 = R.loss(y, t.double())
    assert rel(O.digest(y, full_max=4096, nsample=4096), g['y']) < 1e-5
    assert abs(l1.item() - float(g['l1'])) < 1e-6 and abs(R.loss(y, t.double(), 'MSE').item() - float(g['mse'])) < 1e-6
    l1.backward()
    ups = unique_params(G)
    assert [k for k, _ in ups] == list(g['names'])
    got = np.concatenate([digest(p.grad) for _, p in ups])
    assert rel(got, g['grads']) < 1e-4


def test_restatement_two_adam_steps_match_reference():
    g = golden(2)
    G = init_(R.Generator(2)).double()
    x, t = inputs(2)
    opt = torch.optim.Adam(G.parameters(), lr=1e-4, betas=(0.9, 0.999))
    for it in range(2):
        opt.zero_grad()
        lg = R.loss(G(x.double()), t.double())
        lg.backward()
        opt.step()
        assert abs(lg.item() - float(g['steps'][it])) < 1e-6
        assert rel(np.concatenate([digest(p.detach()) for _, p in unique_params(G)]), g['step%d' % it]) < 1e-5


@pytest.mark.parametrize('scale', SCALES)
def test_hip_model_keys_and_shapes_match_reference(scale):
    from sradsgan_amd.model import amssrn as H
    G = H.GeneratorResNet(scale=scale)
    g = golden(scale)
    assert sorted(G.state_dict().keys()) == list(g['keys'])
    assert [k for k, _ in unique_params(G)] == list(g['names'])
    r = R.Generator(scale)
    assert {k: v.shape for k, v in G.state_dict().items()} == {k: v.shape for k, v in r.state_dict().items()}
    if scale == 9:
        assert G.tail[0].weight is G.tail[2].weight and len(G.state_dict()) == len(unique_params(G)) + 2
    G.load_state_dict(init_(r).state_dict(), strict=True)
    assert float(G.gamma.detach()) == 0.5 and float(G.body[0].c1.rb[1].weight.detach()) == pytest.approx(-0.3)
