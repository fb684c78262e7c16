"""DRCAN on the host: the fp64 restatement (tests/drcan_ref.py) against the reference's vectors (tests/golden/drcan_x*.npz, made by
tools/make_golden_drcan.py from the reference's RCAN), the HIP model's state_dict keys and shapes, RCAN's own load_state_dict, the
base_networks discriminator's keys and refusals, and the generator's gradient parts for the data-parallel exchange.  No GPU call is
made here."""
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import drcan_ref as R

SCALES = (2, 3, 4, 8, 9)
SHAPE = (2, 3, 13, 14)
GROUPS, BLOCKS = 2, 2
CASES = [(s, 16) for s in SCALES] + [(2, 4)]          # (scale, reduction); reduction 4 is stored under 'r4_' in the x2 file


def golden(scale, reduction=16):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'drcan_x%d.npz' % scale))
    if reduction == 16:
        return {k: g[k] for k in g.files if not k.startswith('r4_')}
    return {k[3:]: g[k] for k in g.files if k.startswith('r4_')}


def build_ref(scale, reduction=16, groups=GROUPS, blocks=BLOCKS):
    return O.det_init_(R.Generator(scale, groups, blocks, reduction), prefix='R.')


def inputs(scale):
    x = O.det_fill('drcan.x.%d' % scale, SHAPE, 0.5, 0.5)
    t = O.det_fill('drcan.t.%d' % scale, (SHAPE[0], 3, SHAPE[2] * scale, SHAPE[3] * scale), 0.5, 0.5)
    return x, t


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize('scale,reduction', CASES)
def test_restatement_matches_reference_vectors(scale, reduction):
    g = golden(scale, reduction)
    G = build_ref(scale, reduction).double()
    x, t = inputs(scale)
    y = G(x.double())
    l1 = R.loss(y, t.double())
    assert rel(O.digest(y, full_max=4096, nsample=4096), g['y']) < 1e-5
    assert abs(l1.item() - float(g['l1'])) < 1e-6 and abs(R.loss(y, t.double(), 'MSE').item() - float(g['mse'])) < 1e-6
    l1.backward()
    named = list(G.named_parameters())
    assert [k for k, _ in named] == list(g['names'])
    assert rel(np.concatenate([digest(p.grad) for _, p in named]), g['grads']) < 1e-4


@pytest.mark.parametrize('scale,reduction', CASES)
def test_hip_model_keys_and_shapes_match_reference(scale, reduction):
    from sradsgan_amd.model import drcan as H
    G = H.RCAN(n_resgroups=GROUPS, n_resblocks=BLOCKS, reduction=reduction, scale=scale)
    g = golden(scale, reduction)
    assert sorted(G.state_dict().keys()) == list(g['keys'])
    assert [k for k, _ in G.named_parameters()] == list(g['names'])
    r = build_ref(scale, reduction)
    assert {k: v.shape for k, v in G.state_dict().items()} == {k: v.shape for k, v in r.state_dict().items()}
    assert G.load_state_dict(r.state_dict(), strict=True) is None
    for k, v in G.state_dict().items():
        assert torch.equal(v, r.state_dict()[k]), k


@pytest.mark.parametrize('scale', SCALES)
def test_full_training_configuration_matches_reference_count(scale):
    from sradsgan_amd.model import drcan as H
    g = golden(scale)
    G = H.RCAN(n_colors=3, n_resgroups=10, n_resblocks=20, reduction=16, scale=scale)
    assert sum(p.numel() for p in G.parameters()) == int(g['full_params'])
    assert sorted(G.state_dict().keys()) == list(g['full_keys'])
    assert len(G.res_groups) == 10 and len(G.state_dict()) == len(list(G.parameters()))


def test_constructor_defaults_and_refusals():
    import inspect
    from sradsgan_amd.model import drcan as H
    sig = inspect.signature(H.RCAN.__init__).parameters
    assert [(k, sig[k].default) for k in ('n_colors', 'n_resgroups', 'n_resblocks', 'n_feats', 'kernel_size', 'reduction', 'scale',
                                           'res_scale')] == [('n_colors', 3), ('n_resgroups', 5), ('n_resblocks', 10), ('n_feats', 64),
                                                             ('kernel_size', 3), ('reduction', 4), ('scale', 3), ('res_scale', 1)]
    assert inspect.signature(H.CALayer.__init__).parameters['reduction'].default == 4
    G = H.RCAN(n_resgroups=1, n_resblocks=1)                                     # defaults: x3, reduction 4 -> 16 hidden units
    assert tuple(G.body[0].body[0].body[3].conv_du[0].weight.shape) == (16, 64, 1, 1)
    assert [type(m).__name__ for m in G.tail[0]] == ['HipConv2d', '_Shuffle']
    six = H.RCAN(n_resgroups=1, n_resblocks=1, scale=6)                          # the reference's int(log3(6)) = 1: one x3 stage
    assert len(six.tail[0]) == 2 and tuple(six.tail[0][0].weight.shape) == (576, 64, 3, 3)
    for bad in (dict(scale=5), dict(scale=7)):
        with pytest.raises(NotImplementedError):
            H.RCAN(n_resgroups=1, n_resblocks=1, **bad)
    with pytest.raises(NotImplementedError, match='64 features'):
        H.RCAN(n_resgroups=1, n_resblocks=1, n_feats=32)
    with pytest.raises(NotImplementedError, match='3x3'):
        H.RCAN(n_resgroups=1, n_resblocks=1, kernel_size=5)
    with pytest.raises(NotImplementedError):
        H.CALayer(64, reduction=2)                                               # 32 hidden units: beyond the kernel's 16


def test_load_state_dict_across_scales_and_strict(capsys):
    from sradsgan_amd.model import drcan as H
    src = O.det_init_(H.RCAN(n_resgroups=2, n_resblocks=1, reduction=16, scale=3), prefix='S.')
    dst = H.RCAN(n_resgroups=2, n_resblocks=1, reduction=16, scale=4)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    dst.load_state_dict(src.state_dict())
    assert 'Replace pre-trained upsampler to new one...' in capsys.readouterr().out
    s, d = src.state_dict(), dst.state_dict()
    for k, v in d.items():
        if k.startswith('tail.0.0.'):                                            # 64 -> 576 (x3) against 64 -> 256 (x4): keeps its init
            assert torch.equal(v, before[k]), k
        elif k.startswith('tail.0.2.'):                                          # a second x2 stage the x3 checkpoint does not have
            assert torch.equal(v, before[k]) and k not in s, k
        else:
            assert torch.equal(v, s[k]), k
    sd = dict(src.state_dict())
    sd['body.0.body.7.weight'] = torch.zeros(1)                                  # unexpected body key
    with pytest.raises(KeyError, match='unexpected key'):
        H.RCAN(n_resgroups=2, n_resblocks=1, reduction=16, scale=3).load_state_dict(sd, strict=True)
    sd = dict(src.state_dict())
    sd['tail.9.weight'] = torch.zeros(1)                                         # unexpected tail keys are ignored
    H.RCAN(n_resgroups=2, n_resblocks=1, reduction=16, scale=3).load_state_dict(sd, strict=True)
    sd = dict(src.state_dict())
    del sd['body.1.body.0.body.3.conv_du.2.bias']
    with pytest.raises(KeyError, match='missing keys'):
        H.RCAN(n_resgroups=2, n_resblocks=1, reduction=16, scale=3).load_state_dict(sd, strict=True)
    H.RCAN(n_resgroups=2, n_resblocks=1, reduction=16, scale=3).load_state_dict(sd)      # strict=False: no error


def test_base_networks_discriminator_keys_and_refusals():
    from sradsgan_amd.model import Discriminator as PatchD
    from sradsgan_amd.model.base_networks import Discriminator
    for attention in (False, True):
        d = Discriminator(norm_type='batch', use_spectralnorm=False, attention=attention)
        ref = PatchD(attention=attention)
        assert [(k, v.shape) for k, v in d.state_dict().items()] == [(k, v.shape) for k, v in ref.state_dict().items()]
    keys = list(Discriminator(norm_type='batch').state_dict())
    assert keys[:2] == ['model.0.weight', 'model.0.bias'] and 'model.3.running_mean' in keys and keys[-1] == 'model.23.bias'
    for bad in (dict(), dict(norm_type=''), dict(norm_type='instance'), dict(norm_type='group'),
                dict(norm_type='batch', use_spectralnorm=True)):
        with pytest.raises(NotImplementedError):
            Discriminator(**bad)


def test_generator_gradient_leaves_in_parts():
    from sradsgan_amd import train_step as ts
    from sradsgan_amd.dp import ParamArena
    from sradsgan_amd.model import drcan as H
    G = H.RCAN(n_resgroups=6, n_resblocks=1, reduction=16, scale=4)
    keys = list(G.state_dict())
    step = ts.TrainStep.__new__(ts.TrainStep)
    step.G, step.arena_G = G, ParamArena(G)
    parts, rest = step._plan_g_parts(3, any_device=True)
    assert len(parts) == 3 and [k for k, _ in step._part_groups] == [0, 1, 2]
    assert [g for _, g in step._part_groups] == [G.body[4], G.body[2], G.body[0]]
    spans = sorted(parts + rest)
    assert spans[0][0] == 0 and spans[-1][1] == step.arena_G.numel and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert list(G.state_dict()) == keys                                          # res_groups registers nothing


def test_drcan_trainer_defaults_and_refusals():
    from sradsgan_amd.model import drcan as H
    a = H.default_args()
    assert (a.model_name, a.scale_factor, a.batch_size, a.test_batch_size, a.lr, a.lambda_gp, a.clip_value) == \
        ('DRCAN', 4, 16, 16, 0.0002, 10, 0.01)
    assert (a.penalty_type, a.grad_penalty_Lp_norm, a.loss_Lp_norm, a.relativeGan) == ('LS', 'L2', 'L1', False)
    for bad in (dict(relativeGan=True), dict(loss_Lp_norm='L2'), dict(penalty_type='hinge'), dict(grad_penalty_Lp_norm='L1'),
                dict(grad_penalty_Lp_norm='Linf')):
        with pytest.raises(NotImplementedError):
            H.DRCAN(H.default_args(**bad))
