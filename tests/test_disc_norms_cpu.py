"""PatchDiscriminator's interface without a device: state_dict keys and shapes per norm_type against the list recorded from the
reference (tests/golden/disc_norms.npz) and against the plain-torch restatement, the refusals, the trainer's two optional
attributes; and the restatement (tests/disc_norms_ref.py) against the numbers recorded from the reference itself."""
import argparse

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import disc_norms_ref as DR


def _items(m):
    return [(k, ','.join(map(str, v.shape))) for k, v in m.state_dict().items()]


@pytest.mark.parametrize('norm_type,attention', DR.VARIANTS, ids=[DR.tag(*v) for v in DR.VARIANTS])
def test_keys_and_shapes_are_the_references(golden, norm_type, attention):
    from sradsgan_amd.model import PatchDiscriminator
    g, name = golden('disc_norms'), DR.tag(norm_type, attention)
    got = _items(PatchDiscriminator(norm_type=norm_type, attention=attention))
    assert got == list(zip(g[name + '.keys'].tolist(), g[name + '.shapes'].tolist()))
    assert got == _items(DR.Discriminator(norm_type=norm_type, attention=attention))
    if norm_type == 'instance':
        assert not any('.running_' in k for k, _ in got) and len(got) == len(_items(PatchDiscriminator(norm_type='', attention=attention)))
    if norm_type == 'group':
        assert ('model.3.weight', '1,64,1,1') in got and ('model.3.bias', '1,64,1,1') in got


@pytest.mark.parametrize('attention', [False, True])
def test_batch_variant_is_the_existing_discriminator(attention):
    from sradsgan_amd.model import PatchDiscriminator, base_networks
    assert _items(PatchDiscriminator(norm_type='batch', attention=attention)) == _items(base_networks.Discriminator(norm_type='batch', attention=attention))
    assert _items(PatchDiscriminator(norm_type='batch', attention=attention)) == _items(DR.Discriminator(norm_type='batch', attention=attention))


def test_refusals():
    from sradsgan_amd.model import PatchDiscriminator
    from sradsgan_amd.model.layers import GroupNorm, HipInstanceNorm2d
    with pytest.raises(NotImplementedError, match='u and v on every forward'):
        PatchDiscriminator(use_spectralnorm=True)
    with pytest.raises(ValueError, match='norm_type'):
        PatchDiscriminator(norm_type='layer')
    with pytest.raises(NotImplementedError):
        HipInstanceNorm2d(8, affine=True)
    with pytest.raises(ValueError):
        GroupNorm(48)
    assert list(HipInstanceNorm2d(8).state_dict()) == [] and [tuple(p.shape) for p in GroupNorm(64).parameters()] == [(1, 64, 1, 1)] * 2


def test_weights_init_normal_leaves_group_norm_at_its_identity():
    """utils.weights_init_normal matches 'Conv2d' and 'BatchNorm' class names only: GroupNorm keeps weight = 1, bias = 0."""
    from sradsgan_amd.model import PatchDiscriminator
    from sradsgan_amd.trainer import weights_init_normal
    d = PatchDiscriminator(norm_type='group', attention=True).apply(weights_init_normal)
    norms = [m for m in d.modules() if m.__class__.__name__ == 'GroupNorm']
    assert len(norms) == 7 and all(bool((m.weight == 1).all()) and bool((m.bias == 0).all()) for m in norms)
    assert float(d.model[0].weight.detach().std()) < 0.05


def test_trainer_reads_d_norm_type_and_d_attention():
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import Discriminator, PatchDiscriminator, drcan
    with pytest.raises(ValueError, match='d_norm_type'):                 # checked at construction, before any device is touched
        T.SRADSGAN(T.default_args(data_dir='.', root_dir='.', d_norm_type='layer'))
    with pytest.raises(NotImplementedError, match='DRCAN'):
        drcan.DRCAN(T.default_args(data_dir='.', root_dir='.', d_norm_type='instance'))

    def built(**kw):
        t = object.__new__(T.SRADSGAN)                                   # _new_discriminator reads these two attributes only
        ns = argparse.Namespace(**kw)
        t.d_norm_type, t.d_attention = getattr(ns, 'd_norm_type', None), bool(getattr(ns, 'd_attention', False))
        return t._new_discriminator()

    assert type(built()) is Discriminator and type(built(d_norm_type=None)) is Discriminator
    for nt in ('', 'instance', 'group', 'batch'):
        d = built(d_norm_type=nt)
        assert type(d) is PatchDiscriminator and d.norm_type == nt and d.attention is False
    assert built(d_norm_type='group', d_attention=True).attention is True


@pytest.mark.parametrize('norm_type,attention', DR.VARIANTS, ids=[DR.tag(*v) for v in DR.VARIANTS])
def test_restatement_reproduces_the_recorded_reference(golden, norm_type, attention):
    """Same torch ops in the same order as the reference on the same CPU arithmetic: 2e-4 of each tensor's scale (the recorded
    fp64-vs-rounded-operand figures of the fixture, its own sensitivity measure, are below that for every variant)."""
    g, name = golden('disc_norms'), DR.tag(norm_type, attention)
    suffix, scale = int(g[name + '.suffix']), float(g[name + '.conv_scale'])
    assert float(g[name + '.signal'].min()) >= 0.1 and float(g[name + '.signal'].max()) <= 10
    assert all(f <= 0.5 * b for f, b in zip(g[name + '.stability'].tolist(), (1e-3, 2e-3, 2e-3, 1e-4, 5e-3)))
    d = DR.fill_(DR.Discriminator(norm_type=norm_type, attention=attention), suffix, scale)
    r = DR.run(d, DR.inputs(suffix), torch.from_numpy(g['alpha']), DR.restated_penalty)

    def close(got, want, what):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        err, sc = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-4)
        assert err <= 2e-4 * sc, (name, what, err, sc)

    assert list(r['grads']) == g[name + '.names'].tolist()
    close(r['y'].numpy().ravel(), g[name + '.y'], 'y')
    close(O.digest(r['dx']), g[name + '.dx'], 'dx')
    close(np.concatenate([DR.digest(v) for v in r['grads'].values()]), g[name + '.grads'], 'grads')
    assert abs(r['gp'] - float(g[name + '.gp'])) < 2e-5
    close(np.concatenate([DR.digest(v) for v in r['gp_grads'].values()]), g[name + '.gp_grads'], 'gp grads')


@pytest.mark.parametrize('norm_type', DR.NORM_TYPES, ids=['none', 'instance', 'group'])
def test_restatement_reproduces_the_recorded_iteration(golden, norm_type):
    """oracle generator / feature extractor + the restated discriminator through gan_options_ref.train_step against the iteration
    recorded on the reference's modules: the same ops on the same CPU arithmetic (scalars 2e-5; gradients 1e-3 in digest_score's
    measure, a twentieth of the GPU test's bar for D)."""
    from tests import gan_options_ref as GR
    g, name = golden('disc_norms'), DR.tag(norm_type, True)
    sh = GR.TRAIN_SHAPE
    G = O.det_init_(O.GeneratorResNet(O.ResGroup, n_residual_blocks=sh['n_groups'], n_basic_blocks=sh['n_blocks'], upscale_factor=sh['scale']), prefix='G.')
    Fx = O.det_init_(O.FeatureExtractor(), prefix='F.')
    D = DR.fill_(DR.Discriminator(norm_type=norm_type, attention=True), int(g[name + '.suffix']), float(g[name + '.conv_scale']))
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    sc = GR.train_step(G, D, Fx, torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999)),
                       torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.999)), lr_img, hr_img, torch.from_numpy(g['train_alpha']))
    assert float(np.abs(np.array([sc[k] for k in GR.SCALARS]) - g[name + '.it_scalars']).max()) < 2e-5
    assert 0.01 < sc['gp'] < 100            # the penalty carries signal
    for tag, net in (('G', G), ('D', D)):
        score, worst = GR.digest_score(net, *[g['%s.it_%s_%s' % (name, tag, k)] for k in ('names', 'grads', 'counts', 'maxabs')])
        assert score < 1e-3, (tag, worst, score)
