"""SpectralPatchDiscriminator's interface without a device: state_dict keys, order, shapes and requires_grad flags per variant against
the list recorded from the reference (tests/golden/disc_spectral.npz) and against the plain-torch restatement; dp.ParamArena over its
parameters; the trainer's argument checks and DRCAN's refusal; the library's new entry points; and the restatement
(tests/spectral_ref.py) against the numbers recorded from the reference itself."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import disc_norms_ref as DR
from tests import gan_options_ref as GR
from tests import spectral_ref as SR

IDS = [SR.tag(*v) for v in SR.VARIANTS]


def _items(m):
    flags = dict(m.named_parameters())
    return [(k, ','.join(map(str, v.shape)), bool(flags[k].requires_grad) if k in flags else False) for k, v in m.state_dict().items()]


@pytest.mark.parametrize('norm_type,attention', SR.VARIANTS, ids=IDS)
def test_keys_shapes_and_flags_are_the_references(golden, norm_type, attention):
    from sradsgan_amd.model import SpectralPatchDiscriminator
    g, name = golden('disc_spectral'), SR.tag(norm_type, attention)
    hd = SpectralPatchDiscriminator(norm_type=norm_type, attention=attention)
    got = _items(hd)
    assert got == list(zip(g[name + '.keys'].tolist(), g[name + '.shapes'].tolist(), g[name + '.requires_grad'].tolist()))
    od = SR.Discriminator(norm_type=norm_type, attention=attention)
    assert got == _items(od)
    assert [k for k, _, _ in got][:4] == ['model.0.module.bias', 'model.0.module.weight_u', 'model.0.module.weight_v', 'model.0.module.weight_bar']
    assert got[1][1:] == ('64', False) and got[2][1:] == ('27', False) and got[3][1:] == ('64,3,3,3', True)
    last = len(hd.model) - 1
    assert ('model.%d.weight' % last, '1,512,3,3', True) in got                      # the last conv is a plain conv
    assert all(isinstance(p, torch.nn.Parameter) for p in hd.parameters())
    SR.fill_(od)
    hd.load_state_dict(od.state_dict(), strict=True)
    for (k, a), (_, b) in zip(hd.state_dict().items(), od.state_dict().items()):
        assert torch.equal(a, b), k
    for sn in hd.spectral_layers():                                                  # as constructed: unit vectors
        assert abs(float(sn.module.weight_u.norm()) - 1) < 1e-5 and abs(float(sn.module.weight_v.norm()) - 1) < 1e-5


def test_wrapper_and_refusals():
    from sradsgan_amd.model import PatchDiscriminator, SpectralNorm, SpectralPatchDiscriminator
    from sradsgan_amd.model.layers import HipConv2d
    sn = SpectralNorm(HipConv2d(8, 5, 3, 2, 1))
    assert list(sn.state_dict()) == ['module.bias', 'module.weight_u', 'module.weight_v', 'module.weight_bar']
    assert not hasattr(sn.module, 'weight') and sn.name == 'weight' and sn.power_iterations == 1
    assert tuple(sn.module.weight_u.shape) == (5,) and tuple(sn.module.weight_v.shape) == (72,)
    with pytest.raises(NotImplementedError, match='power_iterations'):
        SpectralNorm(HipConv2d(8, 5, 3, 1, 1), power_iterations=2)
    with pytest.raises(NotImplementedError):
        SpectralNorm(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match='norm_type'):
        SpectralPatchDiscriminator(norm_type='layer')
    with pytest.raises(NotImplementedError, match='u and v on every forward'):      # the refusal stays where it was
        PatchDiscriminator(use_spectralnorm=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                       # no CPU path
        SpectralPatchDiscriminator()(torch.zeros(1, 3, 8, 8))


def test_param_arena_holds_u_and_v_with_zero_slots():
    from sradsgan_amd.dp import ParamArena
    from sradsgan_amd.model import SpectralPatchDiscriminator
    d = SpectralPatchDiscriminator(norm_type='', attention=True)
    before = {k: p.detach().clone() for k, p in d.named_parameters()}
    arena = ParamArena(d)
    assert arena.check_views() and len(arena.params) == len(before)
    lo, hi = arena.flat_p.data_ptr(), arena.flat_p.data_ptr() + 4 * arena.numel
    n_uv = 0
    for k, p in d.named_parameters():
        assert torch.equal(p.detach(), before[k]) and lo <= p.data_ptr() < hi
        if k.endswith(('weight_u', 'weight_v')):
            n_uv += 1
            assert not p.requires_grad and p.grad is not None and not bool(p.grad.any())
    assert n_uv == 16


def test_train_step_never_turns_requires_grad_on_for_u_and_v():
    from sradsgan_amd.model import SpectralPatchDiscriminator
    from sradsgan_amd.train_step import TrainStep
    d = SpectralPatchDiscriminator()
    lin = torch.nn.Linear(1, 1)
    step = TrainStep(lin, d, torch.nn.Linear(1, 1), overlap_wgrad=False)
    assert step._spectral
    for flag in (False, True):
        step._set_d_grad(flag)
        for k, p in d.named_parameters():
            assert p.requires_grad == (flag and not k.endswith(('weight_u', 'weight_v'))), k
    with pytest.raises(ValueError, match='use_graph'):
        TrainStep(lin, SpectralPatchDiscriminator(), torch.nn.Linear(1, 1), use_graph=True, overlap_wgrad=False)


def test_trainer_arguments_and_drcan_refusal():
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import PatchDiscriminator, SpectralPatchDiscriminator, drcan
    with pytest.raises(ValueError, match='explicit args.d_norm_type'):               # no silent choice between BatchNorm and ''
        T.SRADSGAN(T.default_args(data_dir='.', root_dir='.', d_spectralnorm=True))
    with pytest.raises(ValueError, match='d_spectralnorm must be a bool'):
        T.SRADSGAN(T.default_args(data_dir='.', root_dir='.', d_spectralnorm='yes', d_norm_type=''))
    with pytest.raises(ValueError, match='d_norm_type'):
        T.SRADSGAN(T.default_args(data_dir='.', root_dir='.', d_spectralnorm=True, d_norm_type='layer'))
    with pytest.raises(NotImplementedError, match='DRCAN'):
        drcan.DRCAN(T.default_args(data_dir='.', root_dir='.', d_spectralnorm=True))

    def built(**kw):
        t = object.__new__(T.SRADSGAN)
        ns = argparse.Namespace(**kw)
        t.d_norm_type, t.d_attention = getattr(ns, 'd_norm_type', None), bool(getattr(ns, 'd_attention', False))
        t.d_spectralnorm = getattr(ns, 'd_spectralnorm', False)
        return t._new_discriminator()

    for nt in ('', 'instance', 'group', 'batch'):
        d = built(d_norm_type=nt, d_spectralnorm=True, d_attention=True)
        assert type(d) is SpectralPatchDiscriminator and d.norm_type == nt and d.attention is True
    assert type(built(d_norm_type='', d_spectralnorm=False)) is PatchDiscriminator


def test_spectral_init_is_the_documented_departure():
    from sradsgan_amd.model import SpectralPatchDiscriminator
    from sradsgan_amd.model.spectral import spectral_init_
    from sradsgan_amd.trainer import weights_init_normal
    d = SpectralPatchDiscriminator(norm_type='batch', attention=True)
    with pytest.raises(AttributeError):                                              # what the reference's apply() does to a spectral D
        d.apply(weights_init_normal)
    d = SpectralPatchDiscriminator(norm_type='batch', attention=True)
    uv = {k: p.detach().clone() for k, p in d.named_parameters() if k.endswith(('weight_u', 'weight_v'))}
    torch.manual_seed(3)
    spectral_init_(d)
    sd = dict(d.named_parameters())
    for k, p in uv.items():
        assert torch.equal(sd[k].detach(), p), k
    for sn in d.spectral_layers():
        assert not bool(sn.module.bias.detach().any()) and 0.01 < float(sn.module.weight_bar.detach().std()) < 0.03
    assert abs(float(d.model[3].weight.detach().mean()) - 1) < 0.02 and 0.01 < float(d.model[len(d.model) - 1].weight.detach().std()) < 0.03


def test_new_entry_points_on_the_host():
    import os
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    assert lib.srhip_abi_version() == 14 and lib.srhip_sn_entry_bytes() == 88
    assert lib.srhip_sn_tpart_elems(512, 4608) == 2 * 16 * 4608 and lib.srhip_sn_tpart_elems(1, 9) == 18 and lib.srhip_sn_tpart_elems(0, 9) == 0
    assert lib.srhip_sn_dot_parts(512, 4608) == 576 and lib.srhip_sn_dot_parts(5, 27) == 1 and lib.srhip_sn_dot_parts(64, 0) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                           # stands for every device argument: a refused call never reads it
    assert lib.srhip_sn_forward_batched(None, 1, p, 64, 27, None) == -1
    assert lib.srhip_sn_forward_batched(p, 1, p, 0, 27, None) == -1 and lib.srhip_sn_forward_batched(p, 70000, p, 64, 27, None) == -1
    assert lib.srhip_sn_forward_batched(p, 1, p + 4, 64, 27, None) == -1 and b'aligned' in lib.srhip_last_error()
    assert lib.srhip_sn_forward_batched(p, 0, p, 64, 27, None) == 0                  # nothing to do, nothing launched
    ptrs = (ctypes.c_void_p * 1)(p)
    none = (ctypes.c_void_p * 1)(None)
    assert lib.srhip_sn_backward_batched(p, 1, p, ptrs, none, p, 64, 27, None) == -1 and b'no slot' in lib.srhip_last_error()
    assert lib.srhip_sn_backward_batched(p, 1, p, ptrs, ptrs, None, 64, 27, None) == -1


@pytest.mark.parametrize('norm_type,attention', SR.NUMBERED, ids=[SR.tag(*v) for v in SR.NUMBERED])
def test_restatement_reproduces_the_recorded_reference(golden, norm_type, attention):
    """Same torch ops in the same order as the reference on the same CPU arithmetic: 2e-4 of each tensor's scale, u / v / sigma after
    each of the four passes within 1e-6."""
    g, name = golden('disc_spectral'), SR.tag(norm_type, attention)
    suffix, scale = int(g[name + '.suffix']), float(g[name + '.conv_scale'])
    assert float(g[name + '.signal'].min()) >= 0.1 and float(g[name + '.signal'].max()) <= 10
    assert all(f <= 0.5 * b for f, b in zip(g[name + '.stability'].tolist(), (1e-3, 2e-3, 2e-3, 1e-4, 5e-3)))
    d = SR.fill_(SR.Discriminator(norm_type=norm_type, attention=attention), suffix, scale)
    r = SR.run(d, SR.inputs(suffix), torch.from_numpy(g['alpha']), SR.restated_penalty)

    def close(got, want, what, tol=2e-4):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        err, sc = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-4)
        assert got.shape == want.shape and err <= tol * sc, (name, what, err, sc)

    assert list(r['grads']) == g[name + '.names'].tolist() and not any(k.endswith(('weight_u', 'weight_v')) for k in r['grads'])
    close(r['y'].numpy().ravel(), g[name + '.y'], 'y')
    close(O.digest(r['dx']), g[name + '.dx'], 'dx')
    close(np.concatenate([DR.digest(v) for v in r['grads'].values()]), g[name + '.grads'], 'grads')
    assert abs(r['gp'] - float(g[name + '.gp'])) < 2e-5
    close(np.concatenate([DR.digest(v) for v in r['gp_grads'].values()]), g[name + '.gp_grads'], 'gp grads')
    for i, (u, v, s) in enumerate(r['states'], start=1):
        assert float(np.abs(u - g['%s.u%d' % (name, i)]).max()) < 1e-6 and float(np.abs(v - g['%s.v%d' % (name, i)]).max()) < 1e-6
        close(s, g['%s.sigma%d' % (name, i)], 'sigma %d' % i, 1e-6)
    # the passes move the vectors: a pass that did not advance them would meet the previous pass's numbers, not its own
    assert float(np.abs(g[name + '.u2'] - g[name + '.u1']).max()) > 1e-3 and float(np.abs(g[name + '.u4'] - g[name + '.u3']).max()) > 1e-3


@pytest.mark.parametrize('case', list(SR.TRAIN_CASES))
def test_restatement_reproduces_the_recorded_iteration(golden, case):
    """oracle generator / feature extractor + the restated spectral discriminator through gan_options_ref.train_step against the
    iteration recorded on the reference's modules (scalars 2e-5; gradients 1e-3 in digest_score's measure; post-clamp u / v 1e-6), and
    the conditions the tool established: the passes differ, the iteration count shows."""
    g, name = golden('disc_spectral'), SR.tag('', True)
    key, sh = '%s.it_%s' % (name, case), GR.TRAIN_SHAPE
    G = O.det_init_(O.GeneratorResNet(O.ResGroup, n_residual_blocks=sh['n_groups'], n_basic_blocks=sh['n_blocks'], upscale_factor=sh['scale']), prefix='G.')
    Fx = O.det_init_(O.FeatureExtractor(), prefix='F.')
    D = SR.fill_(SR.Discriminator(norm_type='', attention=True), int(g[name + '.suffix']), float(g[name + '.conv_scale']))
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    sc = GR.train_step(G, D, Fx, torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999)),
                       torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.999)), lr_img, hr_img, torch.from_numpy(g['train_alpha']),
                       **SR.TRAIN_CASES[case])
    assert float(np.abs(np.array([sc[k] for k in GR.SCALARS]) - g[key + '_scalars']).max()) < 2e-5
    assert 0.01 < sc['gp'] < 100
    for tag, net in (('G', G), ('D', D)):
        score, worst = GR.digest_score(net, *[g['%s_%s_%s' % (key, tag, k)] for k in ('names', 'grads', 'counts', 'maxabs')])
        assert score < 1e-3, (tag, worst, score)
    u, v = SR.clamp_uv(D)
    assert float(np.abs(u - g[key + '_u']).max()) < 1e-6 and float(np.abs(v - g[key + '_v']).max()) < 1e-6
    assert float(np.abs(g[key + '_u']).max()) <= 0.01 + 1e-9                          # recorded after the clamp
    gap, fewer, more = g[key + '_conditions'].tolist()
    assert gap > 10 * 1e-3 and fewer > 100 * 1e-5 and more > 100 * 1e-5
