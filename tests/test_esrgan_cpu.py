"""ESRGAN without a GPU: the CPU restatement (tests/esrgan_ref.py) against vectors recorded from the reference's model/architecture.py,
model/block.py and GANLoss (tools/make_golden_esrgan.py); the HIP model's parameter layout against the reference's; the criteria
restatement against torch's own losses in fp64; every refusal; checkpoint conversion and network interpolation."""
import argparse
import functools
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import esrgan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_KEYS = {2: 70, 3: 70, 4: 72, 8: 74}
D_KEYS = {96: 69, 128: 69, 192: 83, 256: 83}


@functools.lru_cache(maxsize=None)
def golden(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'esrgan_%s.npz' % name))


def ref_generator(scale, nb=2, dtype=torch.float32, tag=''):
    return R.fill_generator(R.Generator(nb, scale), tag=tag).to(dtype)


def ref_discriminator(size, dtype=torch.float32):
    return R.fill_discriminator(R.Discriminator(size), size).to(dtype)


def ref_extractor(dtype=torch.float32):
    return R.fill_extractor(R.Vgg()).to(dtype)


def case_tag(gan_type, relative):
    return '%s_%s' % (gan_type, 'rel' if relative else 'plain')


# ---- key layouts --------------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('scale', R.SCALES)
def test_generator_keys_equal_the_reference(scale):
    from sradsgan_amd.model import esrgan as E
    want = list(golden('keys')['g_x%d' % scale])
    assert len(want) == G_KEYS[scale]
    hip = E.RRDBNet(3, 3, 64, 2, upscale=scale)                      # built on the CPU
    ref = ref_generator(scale)
    assert sorted(hip.state_dict().keys()) == want and sorted(ref.state_dict().keys()) == want
    hip.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(hip.state_dict(), strict=True)
    if scale == 4:
        assert {'model.0.weight', 'model.1.sub.0.RDB1.conv1.0.weight', 'model.1.sub.2.bias', 'model.3.weight', 'model.6.weight',
                'model.8.weight', 'model.10.bias'} <= set(want)


def test_pixelshuffle_generator_has_the_reference_slots():
    from sradsgan_amd.model import esrgan as E
    hip = E.RRDBNet(3, 3, 64, 1, upscale=4, upsample_mode='pixelshuffle')
    ref = R.Generator(1, 4, upsample_mode='pixelshuffle')
    assert sorted(hip.state_dict().keys()) == sorted(ref.state_dict().keys())
    assert tuple(hip.state_dict()['model.2.weight'].shape) == (256, 64, 3, 3)
    hip.load_state_dict(ref.state_dict(), strict=True)


@pytest.mark.parametrize('size', R.D_SIZES)
def test_discriminator_keys_equal_the_reference(size):
    from sradsgan_amd.model import esrgan as E
    want = list(golden('keys')['d_%d' % size])
    assert len(want) == D_KEYS[size]
    hip = E.DISCRIMINATORS[size](3, 64)
    ref = ref_discriminator(size)
    assert sorted(hip.state_dict().keys()) == want and sorted(ref.state_dict().keys()) == want
    hip.load_state_dict(ref.state_dict(), strict=True)
    assert 'features.3.running_var' in want and 'classifier.2.bias' in want


def test_extractor_keys_and_buffers():
    from sradsgan_amd.model import esrgan as E
    hip, ref = E.VGGFeatureExtractor(), R.Vgg()
    assert sorted(hip.state_dict().keys()) == sorted(ref.state_dict().keys()) and len(hip.state_dict()) == 34
    assert torch.equal(hip.mean, ref.mean) and torch.equal(hip.std, ref.std)
    assert not any(p.requires_grad for p in hip.parameters())
    hip.load_state_dict(ref.state_dict(), strict=True)
    tv = {k: v for k, v in ref.state_dict().items() if k.startswith('features.')}
    tv['classifier.0.weight'] = torch.zeros(1)                       # a torchvision file carries more than the features
    hip.load_torchvision_vgg19(tv)
    del tv['features.34.bias']
    with pytest.raises(KeyError, match='features.34.bias'):
        hip.load_torchvision_vgg19(tv)


def test_published_parameter_count():
    from sradsgan_amd.model import esrgan as E
    assert sum(p.numel() for p in E.RRDBNet(3, 3, 64, 23).parameters()) == 16697987
    assert sum(p.numel() for p in R.Generator(23, 4).parameters()) == 16697987


# ---- the restatement against the recorded reference ------------------------------------------------------------------------------ #

@pytest.mark.parametrize('scale', R.SCALES)
def test_restatement_generator_matches_reference_vectors(scale):
    g = golden('gen')
    G = ref_generator(scale)
    y = G(R.gen_input(scale))
    assert np.abs(R.out_digest(y) - g['y_x%d' % scale]).max() < 2e-5
    (y * R.gen_functional(scale)).sum().backward()
    dig = np.concatenate([R.small_digest(p.grad) for _, p in G.named_parameters()])
    ref = g['grads_x%d' % scale]
    assert dig.shape == ref.shape and np.abs(dig - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_restatement_full_depth_generator_matches_reference_vector():
    G = ref_generator(4, nb=23, tag='23')
    with torch.no_grad():
        y = G(O.det_fill('esrgan.deep.x', R.DEEP_SHAPE, 0.5, 0.5))
    assert np.abs(R.out_digest(y) - golden('gen')['y_deep']).max() < 2e-5


@pytest.mark.parametrize('size', R.D_SIZES)
def test_restatement_discriminator_matches_reference_vectors(size):
    g = golden('disc')
    D = ref_discriminator(size)
    x = R.d_input(size).requires_grad_()
    out = D(x)
    out.sum().backward()
    assert tuple(out.shape) == (2, 1)
    assert np.abs(out.detach().numpy() - g['out_%d' % size]).max() < 2e-5
    ref = g['dx_%d' % size]
    assert np.abs(R.out_digest(x.grad) - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    for k, b in R.bn_buffers(D):
        assert np.abs(b.numpy() - g['buf_%d__%s' % (size, k.replace('.', '__'))]).max() < 1e-5, k


@pytest.mark.parametrize('gan_type,relative', R.STEP_CASES)
def test_restatement_two_iterations_match_reference(gan_type, relative):
    g, tag = golden('step'), case_tag(gan_type, relative)
    G, D, Fx = ref_generator(R.STEP_SCALE), ref_discriminator(R.STEP_D), ref_extractor()
    x, t = R.step_inputs()
    opt_G = torch.optim.Adam(G.parameters(), lr=R.ADAM_LR, betas=(0.9, 0.999))
    opt_D = torch.optim.Adam(D.parameters(), lr=R.ADAM_LR, betas=(0.9, 0.999))
    for it in range(2):
        out = R.train_iteration(G, D, Fx, opt_G, opt_D, x, t, gan_type, relative, **R.WEIGHTS)
        got = np.array([out[k] for k in ('loss_G', 'loss_D', 'pixel', 'content', 'loss_gan')])
        print(tag, it, got, np.abs(got - g[tag][it]).max())
        assert np.abs(got - g[tag][it]).max() < 1e-5 * max(1.0, np.abs(g[tag][it]).max()), (it, got, g[tag][it])
        for net, name in ((G, 'G'), (D, 'D')):
            d = np.abs(np.concatenate([R.small_digest(p.detach()) for _, p in net.named_parameters()]) - g['%s_step%d_%s' % (tag, it, name)])
            # sampled elements: Adam turns a roundoff-signed gradient into a full lr step; sums / norms: a few such elements each
            assert np.median(d) <= 1e-6 and d.max() <= 2 * R.ADAM_LR * (it + 1) * 64, (it, name, d.max())
        bufs = np.concatenate([R.small_digest(b) for _, b in R.bn_buffers(D)])
        ref = g['%s_step%d_Dbuf' % (tag, it)]
        err = np.abs(bufs - ref).max() / max(1.0, np.abs(ref).max())
        print(tag, it, 'BN buffers', err)
        # after the first step the weights carry the +-lr Adam steps above, which move the second call's batch statistics
        assert err < (1e-4 if it == 0 else 1e-2)


# ---- the criteria restatement against torch's losses ------------------------------------------------------------------------------ #

@pytest.mark.parametrize('gan_type', ['vanilla', 'lsgan'])
@pytest.mark.parametrize('labels', [(1.0, 0.0), (0.9, 0.1)])
def test_criteria_restatement_equals_torch_losses_in_fp64(gan_type, labels):
    loss = torch.nn.BCEWithLogitsLoss() if gan_type == 'vanilla' else torch.nn.MSELoss()
    real = (O.det_fill('crit.real', (5, 1), 3.0)).double()
    fake = (O.det_fill('crit.fake', (5, 1), 3.0)).double()

    def c_torch(x, is_real):
        return loss(x, torch.empty_like(x).fill_(labels[0] if is_real else labels[1]))

    def both(fn_restated, fn_torch):
        out = []
        for fn in (fn_restated, fn_torch):
            r, f = real.clone().requires_grad_(), fake.clone().requires_grad_()
            v = fn(r, f)
            v.backward()
            out.append((v.detach(), r.grad, f.grad))
        for a, b in zip(*out):
            if a is None or b is None:
                assert a is None and b is None
            else:
                assert torch.allclose(a, b, rtol=1e-13, atol=1e-15)

    both(lambda r, f: R.criterion(r, True, gan_type, *labels) + R.criterion(f, False, gan_type, *labels),
         lambda r, f: c_torch(r, True) + c_torch(f, False))
    both(lambda r, f: R.ragan_d(r, f, gan_type, *labels),
         lambda r, f: (c_torch(r - torch.mean(f), True) + c_torch(f - torch.mean(r), False)) / 2)
    both(lambda r, f: R.ragan_g(r, f, gan_type, *labels),
         lambda r, f: (c_torch(r.detach() - torch.mean(f), False) + c_torch(f - torch.mean(r.detach()), True)) / 2)
    x = torch.tensor([-100.0, 100.0, 0.0], dtype=torch.float64)
    assert torch.isfinite(R.criterion(x, True, gan_type)) and torch.isnan(R.criterion(x * float('nan'), True, gan_type))


def test_head_restatement_is_the_nchw_flatten():
    x = O.det_fill('head.x', (2, 8, 3, 3), 1.0).double()
    w0, b0 = O.det_fill('head.w0', (5, 72), 0.3).double(), O.det_fill('head.b0', (5,), 0.1).double()
    w1, b1 = O.det_fill('head.w1', (1, 5), 0.3).double(), O.det_fill('head.b1', (1,), 0.1).double()
    z = torch.einsum('jcp,bcp->bj', w0.view(5, 8, 9), x.view(2, 8, 9)) + b0
    want = torch.where(z > 0, z, 0.2 * z) @ w1.t() + b1
    assert torch.allclose(R.head(x, w0, b0, w1, b1), want, rtol=1e-13, atol=1e-15)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------- #

def test_generator_refusals_say_why():
    from sradsgan_amd.model import esrgan as E
    for kwargs, msg in ((dict(nf=32), 'nf = 64, gc = 32'), (dict(gc=16), 'nf = 64, gc = 32'), (dict(norm_type='batch'), 'norm_type'),
                        (dict(act_type='relu'), 'act_type'), (dict(mode='NAC'), 'mode'), (dict(upscale=9), 'x8 network under an x9 name'),
                        (dict(upscale=5), 'upscale must be one of'), (dict(upsample_mode='deconv'), 'upsample mode')):
        args = dict(in_nc=3, out_nc=3, nf=64, nb=2)
        args.update(kwargs)
        with pytest.raises(NotImplementedError, match=msg):
            E.RRDBNet(**args)
    with pytest.raises(ValueError, match='nb must be an integer >= 1'):
        E.RRDBNet(3, 3, 64, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.RRDBNet(3, 3, 64, 1)(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match='30 tensors'):
        E.rrdb_step(torch.zeros(1, 64, 4, 4), [torch.zeros(1)] * 32)


def test_discriminator_extractor_and_criterion_refusals_say_why():
    from sradsgan_amd.model import esrgan as E
    with pytest.raises(NotImplementedError, match='base_nf = 64 only'):
        E.Discriminator_VGG_128(3, 32)
    for kwargs in (dict(norm_type='instance'), dict(norm_type=None), dict(act_type='relu'), dict(mode='NAC')):
        with pytest.raises(NotImplementedError, match="norm_type='batch', act_type='leakyrelu', mode='CNA'"):
            E.Discriminator_VGG_96(3, 64, **kwargs)
    for cls, size in ((E.Discriminator_VGG_96, 128), (E.Discriminator_VGG_128, 96), (E.Discriminator_VGG_192, 256),
                      (E.Discriminator_VGG_256, 192)):
        with pytest.raises(ValueError, match=r'\(96, 128, 192, 256\)'):
            cls(3, 64)(torch.zeros(1, 3, size, size))
    with pytest.raises(NotImplementedError, match='use_bn'):
        E.VGGFeatureExtractor(use_bn=True)
    with pytest.raises(NotImplementedError, match='feature_layer=34'):
        E.VGGFeatureExtractor(feature_layer=35)
    with pytest.raises(NotImplementedError, match='is not found'):
        E.GANLoss('hinge')
    for t in E.GAN_TYPES:
        assert E.GANLoss(t.upper()).gan_type == t
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.gan_loss(torch.zeros(4, 1), True, 'vanilla')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.dhead(torch.zeros(1, 64, 1, 1), torch.zeros(100, 64), torch.zeros(100), torch.zeros(1, 100), torch.zeros(1))


def test_trainer_picks_the_discriminator_by_crop_size_and_refuses_the_rest():
    from sradsgan_amd.model import esrgan as E
    for size in R.D_SIZES:
        t = object.__new__(E.ESRGAN)                                 # (the constructor needs a device; the choice does not)
        t.crop_size = size
        D = t._new_discriminator()
        assert type(D) is E.DISCRIMINATORS[size] and type(D).__name__ == 'Discriminator_VGG_%d' % size and D.size == size
    t = object.__new__(E.ESRGAN)
    t.nb, t.scale_factor = 2, 3
    G = t._new_generator()
    assert isinstance(G, E.RRDBNet) and G.nb == 2 and G.upscale == 3
    assert E.ESRGAN.eval_label == 'esrgan'
    a = E.default_args()
    assert (a.nb, a.gan_type, a.relativeGan, a.gp, a.clip_value, a.crop_size, a.scale_factor) == (23, 'vanilla', True, False, None, 128, 4)
    with pytest.raises(ValueError, match='no Discriminator_VGG_'):
        E.ESRGAN(E.default_args(crop_size=216))
    with pytest.raises(NotImplementedError, match='differentiable once'):
        E.ESRGAN(E.default_args(gp=True))
    with pytest.raises(NotImplementedError, match='differentiable once'):
        E.TrainStep(None, None, None, use_gp=True)
    for kwargs in (dict(d_norm_type='instance'), dict(d_attention=True), dict(d_spectralnorm=True)):
        with pytest.raises(NotImplementedError, match='Discriminator_VGG_'):
            E.ESRGAN(argparse.Namespace(**dict(vars(E.default_args()), **kwargs)))
    with pytest.raises(NotImplementedError, match='weight_lpips'):
        E.ESRGAN(E.default_args(weight_lpips=0.1))
    with pytest.raises(NotImplementedError, match='weight_contrast'):
        E.ESRGAN(E.default_args(weight_contrast=0.1))
    with pytest.raises(NotImplementedError, match='is not found'):
        E.ESRGAN(E.default_args(gan_type='hinge'))
    with pytest.raises(NotImplementedError, match='scale_factor'):
        E.ESRGAN(E.default_args(scale_factor=9))


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------- #

def _renamed(sd, layout, nb):
    fixed = {'new': {'model.0': 'conv_first', 'model.1.sub.%d' % nb: 'trunk_conv', 'model.3': 'upconv1', 'model.6': 'upconv2',
                     'model.8': 'HRconv', 'model.10': 'conv_last'},
             'basicsr': {'model.0': 'conv_first', 'model.1.sub.%d' % nb: 'conv_body', 'model.3': 'conv_up1', 'model.6': 'conv_up2',
                         'model.8': 'conv_hr', 'model.10': 'conv_last'}}[layout]
    out = OrderedDict()
    for k, v in sd.items():
        stem, leaf = k.rsplit('.', 1)
        if stem in fixed:
            out['%s.%s' % (fixed[stem], leaf)] = v
        else:
            _, _, _, i, rdb, conv, _ = stem.split('.')                # model.1.sub.{i}.RDB{j}.conv{k}.0
            if layout == 'new':
                out['RRDB_trunk.%s.%s.%s.%s' % (i, rdb, conv, leaf)] = v
            else:
                out['body.%s.%s.%s.%s' % (i, rdb.lower(), conv, leaf)] = v
    return out


def test_convert_state_dict_round_trips_the_three_layouts():
    from sradsgan_amd.model import esrgan as E
    nb = 2
    sd = ref_generator(4, nb).state_dict()
    same = E.convert_state_dict(sd)
    assert list(same.keys()) == list(sd.keys()) and all(same[k] is sd[k] for k in sd)
    for layout in ('new', 'basicsr'):
        other = _renamed(sd, layout, nb)
        assert len(other) == len(sd) and not any(k.startswith('model.') for k in other)
        back = E.convert_state_dict(other)
        assert sorted(back.keys()) == sorted(sd.keys()) and all(back[k] is sd[k] for k in sd)
        hip = E.RRDBNet(3, 3, 64, nb)
        hip.load_state_dict(other, strict=True)                      # the model's own loader converts
        assert all(torch.equal(v, sd[k]) for k, v in hip.state_dict().items())
    with pytest.raises(ValueError, match='unknown key layout'):
        E.convert_state_dict({'generator.conv.weight': torch.zeros(1)})
    with pytest.raises(ValueError, match='does not belong'):
        E.convert_state_dict(dict(_renamed(sd, 'new', nb), **{'extra.weight': torch.zeros(1)}))


def test_interpolate_networks():
    from sradsgan_amd.model import esrgan as E
    a = ref_generator(4, 1).state_dict()
    b = OrderedDict((k, O.det_fill('interp.' + k, tuple(v.shape), 1.0)) for k, v in a.items())
    for alpha in (0.0, 1.0, 0.3):
        out = E.interpolate_networks(a, b, alpha)
        assert list(out.keys()) == list(a.keys())
        for k in a:
            assert out[k] is not a[k] and out[k] is not b[k]
            assert torch.equal(out[k], (1 - alpha) * a[k] + alpha * b[k])
            if alpha in (0.0, 1.0):
                assert torch.equal(out[k], a[k] if alpha == 0.0 else b[k])
    with pytest.raises(ValueError, match='same keys'):
        E.interpolate_networks(a, dict(list(b.items())[:-1]), 0.5)
