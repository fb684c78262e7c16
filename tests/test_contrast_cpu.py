"""The contrastive VGG19 losses without a device: tests/contrast_ref.py's restatement against the reference's recorded outputs
(tests/golden/contrast.npz, written by tools/make_golden_contrast.py), the module tree of contrast.Vgg19Taps against the reference's
recorded state-dict keys, weight loading, and the argument errors that need no device.

Bound of the restatement check.  The golden values are the reference's own float32 run; the restatement runs in float64.  Features of
the float32 run carry relative errors below 1e-6 (tests/contrast_ref.margins measures them: about 2e-6 on values of about 3), the means
average them, the L1 ratio doubles them and exp(cos / 0.07) multiplies the cosine means' by 14: 1e-5 relative to max(1, |value|)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import contrast_ref as R


@pytest.fixture(scope='module')
def G():
    return np.load(R.GOLDEN)


@pytest.fixture(scope='module')
def cases(G):
    """name -> (a, p, n, taps of a, taps of p, [taps of n_j]) in float64; computed once, never modified."""
    out = {}
    for idx in range(len(R.SHAPES)):
        a, p, n = [torch.from_numpy(G['s%d_%s' % (idx, k)]) for k in 'apn']
        with torch.no_grad():
            out['s%d' % idx] = (a, p, n, R.taps(a.double()), R.taps(p.double()), [R.taps(n[:, j].double()) for j in range(n.shape[1])])
    return out


def test_golden_weights_are_the_generated_ones(G):
    # float64 sums over up to 2.4 M values: their last bits move with the number of threads that summed them
    assert np.allclose(G['backbone_checksum'], R.weights_checksum(R.vgg19_state_dict()), rtol=1e-9, atol=1e-9)
    assert [tuple(G['s%d_a' % i].shape) for i in range(3)] == list(R.SHAPES)


@pytest.mark.parametrize('name', ['s0', 's1', 's2'])
def test_restatement_reproduces_the_reference(G, cases, name):
    _, _, _, fa, fp, fn = cases[name]
    worst = 0.0
    for kind in R.KINDS:
        many = kind.startswith('N')
        for ab in (False, True):
            for nn_ in ((1, 2, 3) if many else (1,)):
                if 'Cosine' in kind:
                    got = R.cos_from_taps(fa, fp, fn[:nn_], many, ab and not many)
                else:
                    got = R.l1_from_taps(fa, fp, fn[:nn_], ab and not many)
                want = float(G['%s_%s_ab%d_n%d' % (name, kind, int(ab), nn_)])
                err = abs(float(got) - want) / max(1.0, abs(want))
                worst = max(worst, err)
                print('%s %s ablation=%s N=%d: reference %.7g, fp64 restatement %.10g, relative difference %.2e' % (
                    name, kind, ab, nn_, want, float(got), err))
                assert err <= 1e-5
    assert worst > 0                                              # float32 against float64: equal bits would mean the same run


def test_loss_entry_point_is_the_taps_composition(G, cases):
    a, p, n, fa, fp, fn = cases['s2']
    assert float(R.loss('NContrastLoss', a, p, n[:, :2])) == float(R.l1_from_taps(fa, fp, fn[:2]))
    assert float(R.loss('ContrastCosineLoss', a, p, n[:, 0], ablation=True)) == float(R.cos_from_taps(fa, fp, fn[:1], False, True))
    val, g = R.loss_and_grad('NContrastCosineLoss', a, p, n)
    assert g.shape == a.shape and g.dtype == torch.float64 and float(g.abs().max()) > 0 and torch.isfinite(val)


def test_cos_restates_the_installed_cosine_similarity():
    a = R.hash16(2 * 8 * 3 * 3, 1).reshape(2, 8, 3, 3).clone()
    x = R.hash16(2 * 8 * 3 * 3, 2).reshape(2, 8, 3, 3).clone()
    a[0, :, 0, 0] = 0
    x[1, :, 1, 1] = 0
    for dt in (torch.float64, torch.float32):
        u, v = a.to(dt), x.to(dt)
        assert torch.equal(R.cos(u, v), F.cosine_similarity(u, v, dim=1))
        g = []
        for fn in (R.cos, lambda s, t: F.cosine_similarity(s, t, dim=1)):
            w = u.clone().requires_grad_(True)
            g.append(torch.autograd.grad(fn(w, v).sum(), w)[0])
        assert torch.equal(g[0], g[1])
        assert torch.isfinite(g[0]).all() and float(g[0][0, :, 0, 0].abs().max()) > 1e6      # zero norm: x_c / (1e-8 |x|), no 0 / 0
        assert bool((g[0][1, :, 1, 1] == 0).all())


@pytest.mark.parametrize('name', ['s0', 's1', 's2'])
def test_inputs_keep_their_margin_from_the_l1_kink(cases, name):
    """The smallest non-zero |a - x| of every tap is at least 64 x the largest fp32-vs-fp64 feature difference there, and the fp32
    run flips no sign (the generator chose the inputs so)."""
    a, p, n = cases[name][:3]
    m = R.margins(a, p, n)
    for t, (small, err, flips) in enumerate(m):
        print('%s tap %d: smallest non-zero difference %.3e, largest fp32 feature error %.3e (ratio %.0f), sign flips %d' % (
            name, t, small, err, small / err, flips))
    assert R.margins_hold(m)


def test_vgg19taps_has_the_reference_state_dict(G):
    from sradsgan_amd.contrast import Vgg19Taps
    sd = Vgg19Taps().state_dict()
    want = {str(k): tuple(int(v) for v in s.split()) for k, s in zip(G['vgg_keys'], G['vgg_shapes'])}
    assert len(want) == 26 and want == R.reference_keys()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert not any(p.requires_grad for p in Vgg19Taps().parameters())
    again = Vgg19Taps().state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)            # the init is deterministic


def test_load_torchvision_vgg19():
    from sradsgan_amd.contrast import Vgg19Taps
    net, sd = Vgg19Taps(), R.vgg19_state_dict()
    extra = dict(sd)
    extra['features.30.weight'] = torch.zeros(1)                    # later layers and the classifier are ignored
    extra['classifier.0.weight'] = torch.zeros(1)
    taken = net.load_torchvision_vgg19(extra)
    assert taken == sorted(sd)
    for i in R.CONVS:
        assert torch.equal(net.conv(i).weight, sd['features.%d.weight' % i]) and torch.equal(net.conv(i).bias, sd['features.%d.bias' % i])
    assert torch.equal(net.state_dict()['slice4.19.weight'], sd['features.19.weight'])
    bad = dict(sd)
    bad['features.10.weight'] = torch.zeros(256, 128, 1, 1)
    with pytest.raises(ValueError, match='features.10.weight'):
        net.load_torchvision_vgg19(bad)
    missing = {k: v for k, v in sd.items() if k != 'features.28.bias'}
    with pytest.raises(KeyError, match='features.28.bias'):
        net.load_torchvision_vgg19(missing)


def test_argument_errors_that_need_no_device():
    from sradsgan_amd import contrast as C
    vgg = C.Vgg19Taps()
    a, p = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)
    for cls in (C.ContrastLoss, C.ContrastCosineLoss):
        loss = cls(vgg=vgg)
        assert loss.vgg is vgg and loss.ab is False and loss.T == 0.07 and loss.weights == [1 / 32, 1 / 16, 1 / 8, 1 / 4, 1.0]
        with pytest.raises(ValueError, match='anchor only'):
            loss(a, p.clone().requires_grad_(True), p)
        with pytest.raises(ValueError, match='anchor only'):
            loss(a, p, p.clone().requires_grad_(True))
        with pytest.raises(ValueError, match='one shape'):
            loss(a, p[:, :, :-1], p)
        with pytest.raises(ValueError, match='shape of a'):
            loss(a, p, torch.zeros(2, 1, 3, 16, 16))
        with pytest.raises(ValueError, match='at least 16'):
            loss(a[:, :, :15], p[:, :, :15], p[:, :, :15])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            loss(a, p, p)
    for cls in (C.NContrastLoss, C.NContrastCosineLoss):
        loss = cls(ablation=True, vgg=vgg)
        with pytest.raises(ValueError, match=r'\[B, N, 3, H, W\]'):
            loss(a, p, p)
        with pytest.raises(ValueError, match='1 <= N <= 8'):
            loss(a, p, torch.zeros(2, 9, 3, 16, 16))
        with pytest.raises(ValueError, match='1 <= N <= 8'):
            loss(a, p, torch.zeros(2, 0, 3, 16, 16))
        with pytest.raises(ValueError, match='anchor only'):
            loss(a, p, torch.zeros(2, 2, 3, 16, 16, requires_grad=True))
    assert C.tap_sizes(40, 44) == [(40, 44), (20, 22), (10, 11), (5, 5), (2, 2)] and C.tap_sizes(16, 16)[-1] == (1, 1)


def test_step_argument_checks():
    from sradsgan_amd.train_step import check_contrast_args
    model = object()
    assert check_contrast_args(None, 0.0, True) is None and check_contrast_args(model, 0.0, False) is None
    assert check_contrast_args(model, 0.5, False) is model
    with pytest.raises(ValueError, match='weight_contrast must be >= 0'):
        check_contrast_args(model, -1.0, False)
    with pytest.raises(ValueError, match='needs contrast'):
        check_contrast_args(None, 1.0, False)
    with pytest.raises(ValueError, match='use_graph'):
        check_contrast_args(model, 1.0, True)
