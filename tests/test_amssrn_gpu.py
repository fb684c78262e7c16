"""AMSSRN on the HIP path (sradsgan_amd.model.amssrn) in split-bf16 and exact-fp32 conv arithmetic: the quadrant non-local attention,
the gamma residual and the wide channel attention (C = 320, 768) against fp64 torch with bit-identical reruns; the generator against
the reference's vectors (tests/golden/amssrn_x*.npz) at x2, x3, x4, x8, x9, its gradients against the fp64 restatement
(tests/amssrn_ref.py), two Adam iterations, the training crop (54 -> 216) and one forward in 'half' arithmetic."""
import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import amssrn_ref as R
from tests.test_amssrn_cpu import SCALES, digest, golden, init_, inputs, rel, unique_params

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CL = torch.channels_last
MODES = ['bf16x3', 'fp32']


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def dev(t):
    return t.to(DEV).contiguous(memory_format=CL)


def hip_model(scale, ref=None):
    from sradsgan_amd.model import amssrn as H
    G = H.GeneratorResNet(scale=scale)
    G.load_state_dict((ref if ref is not None else init_(R.Generator(scale))).state_dict(), strict=True)
    return G.to(DEV)


def grad_score(hip, ref):
    """worst |dg| over max(|g| of the parameter, 1e-2 |g| of the network): a parameter whose own gradient is tiny next to the
    network's is held to the network's scale"""
    hp, rp = dict(unique_params(hip)), dict(unique_params(ref))
    gnet = max(float(p.grad.abs().max()) for p in rp.values())
    worst, wk = 0.0, None
    for k, p in rp.items():
        d = float((hp[k].grad.detach().cpu().double() - p.grad).abs().max())
        s = d / max(float(p.grad.abs().max()), 1e-2 * gnet)
        if s > worst:
            worst, wk = s, k
    return worst, wk


@pytest.mark.parametrize('shape', [(2, 12, 12), (2, 13, 14), (1, 27, 27), (1, 108, 108)])
def test_quadrant_nonlocal_against_fp64_and_bit_identical(shape):
    from sradsgan_amd import ops
    n, h, w = shape
    th, ph, g = (O.det_fill('nlq.%s' % k, (n, 8, h, w), 1.0) for k in 'tpg')
    dy = O.det_fill('nlq.dy', (n, 8, h, w), 1.0)
    runs = []
    for _ in range(2):
        a, b, c = (dev(t).requires_grad_() for t in (th, ph, g))
        y = ops.nonlocal_quadrants(a, b, c)
        y.backward(dev(dy))
        torch.cuda.synchronize()
        runs.append([t.detach().cpu() for t in (y, a.grad, b.grad, c.grad)])
    for p, q in zip(runs[0], runs[1]):
        assert torch.equal(p, q), 'rerun differs'
    a, b, c = (t.double().requires_grad_() for t in (th, ph, g))
    h1, w1 = h // 2, w // 2
    out = torch.zeros(n, 8, h, w, dtype=torch.float64)
    for rs in (slice(0, h1), slice(h1, h)):
        for cs in (slice(0, w1), slice(w1, w)):
            t = a[:, :, rs, cs].flatten(2).transpose(1, 2)
            k = b[:, :, rs, cs].flatten(2)
            v = c[:, :, rs, cs].flatten(2).transpose(1, 2)
            yq = torch.softmax(t @ k, -1) @ v
            out[:, :, rs, cs] = yq.transpose(1, 2).reshape(n, 8, rs.stop - rs.start, cs.stop - cs.start)
    out.backward(dy.double())
    errs = [rel_err(runs[0][0], out)] + [rel_err(runs[0][i + 1], t.grad) for i, t in enumerate((a, b, c))]
    print('nonlocal %s: y %.2e dtheta %.2e dphi %.2e dg %.2e' % ((shape,) + tuple(errs)))
    assert max(errs) < 1e-4


def test_gamma_residual_against_fp64_and_bit_identical():
    from sradsgan_amd import ops
    a, b, g = (O.det_fill('gr.%s' % k, (2, 64, 13, 14), 1.0) for k in 'abg')
    runs = []
    for _ in range(2):
        gam = torch.tensor([0.37], device=DEV, requires_grad=True)
        ad, bd = dev(a).requires_grad_(), dev(b).requires_grad_()
        out = ops.gamma_residual(ad, bd, gam)
        out.backward(dev(g))
        torch.cuda.synchronize()
        runs.append([t.detach().cpu() for t in (out, ad.grad, bd.grad, gam.grad)])
    for p, q in zip(runs[0], runs[1]):
        assert torch.equal(p, q)
    gam64 = torch.tensor([0.37], dtype=torch.float32).double().requires_grad_()
    b64 = b.double().requires_grad_()
    o64 = a.double() + gam64 * b64
    o64.backward(g.double())
    assert rel_err(runs[0][0], o64) < 1e-7 and torch.equal(runs[0][1], g)
    assert rel_err(runs[0][2], b64.grad) < 1e-7
    # dgamma is an fp32 sum of mixed-sign terms: its rounding error scales with sum |g b|, not with the (cancelling) sum itself
    scale = float((g.double() * b.double()).abs().sum())
    assert abs(float(runs[0][3]) - float(gam64.grad)) <= 1e-7 * scale


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('c', [320, 768])
def test_wide_channel_attention_against_fp64(mode, c):
    from sradsgan_amd import ops
    from sradsgan_amd.model.amssrn import CALayer
    ref = R.CA(c)
    O.det_init_(ref, prefix='ca%d.' % c)
    with torch.no_grad():
        ref.conv_du[1].weight.fill_(-0.2)
        ref.conv_du[0].weight.mul_(20.0)
        ref.conv_du[2].weight.mul_(20.0)
    hip = CALayer(c)
    hip.load_state_dict(ref.state_dict())
    hip.to(DEV)
    x = O.det_fill('ca.x%d' % c, (2, c, 13, 14), 1.0, 0.2)
    g = O.det_fill('ca.g%d' % c, (2, c, 13, 14), 1.0)
    xd = dev(x).requires_grad_()
    with ops.conv_math(mode):
        y = hip(xd)
        y.backward(dev(g))
    x64 = x.double().requires_grad_()
    r64 = ref.double()
    y64 = r64(x64)
    y64.backward(g.double())
    tol = 1e-5 if mode == 'fp32' else 5e-5
    assert rel_err(y, y64) < tol and rel_err(xd.grad, x64.grad) < tol
    for (k, p), (_, q) in zip(hip.named_parameters(), r64.named_parameters()):
        assert rel_err(p.grad, q.grad) < 10 * tol, k


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scale', SCALES)
def test_generator_matches_reference_vectors_and_fp64_gradients(mode, scale):
    from sradsgan_amd import ops
    g = golden(scale)
    ref = init_(R.Generator(scale))
    G = hip_model(scale, ref)
    x, t = inputs(scale)
    with ops.conv_math(mode):
        y = G(dev(x))
        l1 = ops.l1_mean(y, dev(t))
        mse = ops.mse_mean(y, dev(t))
        l1.backward()
    torch.cuda.synchronize()
    e_y = rel(O.digest(y, full_max=4096, nsample=4096), g['y'])
    print('amssrn x%d %s: output %.2e l1 %.2e mse %.2e' % (scale, mode, e_y, abs(l1.item() - float(g['l1'])), abs(mse.item() - float(g['mse']))))
    assert e_y < 1e-4
    assert abs(l1.item() - float(g['l1'])) < 1e-5 and abs(mse.item() - float(g['mse'])) < 1e-5
    r64 = ref.double()
    R.loss(r64(x.double()), t.double()).backward()
    score, k = grad_score(G, r64)
    print('amssrn x%d %s: worst gradient score %.2e (%s)' % (scale, mode, score, k))
    assert score < 2e-3
    assert rel(np.concatenate([digest(p.grad) for _, p in unique_params(G)]), g['grads']) < 2e-2


@pytest.mark.parametrize('mode', MODES)
def test_two_adam_iterations_match_reference(mode):
    from sradsgan_amd import ops
    from sradsgan_amd.model import amssrn as H
    g = golden(2)
    G = hip_model(2)
    x, t = inputs(2)
    opt = torch.optim.Adam(G.parameters(), lr=1e-4, betas=(0.9, 0.999))
    with ops.conv_math(mode):
        for it in range(2):
            loss = H.train_step(G, opt, dev(x), dev(t))
            assert abs(loss.item() - float(g['steps'][it])) < 1e-5
            assert rel(np.concatenate([digest(p.detach()) for _, p in unique_params(G)]), g['step%d' % it]) < 1e-4


def test_training_crop_against_fp64():
    """x4 at the training crop (54 -> 216; two images: the fp64 CPU restatement of the batch of 16 would take minutes)."""
    from sradsgan_amd import ops
    ref = init_(R.Generator(4))
    G = hip_model(4, ref)
    x = O.det_fill('amT.x', (2, 3, 54, 54), 0.5, 0.5)
    t = O.det_fill('amT.t', (2, 3, 216, 216), 0.5, 0.5)
    y = G(dev(x))
    ops.l1_mean(y, dev(t)).backward()
    torch.cuda.synchronize()
    r64 = ref.double()
    y64 = r64(x.double())
    R.loss(y64, t.double()).backward()
    e = rel_err(y, y64)
    score, k = grad_score(G, r64)
    print('amssrn training crop: output %.2e, worst gradient score %.2e (%s)' % (e, score, k))
    assert e < 1e-4 and score < 2e-3


def test_half_mode_forward():
    from sradsgan_amd import ops
    ref = init_(R.Generator(4))
    G = hip_model(4, ref)
    x = O.det_fill('amH.x', (2, 3, 54, 54), 0.5, 0.5)
    with ops.conv_math('half'), torch.no_grad():
        y = G(dev(x))
    with torch.no_grad():
        y64 = ref.double()(x.double())
    e = rel_err(y, y64)
    print('amssrn half mode forward: %.2e' % e)
    assert e < 5e-3
