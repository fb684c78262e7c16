"""HAT at its published widths on the HIP path (sradsgan_amd.model.hat with embed_dim 144 / 180 and window 16; csrc/hat_wide.hip) in
split-bf16 and exact-fp32 conv arithmetic: the generator against the reference's vectors (tests/golden/hat180_*.npz, hat144_x2.npz)
and its gradients against the fp64 restatement (tests/hat_ref.py configured by tests/hat_wide_ref.py); two train_step iterations
against the restatement plus Adam; a train-mode step with replayed drop-path factors; grad mode on and off give the same bits; and
the 96-channel generator, built after a 180-channel one in the same process, still gives its golden output.

The bars are tests/test_hat_gpu.py's own (test_generator_matches_reference_vectors_and_fp64_gradients: output 1e-4, losses 1e-5,
gradient score 2e-3, gradient digests 2e-2; test_two_train_steps_match_the_restatement_with_adam: losses 1e-5, parameters 1e-4;
test_train_mode_drop_path_replays_against_fp64: output 1e-4, gradient score 5e-3)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O
from tests import hat_ref as R
from tests import hat_wide_ref as W
from tests.test_hat_cpu import digest, rel, unique_names
from tests.test_hat_gpu import DEV, MODES, dev, grad_score, rel_err
from tests.test_hat_wide_cpu import build, golden

pytestmark = pytest.mark.gpu


def hip_model(ref, name, **kw):
    from sradsgan_amd.model import hat as H
    args = dict(depths=tuple(len(l.residual_group.blocks) for l in ref.layers), num_heads=(6,) * len(ref.layers), **W.model_kwargs(name))
    args.update(kw)
    M = H.GeneratorResNet(**args)
    M.load_state_dict(ref.state_dict(), strict=True)
    return M.to(DEV).eval()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(W.CASES))
def test_wide_generator_matches_reference_vectors_and_fp64_gradients(mode, name):
    """Each fixture at test_hat_gpu.py's bars.  On the MI355X, worst over the four fixtures, fp32 / bf16x3: output against fp64
    7.0e-7 / 2.3e-6, losses 3.0e-8, gradient digests 6.1e-6; gradient score 2.6e-6 except on hat180_x4, 1.88e-3 in both modes: one
    of the 196 608 inputs of the LeakyReLU after conv_before_upsample lies at 1.3e-6 (4e-7 of the largest), and the exact-fp32
    180-channel convolution, which both modes share, lands on the other side of zero than float64 does, which moves
    conv_before_upsample.0.weight's gradient by 5e-3 of its maximum and everything upstream by less.  The fp32 CPU restatement
    happens to keep the sign (its score there is 1.9e-6), so the 8 x rule would set a bar below the unchanged 2e-3, which holds."""
    from sradsgan_amd import ops
    g = golden(name)
    _, scale, shape, _ = W.CASES[name]
    ref = build(name)
    G = hip_model(ref, name)
    x, t = R.inputs(name, shape, scale, W.WS)
    with ops.conv_math(mode):
        y = G(dev(x))
        l1 = ops.l1_mean(y, dev(t))
        mse = ops.mse_mean(y, dev(t))
        l1.backward()
    torch.cuda.synchronize()
    sd = R.state(ref, torch.float64)
    y64 = R.forward(sd, x.double(), W.config(name))
    F.l1_loss(y64, t.double()).backward()
    e_y, e_64 = rel(O.digest(y, full_max=4096, nsample=4096), g['y']), rel_err(y, y64)
    print('%s %s: output %.2e against the fixture, %.2e against fp64, l1 %.2e mse %.2e' % (
        name, mode, e_y, e_64, abs(l1.item() - float(g['l1'])), abs(mse.item() - float(g['mse']))))
    score, k = grad_score(G, sd)
    hp = dict(G.named_parameters())
    e_g = rel(np.concatenate([digest(hp[k].grad) for k in unique_names(G)]), g['grads'])
    print('%s %s: worst gradient score %.2e (%s), gradient digests %.2e' % (name, mode, score, k, e_g))
    assert tuple(y.shape) == tuple(g['y_shape'])
    assert e_y < 1e-4 and e_64 < 1e-4
    assert abs(l1.item() - float(g['l1'])) < 1e-5 and abs(mse.item() - float(g['mse'])) < 1e-5
    assert score < 2e-3
    assert e_g < 2e-2


STEPS_INPUT = ('hat180_x4.steps.5', (1, 3, 16, 32))
KINK_MARGIN = 4e-6


def test_two_train_steps_match_the_restatement_with_adam():
    """hat180_x4's network, two L1 / Adam iterations at test_hat_gpu.py's bars (losses 1e-5, parameters 1e-4).

    Adam's first steps move every parameter by lr * sign(g), so the comparison with fp64 means something only where the fp64
    trajectory is differentiable within fp32 rounding of the point: no input of the LeakyReLU after conv_before_upsample (a sum of
    1620 products, worst-case fp32 error 1620 * 2^-24 * 0.02 = 2e-6, 6e-7 of its maximum) and no |output - target| of the L1 loss
    (output error 5e-7) within KINK_MARGIN = 4e-6 of its kink.  The fixtures' own inputs do not keep that distance (hat180_x4: a
    pre-activation at 4e-7 of the maximum, on whose sign exact-fp32 convolutions in two summation orders disagree, which moves
    conv_before_upsample.0.weight's gradient by 5e-3 and Adam's parameters by 2e-2), so the test draws its own input, the same
    deterministic filler under another tag, and asserts the distance on the fp64 side before it compares anything.  The tag was
    chosen for that distance, on the CPU, from eight tags at (1, 3, 16, 32) and eight at (1, 3, 32, 32): it is the one whose fp64
    two-step run stays farthest from both kinks (8.1e-6; the others 2e-7 to 4e-6), not a draw like any other."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    name = 'hat180_x4'
    scale = W.CASES[name][1]
    tag, shape = STEPS_INPUT
    ref = build(name)
    G = hip_model(ref, name)
    x, t = R.inputs(tag, shape, scale, W.WS)
    opt = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.99))
    sd = R.state(ref, torch.float64)
    names = unique_names(G)
    opt64 = torch.optim.Adam([sd[k] for k in names], lr=2e-4, betas=(0.9, 0.99))
    cfg = W.config(name)
    pre = []

    class SpyF:
        """torch.nn.functional as tests/hat_ref.py sees it, with a leaky_relu that keeps its input (torch's module is untouched)"""

        def __getattr__(self, k):
            return getattr(F, k)

        @staticmethod
        def leaky_relu(a, s):
            pre.append(a.detach())
            return F.leaky_relu(a, s)
    R.F = SpyF()
    try:
        for it in range(2):
            with ops.conv_math('fp32'):
                loss = H.train_step(G, opt, dev(x), dev(t))
            opt64.zero_grad()
            y64 = R.forward(sd, x.double(), cfg)
            l64 = F.l1_loss(y64, t.double())
            l64.backward()
            opt64.step()
            torch.cuda.synchronize()
            margin = min(float(pre[-1].abs().min() / pre[-1].abs().max()), float((y64 - t.double()).abs().min()))
            print('hat180 two steps: step %d loss %.6f (fp64 %.6f), distance from the nearest kink %.2e' % (it, loss.item(), l64.item(), margin))
            assert margin > KINK_MARGIN
            assert loss.dim() == 0 and loss.is_cuda
            assert abs(loss.item() - l64.item()) < 1e-5, (it, loss.item(), l64.item())
    finally:
        R.F = F
    hp = dict(G.named_parameters())
    worst = max(rel_err(hp[k], sd[k]) for k in names)
    print('hat180 two steps: worst parameter rel err %.2e' % worst)
    assert worst < 1e-4


def test_train_mode_drop_path_replays_against_fp64():
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    name = 'hat144_x2'
    ref = R.init_(H.GeneratorResNet(depths=(4, 4), num_heads=(6, 6), drop_path_rate=0.5, **W.model_kwargs(name)))
    G = hip_model(ref, name, drop_path_rate=0.5)
    G.train()
    x = O.det_fill('hatw.dp.x', (4, 3, 32, 32), 0.5, 0.5)
    r = O.det_fill('hatw.dp.r', (4, 3, 64, 64), 1.0)
    torch.manual_seed(3)
    with ops.conv_math('fp32'):
        y = G(dev(x))
        (y * dev(r)).sum().backward()
    factors = {i: tuple(None if f is None else f.cpu() for f in hab.last_drop_factors) for i, hab in enumerate(G.habs)}
    drawn = torch.cat([f for fs in factors.values() for f in fs if f is not None])
    assert (drawn == 0).any() and (drawn > 1).any()
    assert factors[0] == (None, None)
    sd = R.state(ref, torch.float64)
    y64 = R.forward(sd, x.double(), W.config(name, (4, 4)), factors=factors)
    (y64 * r.double()).sum().backward()
    score, k = grad_score(G, sd)
    print('hat144 train-mode drop path: output %.2e, gradient score %.2e (%s)' % (rel_err(y, y64), score, k))
    assert rel_err(y, y64) < 1e-4 and score < 5e-3
    for hab in G.habs:
        hab.replay_drop_factors = tuple(None if f is None else f.to(DEV) for f in hab.last_drop_factors)
    with torch.no_grad(), ops.conv_math('fp32'):
        y2 = G(dev(x))
    assert torch.equal(y.detach(), y2)


@pytest.mark.parametrize('mode', MODES)
def test_grad_mode_on_and_off_give_the_same_bits(mode):
    from sradsgan_amd import ops
    name = 'hat180_x3'
    _, scale, shape, _ = W.CASES[name]
    G = hip_model(build(name), name)
    x, _ = R.inputs(name, shape, scale, W.WS)
    with ops.conv_math(mode):
        y_on = G(dev(x))
        with torch.no_grad():
            y_off = G(dev(x))
    torch.cuda.synchronize()
    assert y_on.requires_grad and not y_off.requires_grad
    assert torch.equal(y_on.detach(), y_off)


def test_the_96_channel_generator_after_a_180_channel_one_keeps_its_golden_output():
    """The dispatch by width holds no state: a 180-channel forward and backward, then the reference family's x4 fixture at its
    own bars (tests/test_hat_gpu.py), then the 180-channel forward again, bit for bit."""
    from sradsgan_amd import ops
    from tests import test_hat_cpu as N
    from tests.test_hat_gpu import hip_model as narrow_model
    wide = 'hat180_x3'
    _, scale, shape, _ = W.CASES[wide]
    Gw = hip_model(build(wide), wide)
    xw, tw = R.inputs(wide, shape, scale, W.WS)
    with ops.conv_math('fp32'):
        yw = Gw(dev(xw))
        ops.l1_mean(yw, dev(tw)).backward()
    g = N.golden('x4')
    nscale, nws, nshape = N.CASES['x4']
    Gn = narrow_model(N.build('x4'))
    x, t = R.inputs('x4', nshape, nscale, nws)
    with ops.conv_math('fp32'):
        y = Gn(dev(x))
        l1 = ops.l1_mean(y, dev(t))
        l1.backward()
        with torch.no_grad():
            yw2 = Gw(dev(xw))
    torch.cuda.synchronize()
    assert rel(O.digest(y, full_max=4096, nsample=4096), g['y']) < 1e-4
    assert abs(l1.item() - float(g['l1'])) < 1e-5
    hp = dict(Gn.named_parameters())
    assert rel(np.concatenate([digest(hp[k].grad) for k in unique_names(Gn)]), g['grads']) < 2e-2
    assert torch.equal(yw.detach(), yw2)


def test_whole_scene_tiling_takes_the_wide_generator():
    """scene.super_resolve_scene only calls generator(x): a scene of one 32 x 32 tile equals the generator on it, quantised as
    tests/test_scene_gpu.py::test_scene_equal_to_one_tile does, and a 40 x 56 scene in overlapping 32-pixel tiles comes back whole."""
    from sradsgan_amd import data, scene as S
    name = 'hat144_x2'
    G = hip_model(build(name), name)
    gen = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (32, 32, 3), generator=gen, dtype=torch.uint8)
    out = S.super_resolve_scene(G, u8, 2, 32, 8)
    with torch.no_grad():
        want = (G(data.to_tensor(u8.to(DEV)[None]))[0] * 255.0).clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (64, 64, 3)
    assert torch.equal(out, want)
    big = torch.randint(0, 256, (40, 56, 3), generator=gen, dtype=torch.uint8)
    assert tuple(S.super_resolve_scene(G, big, 2, 32, 8).shape) == (80, 112, 3)
