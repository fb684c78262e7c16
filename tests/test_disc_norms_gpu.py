"""PatchDiscriminator (norm_type '' | 'instance' | 'group', with and without the attention pair) on the HIP path, in the default
conv arithmetic and in exact fp32: forward, backward and TrainStep.gradient_penalty against the numbers recorded from the reference
(tests/golden/disc_norms.npz) under the bars tests/test_model_gpu.py holds the BatchNorm discriminator to; one TrainStep iteration
per variant against the recorded iteration under train_small's bars; the host orders of TrainStep; batch independence of D."""
import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import disc_norms_ref as DR
from tests import gan_options_ref as GR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR = 1e-4
IDS = [DR.tag(*v) for v in DR.VARIANTS]


def _pair(g, norm_type, attention):
    from sradsgan_amd.model import PatchDiscriminator
    name = DR.tag(norm_type, attention)
    suffix = int(g[name + '.suffix'])
    od = DR.fill_(DR.Discriminator(norm_type=norm_type, attention=attention), suffix, float(g[name + '.conv_scale']))
    hd = PatchDiscriminator(norm_type=norm_type, attention=attention)
    hd.load_state_dict(od.state_dict(), strict=True)
    return hd.to(DEV), od, DR.inputs(suffix), name


def _zero_grad_keys(hd):
    """Biases of the convs that feed an instance norm: the mean subtraction cancels them, their gradient is identically zero and
    every platform sees only the roundoff of a cancelling sum (tests/parity_util.ZERO_GRAD_KEYS, for the same reason)."""
    if hd.norm_type != 'instance':
        return ()
    return tuple('model.%d.bias' % conv_i for conv_i, norm_i, _ in hd._blocks if norm_i is not None)


def _check(table, what, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), FLOOR)
    print('%-40s err %.3e  scale %.3e  ratio %.3e (bar %.0e)' % (what, err, scale, err / scale, tol))
    if not err <= tol * scale:
        table.append((what, err, scale))


def _grads_against(table, hd, recorded, names, tol, what):
    """recorded: the concatenated DR.digest of every parameter gradient in named_parameters() order."""
    hp, zero, at = dict(hd.named_parameters()), _zero_grad_keys(hd), 0
    assert list(hp) == names
    for k in names:
        d = DR.digest(hp[k].grad)
        want = recorded[at:at + d.size]
        at += d.size
        if k in zero:
            scale = float(hp[k.replace('bias', 'weight')].grad.abs().max())
            err = float(hp[k].grad.abs().max())
            print('%-40s |roundoff| %.3e vs weight-gradient scale %.3e' % (what + ' ' + k + ' (zero)', err, scale))
            if not err <= tol * scale:
                table.append((what, k, err, scale))
            continue
        _check(table, what + ' ' + k, d, want, tol)
    assert at == recorded.size


@pytest.mark.parametrize('math', ['bf16x3', 'fp32'])
@pytest.mark.parametrize('norm_type,attention', DR.VARIANTS, ids=IDS)
def test_forward_backward_and_penalty_against_the_reference(golden, norm_type, attention, math):
    from sradsgan_amd import ops
    from sradsgan_amd.train_step import TrainStep
    g = golden('disc_norms')
    hd, _, t, name = _pair(g, norm_type, attention)
    names, bad = g[name + '.names'].tolist(), []
    with ops.conv_math(math):
        x = t['img'].to(DEV).requires_grad_(True)
        y = hd(x)
        y.backward(t['dy'].to(DEV))
        _check(bad, 'y', y.detach().cpu().numpy().ravel(), g[name + '.y'], 1e-3)
        _check(bad, 'd img', O.digest(x.grad), g[name + '.dx'], 2e-3)
        _grads_against(bad, hd, g[name + '.grads'], names, 2e-3, 'grad')
        hd.zero_grad()
        step = TrainStep(torch.nn.Linear(1, 1).to(DEV), hd, torch.nn.Linear(1, 1).to(DEV))
        gp = step.gradient_penalty(t['real'].to(DEV), t['fake'].to(DEV), torch.from_numpy(g['alpha']).to(DEV))
        gp.backward()
        print('%-40s got %.7f recorded %.7f' % ('gp', gp.item(), float(g[name + '.gp'])))
        if not abs(gp.item() - float(g[name + '.gp'])) < 1e-4:
            bad.append(('gp', gp.item(), float(g[name + '.gp'])))
        _grads_against(bad, hd, g[name + '.gp_grads'], names, 5e-3, 'gp grad')
    torch.cuda.synchronize()
    assert not bad, (name, math, bad)


def _nets(g, norm_type):
    from sradsgan_amd import model as M
    og = O.det_init_(O.GeneratorResNet(O.ResGroup, n_residual_blocks=2, n_basic_blocks=1, upscale_factor=4), prefix='G.')
    of = O.det_init_(O.FeatureExtractor(), prefix='F.')
    hg = M.GeneratorResNet(M.ResGroup, n_residual_blocks=2, n_basic_blocks=1, upscale_factor=4)
    hf = M.FeatureExtractor()
    hg.load_state_dict(og.state_dict(), strict=True), hf.load_state_dict(of.state_dict(), strict=True)
    hd, od, _, _ = _pair(g, norm_type, True)
    return (hg.to(DEV), hd, hf.to(DEV)), (og, od, of)


def _batch(g):
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    return lr_img, hr_img, torch.from_numpy(g['train_alpha'])


@pytest.mark.parametrize('norm_type', DR.NORM_TYPES, ids=['none', 'instance', 'group'])
def test_one_training_iteration_against_the_recorded_one_and_twice(golden, norm_type):
    """train_small's shapes (x4, 2 groups x 1 RAB, batch 2, LR 8 -> HR 32), D with the attention pair, against the iteration recorded
    on the reference's modules: the logged scalars within 1e-3, generator gradients 5e-3, discriminator gradients 2e-2 (train_small's
    bars, gan_options_ref.digest_score's measure); the same iteration from the same weights a second time is bit-identical."""
    from sradsgan_amd.train_step import TrainStep
    g, name = golden('disc_norms'), DR.tag(norm_type, True)
    lr_img, hr_img, alpha = _batch(g)
    runs = []
    for rep in range(2):
        (hg, hd, hf), _ = _nets(g, norm_type)
        step = TrainStep(hg, hd, hf)
        got = step(lr_img.to(DEV), hr_img.to(DEV), alpha.to(DEV))
        torch.cuda.synchronize()
        runs.append(([float(got[k]) for k in GR.SCALARS], step.arena_G.flat_g.clone(), step.arena_D.flat_g.clone(), step.arena_D.flat_p.clone()))
    worst = float(np.abs(np.array(runs[1][0]) - g[name + '.it_scalars']).max())
    rec = lambda net: [g['%s.it_%s_%s' % (name, net, k)] for k in ('names', 'grads', 'counts', 'maxabs')]        # noqa: E731
    zero = _zero_grad_keys(hd)
    sg, wg = GR.digest_score(hg, *rec('G'))
    sd, wd = GR.digest_score(hd, *rec('D'), skip=zero)
    hp, net_scale, sz = dict(hd.named_parameters()), float(np.max(g[name + '.it_D_maxabs'])), 0.0
    for k in zero:                                   # identically zero: against zero, on the scale of that conv's weight gradient
        scale = max(float(hp[k.replace('bias', 'weight')].grad.abs().max()), 1e-2 * net_scale)
        sz = max(sz, float(hp[k].grad.abs().max()) / scale)
    print('%s: scalars %.3e  G gradient %.3e (%s)  D gradient %.3e (%s)  zero-gradient biases %.3e  gp %.6f'
          % (name, worst, sg, wg, sd, wd, sz, runs[1][0][5]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    assert worst < 1e-3 and sg < 5e-3 and sd < 2e-2 and sz < 2e-2


@pytest.mark.parametrize('norm_type', DR.NORM_TYPES, ids=['none', 'instance', 'group'])
def test_reusing_d_of_the_fake_batch_gives_the_same_gradients(golden, norm_type):
    """reuse_d_fake (the one-walk backward) against reuse_d_fake=False (every pass of the reference run): the same sums in another
    association.  The adversarial cotangent is scaled once at d gen_hr (the one-walk multiplication) instead of at the loss and
    carried through D's ~30 layers, and D's arena receives its real, fake and penalty terms in another order; each costs a few fp32
    roundings (2^-24 = 6e-8) of the ADDENDS, and D's gradient is a difference of real and fake terms that may be ten to a hundred
    times its own size.  Bar: 1e-4 of each arena's largest entry -- 6e-8 x a few roundings x that cancellation, with a decade to
    spare; a pass too few or too many, or a term taken twice, moves an arena by O(1) of its scale."""
    from sradsgan_amd.train_step import TrainStep
    g = golden('disc_norms')
    lr_img, hr_img, alpha = _batch(g)
    arenas = {}
    for reuse in (True, False):
        (hg, hd, hf), _ = _nets(g, norm_type)
        step = TrainStep(hg, hd, hf, reuse_d_fake=reuse)
        step(lr_img.to(DEV), hr_img.to(DEV), alpha.to(DEV))
        torch.cuda.synchronize()
        arenas[reuse] = (step.arena_G.flat_g.double().cpu(), step.arena_D.flat_g.double().cpu())
    for which, a, b in zip('GD', arenas[True], arenas[False]):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print('%s arena %s: max diff %.3e of %.3e (%.3e)' % (norm_type or 'none', which, err, scale, err / scale))
        assert scale > 0 and err <= 1e-4 * scale


def test_d_of_a_sample_does_not_depend_on_the_batch(golden):
    """What a per-sample norm is for: D(x)[i] with 'instance' and 'group' is bit-identical whatever else is in the batch."""
    g = golden('disc_norms')
    for norm_type in ('instance', 'group'):
        hd, _, t, _ = _pair(g, norm_type, False)
        with torch.no_grad():
            both = hd(t['img'].to(DEV))
            swapped = hd(torch.stack([t['img'][0], t['real'][1]]).to(DEV))
        assert torch.equal(both[0], swapped[0]) and not torch.equal(both[1], swapped[1])
