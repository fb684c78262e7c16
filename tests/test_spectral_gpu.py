"""Spectral normalisation on the HIP path: the batched power iteration and projection kernels (csrc/sn.hip) against fp64; the spectral
patch discriminator's forward, backward and gradient penalty, and (u, v, sigma) after each of four passes, against the numbers recorded
from the reference (tests/golden/disc_spectral.npz); one TrainStep iteration per recorded case; the trainer with a checkpoint round trip."""
import types

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import disc_norms_ref as DR
from tests import gan_options_ref as GR
from tests import spectral_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR = 1e-4
SHAPES = [(1, 9), (5, 27), (64, 27), (64, 576), (512, 4608)]
D_SHAPES = [(64, 27), (64, 576), (128, 576), (128, 1152), (256, 1152), (256, 2304), (512, 2304), (512, 4608)]


def _layer(cout, k, seed):
    g = torch.Generator().manual_seed(100 * seed + cout + k)
    w = (torch.randn(cout, k, generator=g) * 0.02).to(DEV)
    u, v = SR.l2normalize(torch.randn(cout, generator=g)).to(DEV), SR.l2normalize(torch.randn(k, generator=g)).to(DEV)
    return w, u, v


def _power(w, u, v):
    """One power iteration, sigma and the scaled weight with torch ops in the dtype of the arguments."""
    v = SR.l2normalize(w.t() @ u)
    s = w @ v
    u = SR.l2normalize(s)
    sigma = torch.dot(u, w @ v)
    return u, v, sigma, w / sigma


def _bar(what, kernel, restated, exact, bad):
    """The kernel's error against fp64 is at most 4 x the error of torch's own fp32 restatement on this device, floor 1e-6 relative."""
    exact = exact.double()
    scale = max(float(exact.abs().max()), 1e-30)
    ek, et = float((kernel.double() - exact).abs().max()) / scale, float((restated.double() - exact).abs().max()) / scale
    print('%-34s kernel %.3e  torch fp32 %.3e  ratio %.2f' % (what, ek, et, ek / max(et, 1e-30)))
    if not ek <= max(4 * et, 1e-6):
        bad.append((what, ek, et))


def _run_table(layers):
    from sradsgan_amd import ops
    table = ops.SpectralTable(layers)
    out, ws = table.forward()
    return table, out, ws


@pytest.mark.parametrize('together', [False, True], ids=['alone', 'one_table'])
def test_power_iteration_against_fp64(together):
    layers = [_layer(c, k, 1) for c, k in SHAPES]
    start = [tuple(t.clone() for t in l) for l in layers]
    if together:
        table, out, ws = _run_table(layers)
        got = [(ws[i], table.sigmas(out)[i]) for i in range(len(layers))]
    else:
        got = []
        for l in layers:
            table, out, ws = _run_table([l])
            got.append((ws[0], table.sigmas(out)[0]))
    torch.cuda.synchronize()
    bad = []
    for (c, k), (w, u, v), (w0, u0, v0), (weff, sigma) in zip(SHAPES, layers, start, got):
        assert torch.equal(w, w0) and not torch.equal(v, v0)                                  # in place, through the parameter
        assert not torch.equal(u, u0) or c == 1                                                # (a unit vector of one entry stays +-1)
        eu, ev, es, ew = _power(w0.double(), u0.double(), v0.double())
        tu, tv, ts, tw = _power(w0, u0, v0)
        for what, a, b, e in (('u', u, tu, eu), ('v', v, tv, ev), ('sigma', sigma, ts, es), ('W', weff, tw, ew)):
            _bar('(%d, %d) %s' % (c, k, what), a, b, e, bad)
        su, sv, ss = table.snapshot(out, len(layers) - 1 if together else 0) if (c, k) == SHAPES[-1] else (None, None, None)
        if su is not None:                                                                     # the pass's snapshot = the parameters now
            assert torch.equal(su, u) and torch.equal(sv, v) and torch.equal(ss, sigma)
    assert not bad, bad


def test_a_layer_does_not_depend_on_the_table_and_calls_repeat():
    for c, k in SHAPES:
        runs = []
        for others in (False, True, True):
            mine = _layer(c, k, 2)
            layers = ([_layer(cc, kk, 3) for cc, kk in D_SHAPES[:5]] + [mine] + [_layer(cc, kk, 4) for cc, kk in D_SHAPES[5:7]]) if others else [mine]
            table, out, ws = _run_table(layers)
            i = 5 if others else 0
            runs.append((mine[1].clone(), mine[2].clone(), table.sigmas(out)[i].clone(), ws[i].clone()))
        torch.cuda.synchronize()
        for a, b in ((runs[0], runs[1]), (runs[1], runs[2])):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (c, k)


@pytest.mark.parametrize('together', [False, True], ids=['alone', 'one_table'])
def test_projection_against_fp64(together):
    layers = [_layer(c, k, 5) for c, k in SHAPES]
    gen = torch.Generator().manual_seed(77)
    grads = [torch.randn(c, k, generator=gen).to(DEV) for c, k in SHAPES]
    slots0 = [torch.randn(c, k, generator=gen).to(DEV) for c, k in SHAPES]                    # accumulation into a non-zero slot
    slots = [s.clone() for s in slots0]
    snaps = []
    if together:
        table, out, _ = _run_table(layers)
        skipped = 1                                                                            # a layer without a gradient is left alone
        table.backward(out, [g if i != skipped else None for i, g in enumerate(grads)], slots)
        snaps = [table.snapshot(out, i) for i in range(len(layers))]
    else:
        skipped = None
        for i, l in enumerate(layers):
            table, out, _ = _run_table([l])
            table.backward(out, [grads[i]], [slots[i]])
            snaps.append(table.snapshot(out, 0))
    torch.cuda.synchronize()
    bad = []
    for i, ((c, k), (w, _, _), g, s0, s, (u, v, sigma)) in enumerate(zip(SHAPES, layers, grads, slots0, slots, snaps)):
        if i == skipped:
            assert torch.equal(s, s0)
            continue
        proj = lambda w, g, u, v, sg, s0: s0 + (g / sg - (g * w).sum() / (sg * sg) * torch.outer(u, v))      # noqa: E731
        exact = proj(w.double(), g.double(), u.double(), v.double(), sigma.double(), s0.double())
        _bar('(%d, %d) weight_bar gradient' % (c, k), s, proj(w, g, u, v, sigma, s0), exact, bad)
        assert float((s - s0).abs().max()) > 1e-2                                              # something was added
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------- #
def _pair(g, norm_type, attention):
    from sradsgan_amd.model import SpectralPatchDiscriminator
    name = SR.tag(norm_type, attention)
    suffix = int(g[name + '.suffix'])
    od = SR.fill_(SR.Discriminator(norm_type=norm_type, attention=attention), suffix, float(g[name + '.conv_scale']))
    hd = SpectralPatchDiscriminator(norm_type=norm_type, attention=attention)
    hd.load_state_dict(od.state_dict(), strict=True)
    return hd.to(DEV), od, SR.inputs(suffix), name


def _zero_grad_keys(hd):
    """Biases of the convs that feed an instance or batch norm: the mean subtraction cancels them, their gradient is identically zero
    and every platform sees only the roundoff of a cancelling sum (tests/test_disc_norms_gpu.py, for the same reason)."""
    if hd.norm_type not in ('instance', 'batch'):
        return ()
    return tuple('model.%d.module.bias' % conv_i for conv_i, norm_i, _ in hd._blocks if norm_i is not None)


def _check(table, what, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), FLOOR)
    print('%-46s err %.3e  scale %.3e  ratio %.3e (bar %.0e)' % (what, err, scale, err / scale, tol))
    if not (got.shape == want.shape and err <= tol * scale):
        table.append((what, err, scale))


def _grads_against(table, hd, recorded, names, tol, what):
    hp, zero, at = SR.trainable(hd), _zero_grad_keys(hd), 0
    assert list(hp) == names
    for k in names:
        d = DR.digest(hp[k].grad)
        want = recorded[at:at + d.size]
        at += d.size
        if k in zero:
            scale = float(hp[k.replace('bias', 'weight_bar')].grad.abs().max())
            err = float(hp[k].grad.abs().max())
            print('%-46s |roundoff| %.3e vs weight-gradient scale %.3e' % (what + ' ' + k + ' (zero)', err, scale))
            if not err <= tol * scale:
                table.append((what, k, err, scale))
            continue
        _check(table, what + ' ' + k, d, want, tol)
    assert at == recorded.size


def _state_against(table, hd, g, name, i):
    """(u, v, sigma) after pass i within 1e-5 (absolute: entries of unit vectors; sigma relative, per layer) of the recorded values; sigma both as
    the kernel left it in the pass buffer and recomputed from the parameters."""
    u, v, s = SR.state_after_pass(hd)
    for what, got, want in (('u', u, g['%s.u%d' % (name, i)]), ('v', v, g['%s.v%d' % (name, i)])):
        err = float(np.abs(got - want).max())
        print('%-46s err %.3e (bar 1e-05)' % ('pass %d %s' % (i, what), err))
        if not (got.shape == want.shape and err <= 1e-5):
            table.append(('pass %d' % i, what, err))
    want = np.asarray(g['%s.sigma%d' % (name, i)], dtype=np.float64)
    for what, got in (('parameters', s), ('pass buffer', hd._table.sigmas().cpu().double().numpy())):
        err = np.abs(np.asarray(got, dtype=np.float64) - want) / np.abs(want)                  # per layer: the sigmas span a decade
        print('%-46s worst layer %.3e (bar 1e-05)' % ('pass %d sigma (%s)' % (i, what), float(err.max())))
        if not (err.shape == (8,) and bool((err <= 1e-5).all())):
            table.append(('pass %d sigma' % i, what, err.tolist()))


@pytest.mark.parametrize('math', ['bf16x3', 'fp32'])
@pytest.mark.parametrize('norm_type,attention', SR.NUMBERED, ids=[SR.tag(*v) for v in SR.NUMBERED])
def test_forward_backward_penalty_and_four_passes_against_the_reference(golden, norm_type, attention, math):
    """tests/spectral_ref.run's sequence on the HIP discriminator: y 1e-3, d img 2e-3, gradients 2e-3, gp 1e-4, gp gradients 5e-3 (the
    bars of tests/test_disc_norms_gpu.py); u, v, sigma after each pass 1e-5 -- passes 3 and 4 run under no_grad (4 in eval mode)."""
    from sradsgan_amd import ops
    from sradsgan_amd.train_step import TrainStep
    g = golden('disc_spectral')
    hd, _, t, name = _pair(g, norm_type, attention)
    names, bad = g[name + '.names'].tolist(), []
    packs0 = dict(ops.eff_pack_stats)
    with ops.conv_math(math):
        x = t['img'].to(DEV).requires_grad_(True)
        y = hd(x)
        _state_against(bad, hd, g, name, 1)
        y.backward(t['dy'].to(DEV))
        _check(bad, 'y', y.detach().cpu().numpy().ravel(), g[name + '.y'], 1e-3)
        _check(bad, 'd img', O.digest(x.grad), g[name + '.dx'], 2e-3)
        _grads_against(bad, hd, g[name + '.grads'], names, 2e-3, 'grad')
        assert all(p.grad is None for k, p in hd.named_parameters() if k.endswith(('weight_u', 'weight_v')))
        hd.zero_grad()
        step = TrainStep(torch.nn.Linear(1, 1).to(DEV), hd, torch.nn.Linear(1, 1).to(DEV))
        gp = step.gradient_penalty(t['real'].to(DEV), t['fake'].to(DEV), torch.from_numpy(g['alpha']).to(DEV))
        _state_against(bad, hd, g, name, 2)
        gp.backward()
        print('%-46s got %.7f recorded %.7f' % ('gp', gp.item(), float(g[name + '.gp'])))
        if not abs(gp.item() - float(g[name + '.gp'])) < 1e-4:
            bad.append(('gp', gp.item(), float(g[name + '.gp'])))
        _grads_against(bad, hd, g[name + '.gp_grads'], names, 5e-3, 'gp grad')
        with torch.no_grad():
            hd(t['real'].to(DEV))
            _state_against(bad, hd, g, name, 3)
            hd.eval()
            hd(t['fake'].to(DEV))
            hd.train()
            _state_against(bad, hd, g, name, 4)
    torch.cuda.synchronize()
    # an effective weight is packed once per mode and pass: forward operand in all 4 passes, data-gradient operand in passes 1 and 2;
    # each of the penalty's two second-order passes finds the image of every layer again: 2 x 8 lookups, none of them a pack
    packed, reused = ops.eff_pack_stats['packed'] - packs0['packed'], ops.eff_pack_stats['reused'] - packs0['reused']
    print('effective-weight images packed %d, found again %d' % (packed, reused))
    assert packed == 8 * (4 + 2) and reused == 2 * 8
    assert not bad, (name, math, bad)


# ------------------------------------------------------------------------------------------------------------------------- #
def _nets(g):
    from sradsgan_amd import model as M
    og = O.det_init_(O.GeneratorResNet(O.ResGroup, n_residual_blocks=2, n_basic_blocks=1, upscale_factor=4), prefix='G.')
    of = O.det_init_(O.FeatureExtractor(), prefix='F.')
    hg = M.GeneratorResNet(M.ResGroup, n_residual_blocks=2, n_basic_blocks=1, upscale_factor=4)
    hf = M.FeatureExtractor()
    hg.load_state_dict(og.state_dict(), strict=True), hf.load_state_dict(of.state_dict(), strict=True)
    hd, _, _, _ = _pair(g, '', True)
    return hg.to(DEV), hd, hf.to(DEV)


@pytest.mark.parametrize('case', list(SR.TRAIN_CASES))
def test_one_training_iteration_against_the_recorded_one(golden, case):
    """train_small's shapes, the '' + attention spectral D, against the iteration recorded on the reference's modules: scalars 1e-3,
    G gradients 5e-3, D gradients 2e-2 (train_small's bars), post-step u / v 1e-5 of the recorded post-clamp values; the gradient and
    Adam moment slots of u / v exactly zero; reuse_d_fake=True passed in changes nothing; twice from the same state is bit-identical."""
    from sradsgan_amd.train_step import TrainStep
    g, name = golden('disc_spectral'), SR.tag('', True)
    key = '%s.it_%s' % (name, case)
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    alpha = torch.from_numpy(g['train_alpha'])
    runs = []
    for reuse in (True, True, False):
        hg, hd, hf = _nets(g)
        step = TrainStep(hg, hd, hf, reuse_d_fake=reuse, **SR.TRAIN_CASES[case])
        got = step(lr_img.to(DEV), hr_img.to(DEV), alpha.to(DEV))
        torch.cuda.synchronize()
        runs.append(([float(got[k]) for k in GR.SCALARS], step.arena_G.flat_g.clone(), step.arena_D.flat_g.clone(), step.arena_D.flat_p.clone()))
    for other in runs[1:]:
        assert runs[0][0] == other[0] and all(torch.equal(a, b) for a, b in zip(runs[0][1:], other[1:]))
    worst = float(np.abs(np.array(runs[0][0]) - g[key + '_scalars']).max())
    rec = lambda net: [g['%s_%s_%s' % (key, net, k)] for k in ('names', 'grads', 'counts', 'maxabs')]        # noqa: E731
    sg, wg = GR.digest_score(hg, *rec('G'))
    trainable = types.SimpleNamespace(named_parameters=lambda: list(SR.trainable(hd).items()))      # (the reference's u / v have no .grad)
    sd, wd = GR.digest_score(trainable, *rec('D'))
    u, v = SR.clamp_uv(hd)
    eu, ev = float(np.abs(u - g[key + '_u']).max()), float(np.abs(v - g[key + '_v']).max())
    print('%s: scalars %.3e  G gradient %.3e (%s)  D gradient %.3e (%s)  post-step u %.3e v %.3e  gp %.6f'
          % (case, worst, sg, wg, sd, wd, eu, ev, runs[0][0][5]))
    assert worst < 1e-3 and sg < 5e-3 and sd < 2e-2 and eu <= 1e-5 and ev <= 1e-5
    arena = step.arena_D
    off = {id(p): o for p, o in zip(arena.params, arena.offsets)}
    n_uv = 0
    for k, p in hd.named_parameters():
        if k.endswith(('weight_u', 'weight_v')):
            n_uv += 1
            lo, hi = off[id(p)], off[id(p)] + p.numel()
            assert not p.requires_grad and float(p.detach().abs().max()) <= 0.01                     # clamped like every D parameter
            for buf in (arena.flat_g, arena.exp_avg, arena.exp_avg_sq):
                assert not bool(buf[lo:hi].any()), k
    assert n_uv == 16 and arena.check_views()


def test_trainer_runs_and_checkpoints_restore_u_and_v(tmp_path):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import SpectralPatchDiscriminator
    gen = torch.Generator().manual_seed(21)
    train = [torch.randint(0, 256, (2, 32, 32, 3), generator=gen, dtype=torch.uint8) for _ in range(2)]
    hr = torch.rand(2, 3, 32, 32, generator=gen)
    test = [(torch.nn.functional.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]
    args = T.default_args(scale_factor=4, num_epochs=1, batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32, hr_width=32,
                          sample_interval=1, n_residual_blocks=1, n_basic_blocks=1, d_spectralnorm=True, d_norm_type='', d_attention=True)
    net = T.SRADSGAN(args, train_loader=train, test_loader=test)
    hist = net.train()                                                                         # one epoch of two steps
    assert type(net.discriminator) is SpectralPatchDiscriminator and net.step._spectral
    assert len(hist) == 1 and bool(torch.isfinite(torch.tensor([hist[0]['loss_G'], hist[0]['loss_D']])).all())
    net2 = T.SRADSGAN(T.default_args(**dict(vars(args), epoch=1)), train_loader=train, test_loader=test)
    net2._build()
    a, b = net.discriminator.state_dict(), net2.discriminator.state_dict()
    assert list(a) == list(b) and sum(k.endswith(('weight_u', 'weight_v')) for k in a) == 16
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    uv = torch.cat([a[k].flatten() for k in a if k.endswith('weight_u')])
    assert float(uv.abs().max()) <= 0.01 and float(uv.abs().max()) > 0                        # they took part in the steps: clamped
