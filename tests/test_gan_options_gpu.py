"""The four loss options on the device: srhip_gp_penalty_{fwd,bwd} against fp64 for all six (norm, penalty) pairs, the penalty through
the discriminator and one training step per recorded case against tests/golden/gan_options.npz (recorded from the reference by
tools/make_golden_gan_options.py), the relativistic step against the plain one, and the trainers built with the options.

Kernel comparisons use reduction_ref.err / bound (8 x the error of stock fp32 torch on the CPU, floor 32 * 2^-24) and print
`err torch-fp32-err bound` per output before asserting, like test_reductions_gpu.py."""
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import gan_options_ref as GR
from tests import reduction_ref as R
from tests.parity_util import ZERO_GRAD_KEYS, build_pair, grad_score, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOUT = 0.375                                    # the upstream gradient: != 1 and a dyadic fraction, so gout / 256 is exact in fp32
NPIX = [1, 255, 256, 257, 262147]               # 262147 = 256 * LS_MAXB + 3: one grid-stride trip more for three pixels


def _run(fn, g, device):
    x = g.clone().to(device).requires_grad_()
    out = fn(GR.as4(x))
    (out * GOUT).backward()
    return out.detach(), x.grad


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('npix', NPIX)
def test_penalty_kernels_against_fp64(npix, c):
    """Value and dgrads of every (norm, penalty) pair.  At the planted pixels (gan_options_ref.PLANTED) every entry whose fp64 gradient
    is exactly 0 -- the all-zero pixel, the exact-norm-1 pixels under hinge and LS, the channels behind the first Linf maximum, the zero
    entry under the L1 sign -- must be exactly 0, every other entry must carry the reference's sign, and where the arithmetic involves
    no rounding (npix = 256: gout / npix is a power of two; gan_options_ref.gp_exact_planted) the entries are compared bit for bit."""
    from sradsgan_amd import ops
    g = GR.gp_inputs(npix, c)
    rows, zrow = GR.planted_rows(npix, c)
    bad = []
    for norm, pen in GR.PAIRS:
        want_v, want_d = GR.gp_ref(g, GOUT, norm, pen)
        got_v, got_d = _run(lambda x: ops.gp_penalty(x, norm, pen), g, DEV)
        tv, td = GR.gp_autograd(g, GOUT, norm, pen)
        for name, got, want, tgot in (('value', got_v, want_v, tv), ('dgrads', got_d, want_d, td)):
            e, te = R.err(got, want), R.err(tgot, want)
            b = R.bound(te)
            print('gp npix=%-6d C=%d %-4s %-5s %-6s err %.3e  torch-fp32 %.3e  bound %.3e%s' % (npix, c, norm, pen, name, e, te, b, '' if e <= b else '   <-- FAIL'))
            if not e <= b:
                bad.append((norm, pen, name, e, te, b))
        if rows:
            idx = rows + ([zrow] if c > 1 else [])
            gd, wd = got_d.cpu()[idx].double(), want_d[idx]
            if not torch.equal(gd == 0, wd == 0) or not torch.equal(torch.sign(gd), torch.sign(wd)):
                bad.append((norm, pen, 'planted zero / sign pattern', gd.tolist(), wd.tolist()))
            if npix == 256:
                names = [k for k, _ in GR.PLANTED]
                exact = [names.index(k) for k in GR.gp_exact_planted(norm, c)]
                if not torch.equal(gd[exact], wd[exact]):
                    bad.append((norm, pen, 'planted values', gd[exact].tolist(), wd[exact].tolist()))
    assert not bad, bad


def test_default_arguments_take_the_old_entry_points_bit_for_bit(monkeypatch):
    from sradsgan_amd import _hip, ops
    lib = _hip.lib()
    calls = []
    for name in ('srhip_gp_norm_penalty_fwd', 'srhip_gp_norm_penalty_bwd', 'srhip_gp_penalty_fwd', 'srhip_gp_penalty_bwd'):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(fn, name))
    g = GR.gp_inputs(257, 3)
    a_v, a_d = _run(ops.gp_penalty, g, DEV)
    b_v, b_d = _run(lambda x: ops.gp_penalty(x, 'L2', 'LS'), g, DEV)
    assert calls == ['srhip_gp_norm_penalty_fwd', 'srhip_gp_norm_penalty_bwd'] * 2
    assert torch.equal(a_v, b_v) and torch.equal(a_d, b_d)
    _run(lambda x: ops.gp_penalty(x, 'L2', 'hinge'), g, DEV)
    assert calls[-2:] == ['srhip_gp_penalty_fwd', 'srhip_gp_penalty_bwd']
    with pytest.raises(ValueError):
        ops.gp_penalty(GR.as4(g.to(DEV)), 'L3', 'LS')


def _close(got, want, tol, msg=''):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(float(np.abs(want).max()), 1e-4)
    err = float(np.abs(got - want).max())
    print('%-40s max abs err %.3e  scale %.3e  bar %.3e' % (msg, err, scale, tol * scale))
    assert err <= tol * scale, '%s: max abs err %.3e vs scale %.3e' % (msg, err, scale)


@pytest.mark.parametrize('norm,penalty', GR.NON_DEFAULT_PAIRS)
def test_gradient_penalty_double_backward_with_options(golden, norm, penalty):
    """test_model_gpu.py::test_gradient_penalty_double_backward for the five non-default pairs, same bars (|gp| 1e-4, gradients 5e-3 of
    the tensor's scale), on the discriminator whose per-pixel norms straddle 1.  Pixels within 1e-3 of a kink (norm 1; an Linf tie) may
    take the other mask or arg-max here than in the reference: the golden records their share, capped at 1 % of the pixels."""
    from sradsgan_amd import model as M
    from sradsgan_amd.train_step import TrainStep
    g = golden('gan_options')
    assert max(g['gp_shares_' + norm][1:3]) <= 0.01
    od = GR.scaled_discriminator_init_(O.Discriminator())
    hd = M.Discriminator()
    hd.load_state_dict(od.state_dict())
    hd.to(DEV)
    step = TrainStep(torch.nn.Linear(1, 1).to(DEV), hd, torch.nn.Linear(1, 1).to(DEV), penalty_type=penalty, grad_penalty_Lp_norm=norm)
    real = O.det_fill('gp.real', (2, 3, 32, 32), 0.5, 0.5).to(DEV)
    fake = O.det_fill('gp.fake', (2, 3, 32, 32), 0.5, 0.5).to(DEV)
    gp = step.gradient_penalty(real, fake, torch.from_numpy(g['gp_alpha']).to(DEV))
    gp.backward()
    tag = 'gp_%s_%s' % (norm, penalty)
    print('%s: gp %.7f, recorded %.7f, diff %.3e' % (tag, gp.item(), float(g[tag]), abs(gp.item() - float(g[tag]))))
    assert abs(gp.item() - float(g[tag])) < 1e-4
    hp = dict(hd.named_parameters())
    for k in ['model.0.weight', 'model.3.weight', 'model.3.bias', 'model.11.weight', 'model.17.fc2.weight', 'model.18.conv1.weight',
              'model.25.weight']:
        _close(O.digest(hp[k].grad), g[tag + '__grad__' + k.replace('.', '__')], 5e-3, msg=tag + ' ' + k)


def _scaled_pair():
    s = GR.TRAIN_SHAPE
    (hg, hd, hf), (og, od, of) = build_pair(s['n_groups'], s['n_blocks'], s['scale'], DEV)
    GR.scaled_discriminator_init_(od, gain=GR.TRAIN_GAIN)
    hd.load_state_dict(od.state_dict(), strict=True)
    return (hg, hd.to(DEV), hf), (og, od, of)


def _one_step(golden, case):
    """One iteration of `case` (None: default options) on both paths.  Returns the figures parity_util.train_parity reduces
    train_small to: worst |scalar diff| (vs the CPU restatement and, for a recorded case, vs the golden), G and D gradient scores
    (vs the restatement's full gradients and the golden's digests), and the worst relative error of D's BatchNorm buffers."""
    from sradsgan_amd.train_step import TrainStep
    g = golden('gan_options')
    opts = GR.CASES[case] if case else {}
    (hg, hd, hf), (og, od, of) = _scaled_pair()
    step = TrainStep(hg, hd, hf, clip_value=GR.GP_CLIP, **opts)
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    alpha = torch.from_numpy(g['train_alpha'])
    want = GR.train_step(og, od, of, torch.optim.Adam(og.parameters(), lr=2e-4), torch.optim.Adam(od.parameters(), lr=2e-4),
                         lr_img, hr_img, alpha, clip_value=GR.GP_CLIP, **opts)
    got = step(lr_img.to(DEV), hr_img.to(DEV), alpha.to(DEV))
    gv = np.array([float(got[k]) for k in GR.SCALARS])
    worst = float(np.abs(gv - np.array([want[k] for k in GR.SCALARS])).max())
    sg, kg = grad_score((hg,), (og,))
    sd, kd = grad_score((hd,), (od,))
    bn = max(rel_err(a, b) for (k, a), (_, b) in zip(hd.state_dict().items(), od.state_dict().items()) if 'running_' in k)
    nbt = [int(v) for k, v in hd.state_dict().items() if k.endswith('num_batches_tracked')]
    if case:
        worst = max(worst, float(np.abs(gv - g[case + '__scalars'][:6]).max()))
        fields = ('names', 'grads', 'counts', 'maxabs')
        s, k = GR.digest_score(hg, *[g['%s__G_%s' % (case, f)] for f in fields], skip=ZERO_GRAD_KEYS)
        if s > sg:
            sg, kg = s, k + ' (recorded)'
        s, k = GR.digest_score(hd, *[g['%s__D_%s' % (case, f)] for f in fields], skip=ZERO_GRAD_KEYS)
        if s > sd:
            sd, kd = s, k + ' (recorded)'
        names, vals, want_nbt = GR.bn_buffers(hd)
        assert list(names) == list(g[case + '__bn_names'])
        rec = g[case + '__bn']
        bn = max(bn, float(np.abs(vals - rec).max() / max(np.abs(rec).max(), 1e-12)))
        assert nbt == list(g[case + '__nbt']), (nbt, g[case + '__nbt'])
    print('step[%s]: scalars %.3e  G gradient %.3e (%s)  D gradient %.3e (%s)  BatchNorm buffers %.3e  num_batches_tracked %s'
          % (case or 'default', worst, sg, kg, sd, kd, bn, sorted(set(nbt))))
    return dict(worst=worst, g=sg, d=sd, bn=bn, nbt=nbt, gv=gv)


@pytest.mark.parametrize('case', list(GR.CASES))
def test_one_training_step_per_recorded_case(golden, case):
    """The default conv arithmetic.  Bars: what parity_util.train_parity applies to train_small -- scalars 1e-3 absolute, G gradients
    5e-3, D gradients 2e-2 (the double backward through train-mode BatchNorm; train_parity's d_bar), BatchNorm buffers 5e-3 relative;
    num_batches_tracked exactly (5 for the relativistic step, else 4)."""
    r = _one_step(golden, case)
    assert set(r['nbt']) == {5 if case == 'relative' else 4}
    assert r['worst'] < 1e-3 and r['g'] < 5e-3 and r['d'] < 2e-2 and r['bn'] < 5e-3, r


def _state(step):
    return step.arena_G.flat_g.clone(), step.arena_D.flat_g.clone()


def test_relativistic_step_runs_the_plain_passes_and_leaves_the_plain_gradients():
    from sradsgan_amd import ops
    from sradsgan_amd.train_step import TrainStep
    lr_img, hr_img = [t.to(DEV) for t in GR.case_inputs('train_small', 0)]
    alpha = O.det_fill('rel.alpha', (2, 1, 1, 1), 0.5, 0.5).to(DEV)
    with torch.no_grad():
        real_mean = float(ops.mean(_scaled_pair()[0][1](hr_img)))              # D(real) on the step's weights, before any update
    res = {}
    for rel in (False, True):
        (hg, hd, hf), _ = _scaled_pair()                                        # the same state both times
        count = [0]
        hd.register_forward_hook(lambda m, i, o: count.__setitem__(0, count[0] + 1))
        step = TrainStep(hg, hd, hf, clip_value=GR.GP_CLIP, relative=rel)
        out = step(lr_img, hr_img, alpha)
        torch.cuda.synchronize()
        res[rel] = (_state(step), {k: float(out[k]) for k in GR.SCALARS}, count[0], GR.bn_buffers(hd))
    (pg, pd), ps, pn, pb = res[False]
    (rg, rd), rs, rn, rb = res[True]
    assert torch.equal(pg, rg) and torch.equal(pd, rd)                          # both arenas bit for bit
    assert rn <= pn == 3, (pn, rn)                                              # D(gen), D(real), D(interp): no pass more
    ulp = 2.0 ** -23 * max(abs(ps['loss_gan']), abs(real_mean), abs(rs['loss_gan']))
    print('loss_gan plain %.7f relativistic %.7f mean(D(real)) %.7f' % (ps['loss_gan'], rs['loss_gan'], real_mean))
    assert abs(rs['loss_gan'] - (ps['loss_gan'] + real_mean)) <= 2 * ulp
    assert abs(rs['loss_G'] - (ps['loss_G'] + 1e-3 * real_mean)) <= 4 * 2.0 ** -23 * max(abs(ps['loss_G']), 1e-3 * abs(real_mean))
    assert ps['loss_D'] == rs['loss_D'] and ps['gp'] == rs['gp']
    assert set(pb[2]) == {4} and set(rb[2]) == {5} and float(np.abs(pb[1] - rb[1]).max()) > 0


@pytest.mark.parametrize('order', [dict(reuse_d_fake=False), dict(overlap_wgrad=False), dict(overlap_d_step=False)])
def test_other_host_orders_carry_the_options(golden, order):
    """_compute (every pass run) and _compute_shared (one stream; no D stream) with the L2 content loss and the relativistic losses
    together: the logged scalars against the CPU restatement under train_small's 1e-3, D's BatchNorm buffers after the five updates."""
    from sradsgan_amd.train_step import TrainStep
    opts = dict(loss_Lp_norm='L2', relative=True, penalty_type='hinge', grad_penalty_Lp_norm='Linf')
    (hg, hd, hf), (og, od, of) = _scaled_pair()
    step = TrainStep(hg, hd, hf, clip_value=GR.GP_CLIP, **opts, **order)
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    alpha = torch.from_numpy(golden('gan_options')['train_alpha'])
    want = GR.train_step(og, od, of, torch.optim.Adam(og.parameters(), lr=2e-4), torch.optim.Adam(od.parameters(), lr=2e-4),
                         lr_img, hr_img, alpha, clip_value=GR.GP_CLIP, **opts)
    got = step(lr_img.to(DEV), hr_img.to(DEV), alpha.to(DEV))
    worst = max(abs(float(got[k]) - want[k]) for k in GR.SCALARS)
    bn = max(rel_err(a, b) for (k, a), (_, b) in zip(hd.state_dict().items(), od.state_dict().items()) if 'running_' in k)
    sg, _ = grad_score((hg,), (og,))
    sd, _ = grad_score((hd,), (od,))
    print('host order %s: scalars %.3e  G gradient %.3e  D gradient %.3e  BatchNorm buffers %.3e' % (order, worst, sg, sd, bn))
    assert {int(v) for k, v in hd.state_dict().items() if k.endswith('num_batches_tracked')} == {5}
    assert worst < 1e-3 and sg < 5e-3 and sd < 2e-2 and bn < 5e-3


def _loaders(seed):
    g = torch.Generator().manual_seed(seed)
    train = [torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    hr = torch.rand(2, 3, 32, 32, generator=g)
    return train, [(torch.nn.functional.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]


@pytest.mark.parametrize('which', ['hinge_linf', 'relative', 'content_l2', 'drcan', 'sragan'])
def test_trainers_build_and_train_with_the_options(tmp_path, which):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import drcan, sragan
    common = dict(scale_factor=4, num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32,
                  hr_width=32, sample_interval=1)
    if which == 'drcan':                                     # DRCAN keeps the reference defaults (test_drcan_cpu pins its refusals)
        cls, args = drcan.DRCAN, drcan.default_args(n_resgroups=2, n_resblocks=1, **common)
    elif which == 'sragan':
        cls, args = sragan.SRAGAN, sragan.default_args(n_residual_blocks=1, n_basic_blocks=1, penalty_type='hinge',
                                                       grad_penalty_Lp_norm='Linf', loss_Lp_norm='L2', **common)
    else:
        opts = {'hinge_linf': dict(penalty_type='hinge', grad_penalty_Lp_norm='Linf'), 'relative': dict(relativeGan=True),
                'content_l2': dict(loss_Lp_norm='L2')}[which]
        cls, args = T.SRADSGAN, T.default_args(n_residual_blocks=1, n_basic_blocks=1, **common, **opts)
    train, test = _loaders(7)
    net = cls(args, train_loader=train, test_loader=test)
    hist = net.train()
    s = net.step
    assert (s.penalty_type, s.grad_penalty_Lp_norm, s.loss_Lp_norm, s.relative) == (args.penalty_type, args.grad_penalty_Lp_norm,
                                                                                     args.loss_Lp_norm, bool(args.relativeGan))
    assert len(hist) == 1 and all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
    assert os.path.exists(os.path.join(str(tmp_path), 'model', 'generator_param_epoch_1.pkl'))


@pytest.mark.parametrize('bad', [dict(penalty_type='hinge2'), dict(grad_penalty_Lp_norm='L3'), dict(loss_Lp_norm='Linf')])
def test_option_values_outside_the_reference_choices_are_value_errors(bad):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import drcan, sragan
    for make, cls in ((T.default_args, T.SRADSGAN), (drcan.default_args, drcan.DRCAN), (sragan.default_args, sragan.SRAGAN)):
        with pytest.raises(ValueError):
            cls(make(**bad))


def test_trainers_admit_only_penalty_pairs_with_a_recorded_iteration():
    """The kernels and TrainStep take all six (norm, penalty) pairs; the trainers run the three that a recorded iteration of the
    reference covers, and say so for the rest."""
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import sragan
    assert set(T.SRADSGAN.penalty_pairs) == {('L2', 'LS'), ('L1', 'LS'), ('Linf', 'hinge')}
    for norm, penalty in (('L2', 'hinge'), ('L1', 'hinge'), ('Linf', 'LS')):
        for make, cls in ((T.default_args, T.SRADSGAN), (sragan.default_args, sragan.SRAGAN)):
            with pytest.raises(NotImplementedError, match='recorded'):
                cls(make(grad_penalty_Lp_norm=norm, penalty_type=penalty))
