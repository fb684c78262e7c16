"""The four loss options (--penalty_type, --grad_penalty_Lp_norm, --loss_Lp_norm, --relativeGan) without a GPU: the restatement of
tests/gan_options_ref.py against the values tools/make_golden_gan_options.py recorded from the reference (and against train_small.npz
with default options), the conditions the golden's discriminator has to meet, the kernel-test inputs, the relativistic identities the
HIP step relies on, and the C ABI of the new entry points (declared, bound, refusing what they cannot serve)."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import gan_options_ref as GR
from tests.parity_util import ZERO_GRAD_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sradsgan_hip.h')
GP_KEYS = ['model.0.weight', 'model.3.weight', 'model.3.bias', 'model.11.weight', 'model.17.fc2.weight', 'model.18.conv1.weight',
           'model.25.weight']


def _nets(scaled, dtype=torch.float32):
    s = GR.TRAIN_SHAPE
    G = O.GeneratorResNet(O.ResGroup, n_residual_blocks=s['n_groups'], n_basic_blocks=s['n_blocks'], upscale_factor=s['scale'])
    D, Fx = O.Discriminator(), O.FeatureExtractor()
    O.det_init_(G, prefix='G.'), O.det_init_(Fx, prefix='F.')
    GR.scaled_discriminator_init_(D, gain=GR.TRAIN_GAIN) if scaled else O.det_init_(D, prefix='D.')
    return [m.to(dtype) for m in (G, D, Fx)]


def _adams(G, D):
    return torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999)), torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.999))


def test_restatement_with_default_options_reproduces_train_small(golden):
    g = golden('train_small')
    G, D, Fx = _nets(scaled=False)
    oG, oD = _adams(G, D)
    for it in range(2):
        lr_img, hr_img = GR.case_inputs('train_small', it)
        s = GR.train_step(G, D, Fx, oG, oD, lr_img, hr_img, torch.from_numpy(g['alpha%d' % it]))
        np.testing.assert_allclose([s[k] for k in GR.SCALARS], g['scalars%d' % it], rtol=2e-4, atol=2e-5, err_msg='it%d' % it)


@pytest.mark.parametrize('case', list(GR.CASES))
def test_restatement_reproduces_the_recorded_training_cases(golden, case):
    """Scalars as test_oracle_golden compares train_small's; gradients by parity_util.grad_score's measure on the recorded entries under
    its bars (G 5e-3, D 2e-2: the double backward through train-mode BatchNorm); BatchNorm buffers to 1e-3, the counters exactly."""
    g = golden('gan_options')
    G, D, Fx = _nets(scaled=True)
    oG, oD = _adams(G, D)
    lr_img, hr_img = GR.case_inputs('train_small', 0)
    s = GR.train_step(G, D, Fx, oG, oD, lr_img, hr_img, torch.from_numpy(g['train_alpha']), clip_value=GR.GP_CLIP, **GR.CASES[case])
    want = g[case + '__scalars']
    np.testing.assert_allclose([s[k] for k in GR.SCALARS] + [s['d_real_mean']], want, rtol=2e-4, atol=2e-5)
    for tag, net, bar in (('G', G, 5e-3), ('D', D, 2e-2)):
        score, key = GR.digest_score(net, *[g['%s__%s_%s' % (case, tag, f)] for f in ('names', 'grads', 'counts', 'maxabs')],
                                     skip=ZERO_GRAD_KEYS)
        print('%s %s gradient score %.3e (%s)' % (case, tag, score, key))
        assert score < bar, (tag, score, key)
    names, vals, nbt = GR.bn_buffers(D)
    assert list(names) == list(g[case + '__bn_names']) and list(nbt) == list(g[case + '__nbt'])
    assert set(nbt) == {5 if case == 'relative' else 4}
    np.testing.assert_allclose(vals, g[case + '__bn'], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize('norm,penalty', GR.NON_DEFAULT_PAIRS)
def test_oracle_penalty_reproduces_the_recorded_reference_penalties(golden, norm, penalty):
    g = golden('gan_options')
    d = GR.scaled_discriminator_init_(O.Discriminator())
    real = O.det_fill('gp.real', (2, 3, 32, 32), 0.5, 0.5)
    fake = O.det_fill('gp.fake', (2, 3, 32, 32), 0.5, 0.5)
    gp = O.gradient_penalty(d, real, fake, torch.from_numpy(g['gp_alpha']), norm, penalty)
    tag = 'gp_%s_%s' % (norm, penalty)
    assert abs(gp.item() - float(g[tag])) < 1e-4 * max(1.0, float(g[tag]))
    sd = dict(d.named_parameters())
    for k in GP_KEYS:
        want = g[tag + '__grad__' + k.replace('.', '__')]
        err = float(np.abs(O.digest(sd[k].grad) - want).max())
        assert err <= 5e-3 * max(float(np.abs(want).max()), 1e-4), (k, err)


def test_recorded_shares_straddle_one_and_keep_the_bands_thin(golden):
    g = golden('gan_options')
    assert float(g['band']) == GR.BAND == 1e-3 and float(g['band_cap']) == GR.BAND_CAP == 0.01
    assert float(g['gain']) == GR.GP_GAIN and float(g['train_gain']) == GR.TRAIN_GAIN and float(g['clip']) == GR.GP_CLIP
    rows = [('gp_shares_' + n, n) for n in GR.NORMS] + [(c + '__shares', GR.CASES[c].get('grad_penalty_Lp_norm', 'L2')) for c in GR.CASES]
    for key, norm in rows:
        above, band, tie, margin = g[key]
        print('%-22s above 1: %.4f  within 1e-3 of 1: %.4f  Linf near-ties: %.4f  smallest margin %.2e' % (key, above, band, tie, margin))
        assert 0.2 <= above <= 0.8 and band <= 0.01 and tie <= 0.01 and margin >= 0
        assert norm == 'Linf' or tie == 0
    # and they are what the restatement's discriminator gives on this host
    d = GR.scaled_discriminator_init_(O.Discriminator())
    grads = GR.input_gradient(d, O.det_fill('gp.real', (2, 3, 32, 32), 0.5, 0.5), O.det_fill('gp.fake', (2, 3, 32, 32), 0.5, 0.5),
                              torch.from_numpy(g['gp_alpha']))
    for n in GR.NORMS:
        sh = GR.pixel_norm_shares(grads, n)
        assert GR.shares_ok(*sh[:3]) and abs(sh[0] - g['gp_shares_' + n][0]) <= 0.01, (n, sh)


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('npix', [1, 255, 256, 257, 262147])
def test_kernel_inputs_hold_the_planted_pixels_and_nothing_else_near_a_kink(npix, c):
    t = GR.gp_inputs(npix, c)
    assert t.shape == (npix, c) and t.dtype == torch.float32
    rows, zrow = GR.planted_rows(npix, c)
    if npix < GR.MIN_PLANTED_NPIX:
        assert rows == []
    else:
        assert len(set(rows)) == len(GR.PLANTED) and zrow not in rows
        assert torch.equal(t[rows], GR.planted_pixels(c))
        planted = dict(zip([k for k, _ in GR.PLANTED], t[rows].double()))
        assert float(planted['zero'].abs().max()) == 0
        for n in GR.NORMS:
            assert float(GR.pixel_norm(planted['unit_first'][None], n)) == 1.0
        if c >= 3:
            assert all(float(GR.pixel_norm(planted['unit_second_neg'][None], n)) == 1.0 for n in GR.NORMS)
            assert float(GR.pixel_norm(planted['l1_one'][None], 'L1')) == 1.0
            for k in ('tie_half', 'tie_two'):
                a = planted[k].abs()
                assert float(a[0]) == float(a.max()) == float(a[1])
        if c > 1:
            assert float(t[zrow, GR.ZERO_ENTRY_CHANNEL]) == 0.0 and float(t[zrow].abs().max()) > 0
    keep = torch.ones(npix, dtype=torch.bool)
    keep[rows] = False
    for n in GR.NORMS:
        nrm = GR.pixel_norm(t.double(), n)
        assert not bool(((nrm - 1).abs() <= 1e-5)[keep].any()), n
        if npix >= 255:
            share = float((nrm > 1).double().mean())
            assert 0.05 < share < 0.95, (n, share)               # both sides of every mask are exercised


@pytest.mark.parametrize('norm,penalty', GR.PAIRS)
def test_closed_forms_are_autograd_in_fp64(norm, penalty):
    g = GR.gp_inputs(257, 3)
    want_v, want_d = GR.gp_autograd(g, 0.37, norm, penalty, torch.float64)
    v, d = GR.gp_ref(g, 0.37, norm, penalty)
    assert abs(float(v) - float(want_v)) < 1e-14 and float((d - want_d).abs().max()) < 1e-15


def test_relativistic_step_has_the_plain_gradients_and_shifts_loss_gan_by_the_real_mean():
    """What TrainStep(relative=True) relies on, in fp64 on the restatement: with the wgan criterion the relativistic losses are linear,
    so G's and D's gradients are the plain step's, loss_D is the plain loss_D, and loss_gan differs by mean(D(real))."""
    nets = _nets(scaled=True, dtype=torch.float64)
    lr_img, hr_img = [t.double() for t in GR.case_inputs('train_small', 0)]
    alpha = O.det_fill('rel.alpha', (2, 1, 1, 1), 0.5, 0.5).double()
    runs = {}
    for rel in (False, True):
        G, D, Fx = copy.deepcopy(nets)
        oG, oD = _adams(G, D)
        s = GR.train_step(G, D, Fx, oG, oD, lr_img, hr_img, alpha, clip_value=GR.GP_CLIP, relative=rel)
        runs[rel] = (s, [p.grad.clone() for p in G.parameters()], [p.grad.clone() for p in D.parameters() if p.grad is not None],
                     GR.bn_buffers(D))
    (sp, gp_, dp, bp), (sr, gr, dr, br) = runs[False], runs[True]
    for a, b in zip(gp_ + dp, gr + dr):
        assert float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1e-30)
    assert abs(sr['loss_gan'] - (sp['loss_gan'] + sp['d_real_mean'])) < 1e-12 and abs(sr['loss_D'] - sp['loss_D']) < 1e-12
    assert abs(sr['loss_G'] - (sp['loss_G'] + 1e-3 * sp['d_real_mean'])) < 1e-12
    assert set(bp[2]) == {4} and set(br[2]) == {5}
    assert float(np.abs(bp[1] - br[1]).max()) > 0                       # the extra update is observable


def _decl_args(name):
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)' % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_new_entry_points_are_declared_and_bound_with_matching_argument_counts():
    from sradsgan_amd import _hip
    for name, n in (('srhip_gp_penalty_fwd', 9), ('srhip_gp_penalty_bwd', 8)):
        args = _decl_args(name)
        res, types = _hip.SIGNATURES[name]
        assert len(args) == len(types) == n and res is ctypes.c_int
        assert args[-3].split()[-1] == 'norm_kind' and args[-2].split()[-1] == 'penalty_kind' and types[-3] is types[-2] is ctypes.c_int
    assert len(_decl_args('srhip_gp_norm_penalty_fwd')) == 7 and len(_decl_args('srhip_gp_norm_penalty_bwd')) == 6     # untouched


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


def test_new_entry_points_refuse_five_channels_and_unknown_kinds_on_the_host(lib):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)                       # stands for every tensor argument: a refused call never reads it
    assert lib.srhip_abi_version() == 14
    f, b = lib.srhip_gp_penalty_fwd, lib.srhip_gp_penalty_bwd
    for fn, args, word in ((f, (p, p, p, 4096, 10, 5, 0, 0, None), b'1 <= C <= 4'), (b, (p, p, p, 10, 5, 2, 1, None), b'1 <= C <= 4'),
                           (f, (p, p, p, 4096, 10, 3, 3, 0, None), b'unknown kind'), (f, (p, p, p, 4096, 10, 3, 0, 2, None), b'unknown kind'),
                           (b, (p, p, p, 10, 3, -1, 0, None), b'unknown kind'), (b, (p, p, p, 10, 3, 1, 7, None), b'unknown kind'),
                           (f, (p, p, p, 16, 10, 3, 1, 1, None), b'workspace')):
        rc = fn(*args)
        msg = lib.srhip_last_error()
        assert rc != 0 and word in msg and b'gp_penalty' in msg, (rc, msg)


def test_unknown_option_names_are_value_errors():
    from sradsgan_amd import ops
    from sradsgan_amd.train_step import TrainStep
    x = torch.zeros(1, 3, 2, 2)
    for kw in (dict(norm='L3'), dict(penalty='relu'), dict(norm='linf')):
        with pytest.raises(ValueError):
            ops.gp_penalty(x, **kw)
    lin = torch.nn.Linear(1, 1)
    for kw in (dict(penalty_type='LSQ'), dict(grad_penalty_Lp_norm='L0'), dict(loss_Lp_norm='Linf')):
        with pytest.raises(ValueError):
            TrainStep(lin, lin, lin, **kw)
