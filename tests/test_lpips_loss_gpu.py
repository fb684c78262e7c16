"""LPIPS as a loss on the device (LPIPS.loss, csrc/lpips.hip's three backward kernels, TrainStep's weight_lpips) against fp64 autograd of
tests/lpips_loss_ref.py, ATen's max-pool backward and conv_emulation's fp64 contractions.

Bounds.  Head backward and the fp32 end-to-end gradient: the device runs the restatement's arithmetic in fp32 in another order, so the bar
is 8 x the largest error of the restatement's own fp32 CPU autograd (the multiple of test_lpips_gpu._bar), for the head with the floor
2e-6 max|ref|.  End to end a ReLU or an arg-max may flip between two fp32 runs, which moves single elements by more: at most 1e-4 of the
elements may lie beyond the bar, and the fp32 CPU run itself has none.  Pool backward: exact, on the 16-bit grid.  Stem backward:
conv_emulation's element bound with the tau of the fp32 conv routes.  bf16x3: the relative 2-norm distance from fp64 against 4 x that of an
emulated run -- the restatement in fp32 with convs 2-5 and their data gradients through conv_emulation's split-bf16 contraction, which
is what the device computes up to summation order.

Every test prints its figures before it asserts."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O
from tests import conv_emulation as E
from tests import gan_options_ref as GR
from tests import lpips_loss_ref as L
from tests import lpips_ref as R
from tests.parity_util import build_pair, grad_score

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TAU_FP32 = 32 * E.U24


@pytest.fixture(scope='module')
def G():
    return np.load(R.GOLDEN)


@pytest.fixture(scope='module')
def sd():
    return R.alexnet_state_dict()


@pytest.fixture(scope='module')
def model(G, sd):
    from sradsgan_amd.lpips import LPIPS
    m = LPIPS()
    m.load_torchvision_alexnet(sd)
    m.load_lin(R.lin_state_dict(G))
    return m.to(DEV)


@pytest.fixture(scope='module')
def cases(G, sd):
    """name -> (sr, hr, fp64 loss, fp64 gradient, the fp32 CPU run's gradient); computed once, never modified."""
    lin = [G['lin%d' % k] for k in range(5)]
    out = {}
    for name in ('s0', 's1', 's2', 'big'):
        sr, hr = R.big_inputs() if name == 'big' else (torch.from_numpy(G[name + '_sr']), torch.from_numpy(G[name + '_hr']))
        val, g64 = L.loss_and_grad(sr, hr, sd, lin)
        _, g32 = L.loss_and_grad(sr, hr, sd, lin, dtype=torch.float32)
        out[name] = (sr, hr, val, g64, g32.double())
    return out


def _loss_grad(model, sr, hr, **kw):
    pred = sr.to(DEV).requires_grad_(True)
    target = hr.to(DEV)
    val = model.loss(pred, target, **kw)
    val.backward()
    return val.detach().cpu(), pred.grad.cpu(), target


# ---- head backward ------------------------------------------------------------------------------------------------------------------ #
PAIRS = [(0, 1), (0, 2), (2, 0), (1, 1), (3, 4), (3, 5), (4, 2)]             # test_head's: shared indices, a self pair, a pair of equal copies
UP = 0.375


@pytest.mark.parametrize('c', [64, 192, 384, 256])
@pytest.mark.parametrize('hw', [(1, 2), (3, 5), (12, 12)])
def test_head_backward(c, hw):
    from sradsgan_amd import ops
    h, w = hw
    f = F.relu(R.hash16(6 * c * h * w, c + h).float().reshape(6, c, h, w) + 0.1) * 3      # test_head's features and zero pixels
    f[0, :, 0, 0] = 0
    f[1, :, 0, 0] = 0
    f[2, :, 0, w - 1] = 0
    f[5] = f[3]
    lw = (R.hash16(c, 3 * c) + 0.5).float()
    count = len(PAIRS) * h * w
    pt = torch.tensor(PAIRS, dtype=torch.int32, device=DEV)
    up = torch.tensor(UP, device=DEV)
    got = ops.lpips_head_bwd_raw(f.to(DEV), pt, lw.to(DEV), up, count).cpu()
    again = ops.lpips_head_bwd_raw(f.to(DEV), pt, lw.to(DEV), up, count).cpu()
    s = UP / count
    ref = torch.cat([L.head_grad_autograd(f[j:j + 1].double(), f[i:i + 1].double(), lw.double(), s) for i, j in PAIRS])
    ref32 = torch.cat([L.head_grad_autograd(f[j:j + 1], f[i:i + 1], lw, s) for i, j in PAIRS]).double()
    e32 = float((ref32 - ref).abs().max())
    bar = max(8 * e32, 2e-6 * float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    print('head bwd C=%d %dx%d: err %.2e, bar %.2e (CPU fp32 %.2e, max|ref| %.2e), err / bar %.3f' % (
        c, h, w, err, bar, e32, float(ref.abs().max()), err / bar))
    assert tuple(got.shape) == (len(PAIRS), c, h, w) and float(ref.abs().max()) > 0
    assert torch.isfinite(got).all()
    pred = torch.stack([f[j] for _, j in PAIRS])
    assert bool((got[pred <= 0] == 0).all())                               # through the ReLU: exact zeros
    for p, (_, j) in enumerate(PAIRS):                                     # the zero-norm pred pixels: zeros, no 0 / 0
        if j in (0, 1):
            assert bool((got[p, :, 0, 0] == 0).all())
        if j == 2:
            assert bool((got[p, :, 0, w - 1] == 0).all())
    assert bool((got[3] == 0).all()) and bool((got[5] == 0).all())          # identical inputs: no pull at all
    assert err <= bar
    assert torch.equal(got, again)


def test_head_backward_passes_a_nan_feature_on():
    from sradsgan_amd import ops
    f = F.relu(R.hash16(2 * 64 * 2 * 2, 5).float().reshape(2, 64, 2, 2) + 0.1)
    f[1, 3, 0, 1] = float('nan')
    pt = torch.tensor([(0, 1)], dtype=torch.int32, device=DEV)
    got = ops.lpips_head_bwd_raw(f.to(DEV), pt, torch.ones(64, device=DEV), torch.tensor(1.0, device=DEV), 4).cpu()
    assert torch.isnan(got[0, 3, 0, 1]) and torch.isfinite(got[0, :, 1, :]).all() and torch.isfinite(got[0, :, 0, 0]).all()


# ---- pool backward ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('shape', [(2, 8, 11, 64), (1, 53, 53, 64), (2, 26, 26, 192), (1, 3, 3, 64)])
def test_maxpool3x3s2_backward_is_bit_equal_to_aten(shape):
    """x and dy on hash16's 16-bit grid: ties occur (the first maximum must win) and sums of four dy terms plus a residual are exact."""
    from sradsgan_amd import ops
    n, h, w, c = shape
    x = (R.hash16(n * c * h * w, 7 + h) * 4).float().reshape(n, c, h, w)
    ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    dy = R.hash16(n * c * ho * wo, 11 + h).float().reshape(n, c, ho, wo)
    res = R.hash16(n * c * h * w, 13 + h).float().reshape(n, c, h, w)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2).backward(dy)
    want = xr.grad
    windows = F.unfold(x, 3, stride=2).reshape(n, c, 9, -1)
    ties = int(((windows == windows.max(2, keepdim=True).values).sum(2) > 1).sum())
    got = ops.max_pool3x3s2_bwd_raw(x.to(DEV), dy.to(DEV)).cpu()
    fused = ops.max_pool3x3s2_bwd_raw(x.to(DEV), dy.to(DEV), relu=True, residual=res.to(DEV)).cpu()
    masked = ops.max_pool3x3s2_bwd_raw(x.to(DEV), dy.to(DEV), relu=True).cpu()
    print('pool bwd %s: %d windows with a tied maximum, %d inputs in two or more windows take a gradient' % (
        shape, ties, int((want != 0).sum())))
    assert ties > 0 or h == 3
    assert torch.equal(got, want)
    assert torch.equal(masked, want * (x > 0))
    assert torch.equal(fused, want * (x > 0) + res)
    with pytest.raises(ValueError):
        ops.max_pool3x3s2_bwd_raw(x.to(DEV), dy.to(DEV)[:, :, :, :-1] if wo > 1 else torch.zeros(n, c, ho, 2, device=DEV))


# ---- stem backward ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('hw', [(31, 31), (35, 47), (34, 45), (33, 44)])
def test_stem_backward(sd, hw, normalize):
    """all four residues of (H - 7) mod 4, tiles cut by the image edge, two images"""
    from sradsgan_amd import ops
    h, w = hw
    ho, wo = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    g = R.hash16(2 * 64 * ho * wo, 50 + h).float().reshape(2, 64, ho, wo)
    wt = sd['features.0.weight']
    got = ops.lpips_stem_bwd_raw(g.to(DEV), wt.to(DEV).permute(2, 3, 1, 0).contiguous(), hw, normalize).cpu()
    again = ops.lpips_stem_bwd_raw(g.to(DEV), wt.to(DEV).permute(2, 3, 1, 0).contiguous(), hw, normalize).cpu()
    ref, absref = E.conv_dgrad(g, wt, (2, 3, h, w), 4, 2, 'fp32')
    fac = ((2.0 if normalize else 1.0) / torch.tensor(R.SCALE, dtype=torch.float64)).view(1, 3, 1, 1)
    ratio = E.assert_conv_close(got, ref * fac, absref * fac, TAU_FP32, what='lpips stem bwd %dx%d' % hw)
    print('stem bwd %dx%d normalize=%s: err / bound %.3f' % (hw + (normalize, ratio)))
    assert tuple(got.shape) == (2, 3, h, w) and float(ref.abs().min(dim=1).values.max()) > 0
    assert torch.equal(got, again)
    one = ops.lpips_stem_bwd_raw(g[1:].to(DEV), wt.to(DEV).permute(2, 3, 1, 0).contiguous(), hw, normalize).cpu()
    assert torch.equal(one[0], got[1])                                     # an image's gradient does not depend on the batch


# ---- end to end --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('name', ['s0', 's1', 's2', 'big'])
def test_fp32_gradient_end_to_end(model, cases, name):
    from sradsgan_amd import ops
    sr, hr, val, g64, g32 = cases[name]
    with ops.conv_math('fp32'):
        got_val, got, target = _loss_grad(model, sr, hr)
        metric = model(sr.to(DEV), hr.to(DEV)).cpu()
    e32 = float((g32 - g64).abs().max())
    bar = 8 * e32
    gmax = float(g64.abs().max())
    err = (got.double() - g64).abs()
    share = float((err > bar).double().mean())
    print('%s fp32: max|g| %.3e, CPU fp32 error %.2e (%.2e of max|g|), bar %.2e; gpu worst %.2e, share beyond the bar %.2e' % (
        name, gmax, e32, e32 / gmax, bar, float(err.max()), share))
    assert got_val.dtype == torch.float32 and got_val.dim() == 0 and tuple(got.shape) == tuple(sr.shape)
    assert float(((g32 - g64).abs() > bar).double().mean()) == 0.0         # the fp32 CPU run has no element beyond the bar
    assert torch.isfinite(got).all() and gmax > 0
    assert share <= 1e-4
    mean = float(metric.mean())
    assert abs(float(got_val) - mean) <= 2.0 ** -23 * mean                  # the loss is the metric's batch mean, rounded to fp32
    assert abs(mean - float(val)) <= 1e-5 * float(val)
    assert target.grad is None


@pytest.mark.parametrize('name', ['s0', 'big'])
def test_bf16x3_gradient_and_half_is_the_same_bits(model, cases, G, sd, name):
    from sradsgan_amd import ops
    sr, hr, _, g64, _ = cases[name]
    lin = [G['lin%d' % k] for k in range(5)]
    _, emu = L.loss_and_grad(sr, hr, sd, lin, dtype=torch.float32, conv=L.emulated_conv('bf16x3'))
    with ops.conv_math('bf16x3'):
        _, got, _ = _loss_grad(model, sr, hr)
    with ops.conv_math('half'):
        _, half, _ = _loss_grad(model, sr, hr)
        assert ops.get_conv_math() == 'half'
    e = float((emu.double() - g64).norm() / g64.norm())
    d = float((got.double() - g64).norm() / g64.norm())
    print('%s bf16x3: emulated run %.3e, gpu %.3e relative 2-norm distance from fp64; ratio %.3f' % (name, e, d, d / e))
    assert d <= 4 * e
    assert torch.equal(half, got)


def test_loss_node_contract(model, cases):
    sr, hr = cases['s0'][:2]
    pred = sr.to(DEV).requires_grad_(True)
    target = hr.to(DEV)
    val = model.loss(pred, target)
    g, = torch.autograd.grad(val, pred, create_graph=True)
    with pytest.raises(RuntimeError):                                       # once_differentiable: no double backward
        g.sum().backward()
    again, = torch.autograd.grad(model.loss(pred, target), pred)
    assert torch.equal(again, g.detach())                                   # deterministic
    scaled, = torch.autograd.grad(model.loss(pred, target) * 0.25, pred)    # the upstream gradient reaches the kernels
    assert bool(((scaled - 0.25 * again).abs() <= 2.0 ** -22 * again.abs()).all())
    with torch.no_grad():
        plain = model.loss(pred, target)
    assert not plain.requires_grad and torch.equal(plain, val.detach())
    assert not model.loss(pred.detach(), target).requires_grad
    with pytest.raises(ValueError, match='pred only'):
        model.loss(pred, target.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='shape mismatch'):
        model.loss(pred, target[:, :, :-1])
    with pytest.raises(ValueError, match='at least 31'):
        model.loss(pred[:, :, :30], target[:, :, :30])


# ---- the training step -------------------------------------------------------------------------------------------------------------- #
def _nets():
    s = GR.TRAIN_SHAPE
    (hg, hd, hf), (_, od, _) = build_pair(s['n_groups'], s['n_blocks'], s['scale'], DEV)
    GR.scaled_discriminator_init_(od, gain=GR.TRAIN_GAIN)
    hd.load_state_dict(od.state_dict(), strict=True)
    return hg, hd.to(DEV), hf


@pytest.mark.parametrize('order', [dict(), dict(overlap_wgrad=False), dict(reuse_d_fake=False)],
                         ids=['onewalk', 'shared', 'plain'])
def test_step_adds_the_lpips_gradient_to_the_generator_alone(model, order, request):
    """HR tiles 32 x 32 (train_small's).  G's gradient with weight_lpips = 1 minus the one with weight 0 is the gradient of
    lpips.loss(G(lr), hr) through G alone (parity_util.grad_score < 5e-3, test_gan_options_gpu's bar for G); loss_G moves by the logged
    term; D's arena keeps its bits."""
    from sradsgan_amd.train_step import TrainStep
    order_id = request.node.callspec.id
    lr_img, hr_img = [t.to(DEV) for t in GR.case_inputs('train_small', 0)]
    alpha = O.det_fill('lpips.alpha', (2, 1, 1, 1), 0.5, 0.5).to(DEV)
    res = {}
    for weight in (0.0, 1.0):
        hg, hd, hf = _nets()
        step = TrainStep(hg, hd, hf, clip_value=GR.GP_CLIP, lpips=model if weight else None, weight_lpips=weight, **order)
        taken = []
        for name in ('_compute_onewalk', '_compute_shared', '_compute_plain'):
            setattr(step, name, (lambda fn, name: lambda *a: (taken.append(name), fn(*a))[1])(getattr(step, name), name))
        out = step(lr_img, hr_img, alpha)
        assert taken == ['_compute_' + order_id]
        torch.cuda.synchronize()
        res[weight] = (step.arena_G.flat_g.clone(), step.arena_D.flat_g.clone(), {k: float(v) for k, v in out.items() if v.dim() == 0},
                       hg, step)
    g0, d0, s0, _, _ = res[0.0]
    g1, d1, s1, hg1, step1 = res[1.0]
    assert 'lpips' not in s0 and s1['lpips'] > 0
    assert torch.equal(d0, d1)
    assert abs((s1['loss_G'] - s0['loss_G']) - s1['lpips']) < 1e-3
    for k in ('pixel', 'content', 'loss_gan', 'loss_D', 'gp'):
        assert s0[k] == s1[k], k
    ref_g = _nets()[0]
    direct = model.loss(ref_g(lr_img), hr_img)
    direct.backward()
    direct = float(direct.detach())
    step1.arena_G.flat_g.copy_(g1 - g0)                                     # hg1's .grad tensors are views of the arena
    score, worst = grad_score((hg1,), (ref_g.cpu(),))
    print('step %s: lpips %.6f (direct %.6f), G gradient difference vs lpips through G alone: score %.3e (%s)' % (
        order, s1['lpips'], direct, score, worst))
    assert abs(direct - s1['lpips']) <= 1e-5 * direct
    assert float((g1 - g0).abs().max()) > 0 and score < 5e-3


def test_step_and_trainers_refuse_what_they_cannot_run(model, tmp_path):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import drcan
    from sradsgan_amd.train_step import TrainStep
    hg, hd, hf = _nets()
    with pytest.raises(ValueError, match='use_graph'):
        TrainStep(hg, hd, hf, lpips=model, weight_lpips=1.0, use_graph=True)
    with pytest.raises(ValueError, match='weight_lpips'):
        TrainStep(hg, hd, hf, weight_lpips=1.0)
    TrainStep(hg, hd, hf, use_graph=True)                                   # weight 0: the graph path is untouched
    common = dict(scale_factor=4, num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32,
                  hr_width=32, sample_interval=1)
    train, test = _loaders(7)
    net = T.SRADSGAN(T.default_args(n_residual_blocks=1, n_basic_blocks=1, weight_lpips=0.5, **common), train_loader=train,
                     test_loader=test)
    with pytest.raises(ValueError, match='lpips_alexnet'):                  # no weights loaded: refused when the step is built
        net.train()
    with pytest.raises(ValueError, match='weight_lpips'):
        T.SRADSGAN(T.default_args(weight_lpips=-1.0, **common))
    with pytest.raises(NotImplementedError, match='LPIPS'):
        drcan.DRCAN(drcan.default_args(n_resgroups=2, n_resblocks=1, weight_lpips=0.5, **common))


def _loaders(seed):
    g = torch.Generator().manual_seed(seed)
    train = [torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    hr = torch.rand(2, 3, 32, 32, generator=g)
    return train, [(F.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]


@pytest.mark.parametrize('which', ['sradsgan', 'sragan'])
def test_trainers_train_one_epoch_with_the_lpips_term(model, tmp_path, which):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import sragan
    common = dict(scale_factor=4, num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32,
                  hr_width=32, sample_interval=1, n_residual_blocks=1, n_basic_blocks=1, weight_lpips=0.5)
    cls, args = (T.SRADSGAN, T.default_args(**common)) if which == 'sradsgan' else (sragan.SRAGAN, sragan.default_args(**common))
    train, test = _loaders(7)
    net = cls(args, train_loader=train, test_loader=test)
    net.set_lpips(model)
    hist = net.train()
    assert net.step.lpips is model and net.step.weight_lpips == 0.5
    assert len(hist) == 1 and all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas', 'lpips')]))
    lines = open(os.path.join(str(tmp_path), 'loss_log.txt')).read().splitlines()
    assert len(lines) == 2 and all('lpips: ' in ln for ln in lines), lines
    assert all(float(ln.split('lpips: ')[1].split()[0]) > 0 for ln in lines)
    assert os.path.exists(os.path.join(str(tmp_path), 'model', 'generator_param_epoch_1.pkl'))
