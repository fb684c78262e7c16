"""The contrastive VGG19 losses on the device (sradsgan_amd/contrast.py, csrc/contrast.hip, TrainStep's weight_contrast) against ATen's
max pool, exact float64 sums on a 16-bit grid, and fp64 autograd of tests/contrast_ref.py.

Bounds.  Pool: bit-equal, on a coarse grid so that ties occur.  L1 forward: the inputs lie on a 16-bit grid, every |a - x| and every
partial sum is exact in float64, so the means equal torch's fp64 means to 4 ulp (one division) and alpha, beta to 4 ulp after the few
float64 operations of the ratio; the float32 loss is that value rounded once.  L1 backward: 8 * 2^-24 * (|alpha| + sum |beta_j|) * |up|
per element.  Cosine passes and the fp32 end-to-end gradient: the device runs the restatement's arithmetic in fp32 in another order, so
the bar is 8 x the largest error of the restatement's own fp32 CPU run (test_lpips_gpu._bar's multiple), for the kernels with the floor
2e-6 max|ref|.  End to end a ReLU or an arg-max may flip between two fp32 runs: at most 1e-4 of the elements may lie beyond the bar.
The L1 forms' own kink is kept away by the choice of the inputs (tools/make_golden_contrast.py; re-asserted here).  bf16x3: the relative
2-norm distance from fp64 against 4 x that of the restatement in fp32 with every conv and its data gradient through conv_emulation's
split-bf16 contraction.

Every test prints its figures before it asserts."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O
from tests import contrast_ref as R
from tests import gan_options_ref as GR
from tests.parity_util import build_pair, grad_score

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CL = torch.channels_last
EPS64 = 2.0 ** -52
UP = 0.375
B = 2


def dev(t):
    return t.to(DEV).contiguous(memory_format=CL) if t.dim() == 4 else t.to(DEV)


# ---- the floor-mode pool ------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('shape', [(1, 3, 3, 64), (2, 5, 7, 128), (1, 27, 27, 512), (2, 13, 13, 512), (1, 2, 3, 64)])
def test_floor_pool_is_bit_equal_to_aten(shape):
    """x on a grid of quarters in [-2, 2] (built from hash16's 16-bit grid), so windows tie and the first maximum must win; dy and the
    residual on the 16-bit grid, so the fused sums are exact."""
    from sradsgan_amd import contrast as C
    n, h, w, c = shape
    x = (torch.round(R.hash16(n * c * h * w, 7 + h) * 16) / 4).float().reshape(n, c, h, w)
    ho, wo = h // 2, w // 2
    dy = R.hash16(n * c * ho * wo, 11 + h).float().reshape(n, c, ho, wo)
    res = R.hash16(n * c * h * w, 13 + h).float().reshape(n, c, h, w)
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    y.backward(dy)
    want = xr.grad
    windows = F.unfold(x, 2, stride=2).reshape(n, c, 4, -1)
    ties = int(((windows == windows.max(2, keepdim=True).values).sum(2) > 1).sum())
    got_y = C.max_pool2x2_floor_raw(dev(x)).cpu()
    got = C.max_pool2x2_floor_bwd_raw(dev(x), dev(dy)).cpu()
    masked = C.max_pool2x2_floor_bwd_raw(dev(x), dev(dy), relu=True).cpu()
    fused = C.max_pool2x2_floor_bwd_raw(dev(x), dev(dy), relu=True, residual=dev(res)).cpu()
    print('floor pool %s: %d of %d windows tie, %d inputs take a gradient' % (shape, ties, windows.shape[-1] * n * c, int((want != 0).sum())))
    assert ties > 0
    assert torch.equal(got_y, y.detach())
    assert torch.equal(got, want)
    if h % 2:
        assert bool((got[:, :, h - 1] == 0).all())                             # the odd last row belongs to no window
    if w % 2:
        assert bool((got[:, :, :, w - 1] == 0).all())
    assert torch.equal(masked, want * (x > 0))
    assert torch.equal(fused, want * (x > 0) + res)
    with pytest.raises(ValueError):
        C.max_pool2x2_floor_bwd_raw(dev(x), torch.zeros(n, c, ho, wo + 1, device=DEV))


# ---- the distance kernels on their own ---------------------------------------------------------------------------------------------- #
def _tap(n_neg, c, h, w, salt):
    """[(2 + n_neg) B, C, h, w] features on a 16-bit grid (ReLU outputs, about 40 % zeros): the last negative equals the anchor, sample
    0's first 8 channels are equal in every operand, sample 0's anchor pixel (0, 0) and sample 1's positive pixel (h-1, w-1) are zero."""
    m = (2 + n_neg) * B
    f = (F.relu(R.hash16(m * c * h * w, salt) + 0.125) * 3).float().reshape(m, c, h, w)
    f[0, :, 0, 0] = 0
    f[(1 + n_neg) * B:] = f[:B]
    for k in range(1, 2 + n_neg):
        f[k * B, :8] = f[0, :8]
    f[B + 1, :, h - 1, w - 1] = 0
    return f


def _split(f, n_neg):
    return f[:B], [f[(k + 1) * B:(k + 2) * B] for k in range(1 + n_neg)]


CASES = [(c, hw, n) for c in (64, 128, 512) for hw in ((1, 1), (3, 5), (13, 13)) for n in (1, 3)]
IDS = ['C%d-%dx%d-N%d' % (c, hw[0], hw[1], n) for c, hw, n in CASES]


@pytest.mark.parametrize('c,hw,n_neg', CASES, ids=IDS)
def test_l1_forward_and_finish(c, hw, n_neg):
    from sradsgan_amd import contrast as C
    h, w = hw
    kops = 1 + n_neg
    f = _tap(n_neg, c, h, w, c + h + n_neg)
    a, xs = _split(f, n_neg)
    count = B * c * h * w
    partial = torch.empty(5, kops, C.l1_parts(), device=DEV, dtype=torch.float64)
    for t in range(5):
        C.contrast_l1_fwd_raw(dev(f), kops, partial[t])
    got = (partial[0].sum(-1) / count).cpu()
    want = torch.stack([(a.double() - x.double()).abs().mean() for x in xs])
    rel = float(((got - want).abs() / want.clamp_min(1e-300)).max())
    print('l1 fwd C=%d %dx%d N=%d: means %s, worst relative difference %.2e (4 ulp = %.2e)' % (c, h, w, n_neg, got.tolist(), rel, 4 * EPS64))
    assert float(want[-1]) == 0.0 and float(got[-1]) == 0.0                    # the negative that equals the anchor
    assert bool(((got - want).abs() <= 4 * EPS64 * want).all()) and float(want[0]) > 0
    assert torch.equal(partial[0], partial[4])
    for ablation in (False, True):
        loss, coef = C.contrast_l1_finish_raw(partial, [count] * 5, ablation)
        dap, dan = float(want[0]), sum(float(v) for v in want[1:])
        den = dan + 1e-7
        ratio = dap if ablation else dap / den
        ref = sum(wt * ratio for wt in R.WEIGHTS)
        alpha = torch.tensor([wt / count if ablation else wt / (count * den) for wt in R.WEIGHTS], dtype=torch.float64)
        beta = torch.tensor([0.0 if ablation else wt * dap / (count * den * den) for wt in R.WEIGHTS], dtype=torch.float64)
        coef = coef.cpu()
        print('   ablation=%s: loss %.9g (fp64 %.17g), alpha[4] %.17g (ref %.17g), beta[4] %.17g (ref %.17g)' % (
            ablation, float(loss), float(ref), float(coef[4, 0]), float(alpha[4]), float(coef[4, 1]), float(beta[4])))
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert abs(float(loss) - float(ref)) <= (2.0 ** -24 + 4 * EPS64) * abs(float(ref))
        assert bool(((coef[:, 0] - alpha).abs() <= 4 * EPS64 * alpha.abs()).all())
        for k in range(1, kops):
            assert bool(((coef[:, k] - beta).abs() <= 4 * EPS64 * beta.abs()).all())


@pytest.mark.parametrize('c,hw,n_neg', CASES, ids=IDS)
def test_l1_backward(c, hw, n_neg):
    from sradsgan_amd import contrast as C
    h, w = hw
    kops = 1 + n_neg
    f = _tap(n_neg, c, h, w, 2 * c + h + n_neg)
    a, xs = _split(f, n_neg)
    coef = torch.tensor([0.37 / (1 + 0.3 * k) * (1 if k % 2 == 0 else 1.7) for k in range(kops)], dtype=torch.float64)
    up = torch.tensor(UP, device=DEV)
    got = C.contrast_l1_bwd_raw(dev(f), kops, coef.to(DEV), up).cpu()
    again = C.contrast_l1_bwd_raw(dev(f), kops, coef.to(DEV), up).cpu()
    s = coef[0] * torch.sign(a.double() - xs[0].double())
    for k in range(1, kops):
        s = s - coef[k] * torch.sign(a.double() - xs[k].double())
    ref = torch.where(a > 0, UP * s, torch.zeros_like(s))
    bound = 8 * 2.0 ** -24 * float(coef.abs().sum()) * UP
    err = float((got.double() - ref).abs().max())
    print('l1 bwd C=%d %dx%d N=%d: err %.2e, bound %.2e, max|ref| %.2e' % (c, h, w, n_neg, err, bound, float(ref.abs().max())))
    assert tuple(got.shape) == (B, c, h, w) and float(ref.abs().max()) > 0
    assert err <= bound
    assert bool((got[a <= 0] == 0).all())                                      # through the ReLU: exact zeros
    assert bool((got[0, :8] == 0).all())                                       # the anchor equals every operand: sign(0) = 0
    assert torch.equal(got, again)


def _cos_terms(m, n_form, ablation):
    """[B] terms of one tap from the means m [B, kops] (float64)."""
    e = (m / R.T).exp()
    if n_form:
        return -torch.log(e[:, 0] / (e[:, 1:].sum(1) + e[:, 0]))
    if ablation:
        return -torch.log(e[:, 0])
    return -torch.log(e[:, 0] / (e[:, 1] + 1e-7))


def _bar(ref, ref32):
    e32 = float((ref32.double() - ref).abs().max())
    return max(8 * e32, 2e-6 * float(ref.abs().max())), e32


@pytest.mark.parametrize('c,hw,n_neg', CASES, ids=IDS)
def test_cosine_forward_and_finish(c, hw, n_neg):
    from sradsgan_amd import contrast as C
    h, w = hw
    kops = 1 + n_neg
    f = _tap(n_neg, c, h, w, 3 * c + h + n_neg)
    a, xs = _split(f, n_neg)
    partial = torch.empty(5, B, kops, C.cos_parts(), device=DEV, dtype=torch.float64)
    for t in range(5):
        C.contrast_cos_fwd_raw(dev(f), kops, partial[t])
    got = (partial[0].sum(-1) / (h * w)).cpu()                                  # [B, kops]
    ref = torch.stack([R.cos(a.double(), x.double()).mean((1, 2)) for x in xs], 1)
    ref32 = torch.stack([R.cos(a, x).mean((1, 2)) for x in xs], 1)
    bar, e32 = _bar(ref, ref32)
    err = float((got - ref).abs().max())
    print('cos fwd C=%d %dx%d N=%d: err %.2e, bar %.2e (CPU fp32 %.2e), err / bar %.3f' % (c, h, w, n_neg, err, bar, e32, err / bar))
    assert torch.isfinite(got).all() and err <= bar
    assert abs(float(got[1, -1]) - 1.0) <= bar                                  # the negative that equals the anchor (sample 1: no zero pixel)
    assert torch.equal(partial[0], partial[4])
    forms = [(True, False)] + ([(False, False), (False, True)] if n_neg == 1 else [])
    for n_form, ablation in forms:
        loss, gamma = C.contrast_cos_finish_raw(partial, [h * w] * 5, n_form, ablation)
        m = got.clone().requires_grad_(True)
        val = sum(wt * _cos_terms(m, n_form, ablation) for wt in R.WEIGHTS).mean()
        per_tap = [torch.autograd.grad((wt * _cos_terms(m, n_form, ablation)).mean(), m)[0] for wt in R.WEIGHTS]
        gref = torch.stack(per_tap)
        gerr = float((gamma.cpu() - gref).abs().max())
        print('   N form=%s ablation=%s: loss %.9g (fp64 of the device means %.12g), gamma err %.2e of %.2e' % (
            n_form, ablation, float(loss), float(val), gerr, float(gref.abs().max())))
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert abs(float(loss) - float(val)) <= (2.0 ** -24 + 64 * EPS64) * max(abs(float(val)), 1.0)
        assert gerr <= 1e-12 * float(gref.abs().max())
    if n_neg == 3:
        with pytest.raises(RuntimeError):                                       # the single-negative form takes one negative
            C.contrast_cos_finish_raw(partial, [h * w] * 5, False, False)


@pytest.mark.parametrize('c,hw,n_neg', CASES, ids=IDS)
def test_cosine_backward(c, hw, n_neg):
    from sradsgan_amd import contrast as C
    h, w = hw
    kops = 1 + n_neg
    f = _tap(n_neg, c, h, w, 5 * c + h + n_neg)
    a, xs = _split(f, n_neg)
    gamma = (R.hash16(B * kops, 40 + c) * 4).reshape(B, kops)
    up = torch.tensor(UP, device=DEV)
    got = C.contrast_cos_bwd_raw(dev(f), kops, gamma.to(DEV), up).cpu()
    again = C.contrast_cos_bwd_raw(dev(f), kops, gamma.to(DEV), up).cpu()

    def autograd(dt):
        pre = a.to(dt).clone().requires_grad_(True)
        fr = torch.relu(pre)
        val = UP * sum((gamma[:, k].to(dt) * R.cos(fr, xs[k].to(dt)).mean((1, 2))).sum() for k in range(kops))
        return torch.autograd.grad(val, pre)[0]
    ref, ref32 = autograd(torch.float64), autograd(torch.float32)
    bar, e32 = _bar(ref, ref32)
    err = float((got.double() - ref).abs().max())
    print('cos bwd C=%d %dx%d N=%d: err %.2e, bar %.2e (CPU fp32 %.2e, max|ref| %.2e), err / bar %.3f' % (
        c, h, w, n_neg, err, bar, e32, float(ref.abs().max()), err / bar))
    assert tuple(got.shape) == (B, c, h, w) and float(ref.abs().max()) > 0
    assert torch.isfinite(got).all()
    assert bool((got[a <= 0] == 0).all()) and bool((got[0, :, 0, 0] == 0).all())   # through the ReLU; the zero-norm anchor pixel
    assert err <= bar
    assert torch.equal(got, again)


def test_cosine_gradient_of_a_sample_does_not_depend_on_the_batch():
    """Forward, finish and backward for the batch of two and for each sample alone: gamma carries 1 / B, so the gradient alone is
    exactly B x the gradient in the batch."""
    from sradsgan_amd import contrast as C
    c, h, w, n_neg = 128, 3, 5, 3
    kops = 1 + n_neg
    f = _tap(n_neg, c, h, w, 77)
    up = torch.tensor(UP, device=DEV)

    def run(ft):
        b = ft.shape[0] // (kops + 1)
        partial = torch.empty(5, b, kops, C.cos_parts(), device=DEV, dtype=torch.float64)
        for t in range(5):
            C.contrast_cos_fwd_raw(dev(ft), kops, partial[t])
        _, gamma = C.contrast_cos_finish_raw(partial, [h * w] * 5, True, False)
        return C.contrast_cos_bwd_raw(dev(ft), kops, gamma[4].contiguous(), up).cpu(), gamma.cpu()
    both, gamma = run(f)
    for s in range(B):
        alone, g1 = run(f[s::B].contiguous())
        print('sample %d: gamma alone / in the batch %s' % (s, (g1[4, 0] / gamma[4, s]).tolist()))
        assert torch.equal(g1[:, 0], gamma[:, s] * B)
        assert torch.equal(alone[0], both[s] * B) and float(alone.abs().max()) > 0


def test_cosine_backward_keeps_a_nan_in_its_pixel():
    from sradsgan_amd import contrast as C
    f = _tap(1, 64, 3, 5, 5)
    f[1, 3, 1, 2] = float('nan')
    gamma = torch.ones(B, 2, dtype=torch.float64, device=DEV)
    got = C.contrast_cos_bwd_raw(dev(f), 2, gamma, torch.tensor(1.0, device=DEV)).cpu()
    bad = torch.isnan(got)
    assert bool(bad[1, 3, 1, 2]) and int(bad[0].sum()) == 0
    bad[1, :, 1, 2] = False
    assert int(bad.sum()) == 0
    partial = torch.empty(B, 2, C.cos_parts(), device=DEV, dtype=torch.float64)
    sums = C.contrast_cos_fwd_raw(dev(f), 2, partial).sum(-1).cpu()
    assert torch.isnan(sums[1]).all() and torch.isfinite(sums[0]).all()         # NaN in, NaN out: that sample's means, no other's


# ---- end to end --------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope='module')
def G():
    return np.load(R.GOLDEN)


@pytest.fixture(scope='module')
def vgg():
    from sradsgan_amd.contrast import Vgg19Taps
    net = Vgg19Taps()
    net.load_torchvision_vgg19(R.vgg19_state_dict())
    return net.to(DEV)


@pytest.fixture(scope='module')
def losses(vgg):
    from sradsgan_amd import contrast as C
    return {k: getattr(C, k)(vgg=vgg) for k in R.KINDS}


@pytest.fixture(scope='module')
def inputs(G):
    """name -> (a, p, n [B,3,3,H,W]); never modified."""
    return {'s%d' % i: tuple(torch.from_numpy(G['s%d_%s' % (i, k)]) for k in 'apn') for i in range(len(R.SHAPES))}


_REFS = {}


def _negatives(kind, n):
    return n if kind.startswith('N') else n[:, 0].contiguous()


def _reference(kind, name, inputs):
    """(fp64 loss, fp64 gradient, the fp32 CPU run's gradient) of a case; computed once, never modified."""
    if (kind, name) not in _REFS:
        a, p, n = inputs[name]
        val, g64 = R.loss_and_grad(kind, a, p, _negatives(kind, n))
        _, g32 = R.loss_and_grad(kind, a, p, _negatives(kind, n), dtype=torch.float32)
        _REFS[kind, name] = (val, g64, g32.double())
    return _REFS[kind, name]


def _loss_grad(loss, a, p, n):
    anchor = a.to(DEV).requires_grad_(True)
    pos, neg = p.to(DEV), n.to(DEV)
    val = loss(anchor, pos, neg)
    val.backward()
    assert pos.grad is None and neg.grad is None
    return val.detach().cpu(), anchor.grad.cpu()


@pytest.mark.parametrize('name', ['s0', 's1', 's2'])
def test_inputs_keep_their_margin(inputs, name):
    m = R.margins(*inputs[name])
    print('%s: per tap (smallest non-zero difference, largest fp32 feature error, sign flips) %s' % (name, m))
    assert R.margins_hold(m)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', ['s0', 's1', 's2'])
def test_fp32_loss_and_gradient_end_to_end(losses, inputs, name, kind):
    from sradsgan_amd import ops
    a, p, n = inputs[name]
    val, g64, g32 = _reference(kind, name, inputs)
    with ops.conv_math('fp32'):
        got_val, got = _loss_grad(losses[kind], a, p, _negatives(kind, n))
    e32 = float((g32 - g64).abs().max())
    bar = 8 * e32
    gmax = float(g64.abs().max())
    err = (got.double() - g64).abs()
    share = float((err > bar).double().mean())
    rel = abs(float(got_val) - float(val)) / abs(float(val))
    print('%s %s fp32: loss %.7g (fp64 %.10g, relative difference %.2e); max|g| %.3e, CPU fp32 error %.2e (%.2e of max|g|), bar %.2e; '
          'gpu worst %.2e, share beyond the bar %.2e, relative 2-norm distance %.2e' % (
              name, kind, float(got_val), float(val), rel, gmax, e32, e32 / gmax, bar, float(err.max()), share,
              float((got.double() - g64).norm() / g64.norm())))
    assert got_val.dtype == torch.float32 and got_val.dim() == 0 and tuple(got.shape) == tuple(a.shape)
    assert rel <= 1e-5
    assert float(((g32 - g64).abs() > bar).double().mean()) == 0.0              # the fp32 CPU run has no element beyond the bar
    assert torch.isfinite(got).all() and gmax > 0
    assert share <= 1e-4


@pytest.mark.parametrize('kind', R.KINDS)
def test_ablation_end_to_end(vgg, inputs, kind):
    """ablation=True: the single-negative classes drop the negative, the N classes ignore the flag (as the reference does)."""
    from sradsgan_amd import contrast as C
    from sradsgan_amd import ops
    a, p, n = inputs['s2']
    neg = _negatives(kind, n)
    val, g64 = R.loss_and_grad(kind, a, p, neg, ablation=True)
    _, g32 = R.loss_and_grad(kind, a, p, neg, ablation=True, dtype=torch.float32)
    with ops.conv_math('fp32'):
        got_val, got = _loss_grad(getattr(C, kind)(ablation=True, vgg=vgg), a, p, neg)
    bar = 8 * float((g32.double() - g64).abs().max())
    share = float(((got.double() - g64).abs() > bar).double().mean())
    rel = abs(float(got_val) - float(val)) / abs(float(val))
    print('%s ablation: loss %.7g (fp64 %.10g, relative difference %.2e), share beyond the bar %.2e' % (kind, float(got_val), float(val), rel,
                                                                                                       share))
    assert rel <= 1e-5 and share <= 1e-4
    if not kind.startswith('N'):
        assert abs(float(val) - float(_reference(kind, 's2', inputs)[0])) > 1e-3 * abs(float(val))


@pytest.mark.parametrize('kind', R.KINDS)
def test_bf16x3_gradient_and_half_is_the_same_bits(losses, inputs, kind):
    from sradsgan_amd import ops
    a, p, n = inputs['s0']
    neg = _negatives(kind, n)
    _, g64, _ = _reference(kind, 's0', inputs)
    _, emu = R.loss_and_grad(kind, a, p, neg, dtype=torch.float32, conv=R.emulated_conv('bf16x3'))
    with ops.conv_math('bf16x3'):
        _, got = _loss_grad(losses[kind], a, p, neg)
    with ops.conv_math('half'):
        _, half = _loss_grad(losses[kind], a, p, neg)
        assert ops.get_conv_math() == 'half'
    e = float((emu.double() - g64).norm() / g64.norm())
    d = float((got.double() - g64).norm() / g64.norm())
    print('%s bf16x3: emulated run %.3e, gpu %.3e relative 2-norm distance from fp64; ratio %.3f' % (kind, e, d, d / e))
    assert d <= 4 * e
    assert torch.equal(half, got)


@pytest.mark.parametrize('kind', ['NContrastLoss', 'ContrastCosineLoss'])
def test_loss_node_contract(losses, inputs, kind):
    a, p, n = inputs['s0']
    loss = losses[kind]
    anchor = a.to(DEV).requires_grad_(True)
    pos, neg = p.to(DEV), _negatives(kind, n).to(DEV)
    val = loss(anchor, pos, neg)
    g, = torch.autograd.grad(val, anchor, create_graph=True)
    with pytest.raises(RuntimeError):                                           # once_differentiable: no double backward
        g.sum().backward()
    again, = torch.autograd.grad(loss(anchor, pos, neg), anchor)
    assert torch.equal(again, g.detach())                                       # deterministic
    scaled, = torch.autograd.grad(loss(anchor, pos, neg) * 0.25, anchor)        # the upstream gradient reaches the kernels
    assert bool(((scaled - 0.25 * again).abs() <= 2.0 ** -22 * again.abs()).all())
    with torch.no_grad():
        plain = loss(anchor, pos, neg)
    assert not plain.requires_grad and torch.equal(plain, val.detach())
    assert not loss(anchor.detach(), pos, neg).requires_grad
    with pytest.raises(ValueError, match='anchor only'):
        loss(anchor, pos.clone().requires_grad_(True), neg)
    with pytest.raises(ValueError, match='anchor only'):
        loss(anchor, pos, neg.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='one shape'):
        loss(anchor, pos[:, :, :-1], neg)
    with pytest.raises(ValueError, match='at least 16'):
        loss(anchor[:, :, :15], pos[:, :, :15], neg[..., :15, :])


# ---- the training step -------------------------------------------------------------------------------------------------------------- #
def _nets():
    s = GR.TRAIN_SHAPE
    (hg, hd, hf), (_, od, _) = build_pair(s['n_groups'], s['n_blocks'], s['scale'], DEV)
    GR.scaled_discriminator_init_(od, gain=GR.TRAIN_GAIN)
    hd.load_state_dict(od.state_dict(), strict=True)
    return hg, hd.to(DEV), hf


def _step_inputs():
    lr_img, hr_img = [t.to(DEV) for t in GR.case_inputs('train_small', 0)]
    bc = F.interpolate(lr_img, size=hr_img.shape[2:], mode='bicubic', align_corners=False)
    alpha = O.det_fill('contrast.alpha', (2, 1, 1, 1), 0.5, 0.5).to(DEV)
    return lr_img, hr_img, bc, alpha


@pytest.mark.parametrize('order,kind', [(dict(), 'ContrastLoss'), (dict(overlap_wgrad=False), 'ContrastLoss'),
                                        (dict(reuse_d_fake=False), 'ContrastLoss'), (dict(), 'ContrastCosineLoss')],
                         ids=['onewalk', 'shared', 'plain', 'onewalk-cosine'])
def test_step_adds_the_contrast_gradient_to_the_generator_alone(losses, order, kind, request):
    """HR tiles 32 x 32 (train_small's).  G's gradient with weight_contrast = 1 minus the one with weight 0 is the gradient of
    contrast(G(lr), hr, bc) through G alone (parity_util.grad_score < 5e-3, the project's bar for G); loss_G moves by the logged term;
    D's arena keeps its bits; every other logged scalar is unchanged."""
    from sradsgan_amd.train_step import TrainStep
    order_id = request.node.callspec.id.split('-')[0]
    model = losses[kind]
    lr_img, hr_img, bc, alpha = _step_inputs()
    res = {}
    for weight in (0.0, 1.0):
        hg, hd, hf = _nets()
        step = TrainStep(hg, hd, hf, clip_value=GR.GP_CLIP, contrast=model if weight else None, weight_contrast=weight, **order)
        taken = []
        for name in ('_compute_onewalk', '_compute_shared', '_compute_plain'):
            setattr(step, name, (lambda fn, name: lambda *a: (taken.append(name), fn(*a))[1])(getattr(step, name), name))
        out = step(lr_img, hr_img, alpha, negatives=bc) if weight else step(lr_img, hr_img, alpha)
        assert taken == ['_compute_' + order_id]
        torch.cuda.synchronize()
        res[weight] = (step.arena_G.flat_g.clone(), step.arena_D.flat_g.clone(), {k: float(v) for k, v in out.items() if v.dim() == 0},
                       hg, step)
    g0, d0, s0, _, _ = res[0.0]
    g1, d1, s1, hg1, step1 = res[1.0]
    assert 'contrast' not in s0 and 'contrast' in s1 and np.isfinite(s1['contrast'])
    assert torch.equal(d0, d1)
    assert abs((s1['loss_G'] - s0['loss_G']) - s1['contrast']) < 1e-3 * max(1.0, abs(s1['contrast']))
    for k in ('pixel', 'content', 'loss_gan', 'loss_D', 'gp'):
        assert s0[k] == s1[k], k
    ref_g = _nets()[0]
    direct = model(ref_g(lr_img), hr_img, bc)
    direct.backward()
    direct = float(direct.detach())
    step1.arena_G.flat_g.copy_(g1 - g0)                                         # hg1's .grad tensors are views of the arena
    score, worst = grad_score((hg1,), (ref_g.cpu(),))
    print('step %s %s: contrast %.6f (direct %.6f), G gradient difference vs the loss through G alone: score %.3e (%s)' % (
        order, kind, s1['contrast'], direct, score, worst))
    assert abs(direct - s1['contrast']) <= 1e-5 * abs(direct)
    assert float((g1 - g0).abs().max()) > 0 and score < 5e-3


def test_step_with_weight_zero_ignores_the_negatives():
    """weight_contrast = 0 (the default) with negatives passed: outputs, gradients and updated parameters of both nets equal, bit for
    bit, those of a step called without the keyword."""
    from sradsgan_amd.train_step import TrainStep
    lr_img, hr_img, bc, alpha = _step_inputs()
    res = []
    for with_kw in (False, True):
        hg, hd, hf = _nets()
        step = TrainStep(hg, hd, hf, clip_value=GR.GP_CLIP)
        out = step(lr_img, hr_img, alpha, negatives=bc) if with_kw else step(lr_img, hr_img, alpha)
        torch.cuda.synchronize()
        res.append((out, [t.clone() for t in (step.arena_G.flat_g, step.arena_D.flat_g, step.arena_G.flat_p, step.arena_D.flat_p)]))
    (o0, t0), (o1, t1) = res
    assert sorted(o0) == sorted(o1) and 'contrast' not in o1
    assert all(torch.equal(o0[k], o1[k]) for k in o0)
    assert all(torch.equal(x, y) for x, y in zip(t0, t1))


def _loaders(seed):
    g = torch.Generator().manual_seed(seed)
    train = [torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    hr = torch.rand(2, 3, 32, 32, generator=g)
    return train, [(F.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]


def test_step_and_trainers_refuse_what_they_cannot_run(losses, tmp_path):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import drcan
    from sradsgan_amd.train_step import TrainStep
    model = losses['ContrastLoss']
    hg, hd, hf = _nets()
    with pytest.raises(ValueError, match='use_graph'):
        TrainStep(hg, hd, hf, contrast=model, weight_contrast=1.0, use_graph=True)
    with pytest.raises(ValueError, match='needs contrast'):
        TrainStep(hg, hd, hf, weight_contrast=1.0)
    with pytest.raises(ValueError, match='weight_contrast must be >= 0'):
        TrainStep(hg, hd, hf, contrast=model, weight_contrast=-1.0)
    lr_img, hr_img, bc, alpha = _step_inputs()
    step = TrainStep(hg, hd, hf, contrast=model, weight_contrast=1.0)
    before = step.arena_G.flat_p.clone()
    with pytest.raises(ValueError, match='negatives'):
        step(lr_img, hr_img, alpha)
    assert torch.equal(before, step.arena_G.flat_p)                             # refused before anything ran
    common = dict(scale_factor=4, num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32,
                  hr_width=32, sample_interval=1)
    train, test = _loaders(7)
    net = T.SRADSGAN(T.default_args(n_residual_blocks=1, n_basic_blocks=1, weight_contrast=0.5, **common), train_loader=train,
                     test_loader=test)
    with pytest.raises(ValueError, match='contrast_vgg19'):                     # no weights loaded: refused when the step is built
        net.train()
    with pytest.raises(ValueError, match='weight_contrast'):
        T.SRADSGAN(T.default_args(weight_contrast=-1.0, **common))
    with pytest.raises(ValueError, match='contrast_loss'):
        T.SRADSGAN(T.default_args(weight_contrast=1.0, contrast_loss='l2', **common))
    with pytest.raises(NotImplementedError, match='contrastive'):
        drcan.DRCAN(drcan.default_args(n_resgroups=2, n_resblocks=1, weight_contrast=0.5, **common))


@pytest.mark.parametrize('which', ['sradsgan', 'sragan'])
def test_trainers_train_one_epoch_with_the_contrast_term(losses, tmp_path, which):
    """SRADSGAN with a model handed over (set_contrast), SRAGAN with args.contrast_vgg19 / contrast_loss='cosine' / contrast_ablation."""
    from sradsgan_amd import contrast as C
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import sragan
    common = dict(scale_factor=4, num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32,
                  hr_width=32, sample_interval=1, n_residual_blocks=1, n_basic_blocks=1, weight_contrast=0.5)
    train, test = _loaders(7)
    if which == 'sradsgan':
        net = T.SRADSGAN(T.default_args(**common), train_loader=train, test_loader=test)
        net.set_contrast(losses['ContrastLoss'])
    else:
        path = os.path.join(str(tmp_path), 'vgg19.pth')
        torch.save(R.vgg19_state_dict(), path)
        net = sragan.SRAGAN(sragan.default_args(contrast_loss='cosine', contrast_ablation=True, contrast_vgg19=path, **common),
                            train_loader=train, test_loader=test)
    hist = net.train()
    if which == 'sradsgan':
        assert net.step.contrast is losses['ContrastLoss']
    else:
        assert isinstance(net.step.contrast, C.ContrastCosineLoss) and net.step.contrast.ab
        assert torch.equal(net.step.contrast.vgg.conv(28).bias.cpu(), R.vgg19_state_dict()['features.28.bias'])
    assert net.step.weight_contrast == 0.5
    assert len(hist) == 1 and all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
    lines = open(os.path.join(str(tmp_path), 'loss_log.txt')).read().splitlines()
    assert len(lines) == 2 and all('contrast: ' in ln for ln in lines), lines
    assert all(np.isfinite(float(ln.split('contrast: ')[1].split()[0])) for ln in lines)
    assert os.path.exists(os.path.join(str(tmp_path), 'model', 'generator_param_epoch_1.pkl'))
