"""ESRGAN on the HIP path (sradsgan_amd.model.esrgan) against the reference's vectors (tests/golden/esrgan_*.npz) and the fp64 CPU
restatement (tests/esrgan_ref.py), in split-bf16 and exact-fp32 conv arithmetic: the criteria kernel, the discriminators' dense head
and the input normalisation (csrc/esrgan.hip) against fp64 with derived bounds; rrdb_step, RRDBNet, the four discriminators, the
perceptual extractor and two iterations of the step; the existing scene and self-ensemble entry points on the new generator."""
import functools

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import esrgan_ref as R
from tests.test_esrgan_cpu import case_tag, golden, ref_discriminator, ref_extractor, ref_generator

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MODES = ['bf16x3', 'fp32']
CL = torch.channels_last
U = 2.0 ** -24                        # unit roundoff of fp32


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def dev_nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def hip_generator(ref, scale, nb=2):
    from sradsgan_amd.model import esrgan as E
    G = E.RRDBNet(3, 3, 64, nb, upscale=scale)
    G.load_state_dict(ref.state_dict(), strict=True)
    return G.to(DEV)


def hip_discriminator(ref, size):
    from sradsgan_amd.model import esrgan as E
    D = E.DISCRIMINATORS[size](3, 64)
    D.load_state_dict(ref.state_dict(), strict=True)
    return D.to(DEV)


def hip_extractor(ref):
    from sradsgan_amd.model import esrgan as E
    Fx = E.VGGFeatureExtractor()
    Fx.load_state_dict(ref.state_dict(), strict=True)
    return Fx.to(DEV)


# ---- the criteria kernel ------------------------------------------------------------------------------------------------------- #

COUNTS = [1, 2, 63, 64, 65, 1000, 23328]          # 23 328 = 32 * 27 * 27, a patch discriminator's B h w


def _criteria_inputs(count):
    a = O.det_fill('gan.a.%d' % count, (count, 1), 4.0)
    b = O.det_fill('gan.b.%d' % count, (max(1, (count * 3) // 4), 1), 4.0, 0.5)      # its own count
    return a, b


def _criteria_torch(a, b, gan_type, label, relativistic, up):
    """(value, da, db) of torch's own composition (sradsgan.py:56-67, :843) in a's dtype"""
    loss = torch.nn.BCEWithLogitsLoss() if gan_type == 'vanilla' else torch.nn.MSELoss()
    a, b = a.clone().requires_grad_(), b.clone().requires_grad_()
    x = a - torch.mean(b) if relativistic else a
    v = loss(x, torch.empty_like(x).fill_(label))
    (v * up).backward()
    return v.detach(), a.grad, b.grad if relativistic else None


def _criteria_hip(a, b, gan_type, label, relativistic, up):
    from sradsgan_amd.model import esrgan as E
    a, b = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    v = E._GanLoss.apply(a, b if relativistic else None, E.GAN_MODES[gan_type], label, relativistic)
    (v * up).backward()
    torch.cuda.synchronize()
    return v.detach().cpu(), a.grad.cpu(), b.grad.cpu() if relativistic else None


@pytest.mark.parametrize('gan_type', ['vanilla', 'lsgan'])
@pytest.mark.parametrize('count', COUNTS)
def test_criteria_kernel_matches_fp64_within_the_bar_of_torch_fp32(count, gan_type):
    """value and gradients against the fp64 restatement.  The bar is max(4 e_ref, 2^-21 |value|), e_ref the error of torch's own fp32
    CPU evaluation of the same composition against the same fp64 numbers (factor 4: device exp / log1p may differ from libm by a
    few ulp); for a gradient tensor both errors and |value| are maxima over the tensor."""
    a, b = _criteria_inputs(count)
    up = 3.0
    worst = 0.0
    for relativistic in (False, True):
        for label in (1.0, 0.0, 0.9):
            a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
            x64 = a64 - b64.mean() if relativistic else a64
            v64 = R.criterion(x64, True, gan_type, real_label_val=label)
            (v64 * up).backward()
            want = (v64.detach(), a64.grad, b64.grad if relativistic else None)
            ref32 = _criteria_torch(a, b, gan_type, label, relativistic, up)
            got = _criteria_hip(a, b, gan_type, label, relativistic, up)
            assert got[0].dim() == 0 and got[0].dtype == torch.float32
            for name, g, r32, w in zip(('value', 'da', 'db'), got, ref32, want):
                if w is None:
                    assert g is None
                    continue
                e_ref = float((r32.double() - w).abs().max())
                err = float((g.double() - w).abs().max())
                bar = max(4 * e_ref, 2.0 ** -21 * float(w.abs().max()))
                worst = max(worst, err / bar if bar > 0 else (0.0 if err == 0 else float('inf')))
                assert err <= bar, (name, relativistic, label, err, bar, e_ref)
    print('criteria %s count %d: worst error / bar = %.3f' % (gan_type, count, worst))


@pytest.mark.parametrize('gan_type', ['vanilla', 'lsgan'])
def test_criteria_kernel_extremes_nan_and_repeatability(gan_type):
    from sradsgan_amd.model import esrgan as E
    a = torch.tensor([[-100.0], [100.0], [0.0], [3.0]])
    b = torch.tensor([[100.0], [-100.0], [1.0]])
    for relativistic in (False, True):
        for label in (1.0, 0.0):
            v, da, db = _criteria_hip(a, b, gan_type, label, relativistic, 1.0)
            assert torch.isfinite(v) and torch.isfinite(da).all() and (db is None or torch.isfinite(db).all())
            v2, da2, db2 = _criteria_hip(a, b, gan_type, label, relativistic, 1.0)
            assert torch.equal(v, v2) and torch.equal(da, da2) and (db is None or torch.equal(db, db2))        # equal bits
    bad = a.clone()
    bad[2] = float('nan')
    assert torch.isnan(_criteria_hip(bad, b, gan_type, 1.0, False, 1.0)[0])
    assert torch.isnan(_criteria_hip(a, torch.tensor([[float('nan')], [1.0]]), gan_type, 1.0, True, 1.0)[0])     # through mean(b)
    big = O.det_fill('gan.rep', (23328, 1), 4.0)
    r1, r2 = (_criteria_hip(big, big.flip(0), gan_type, 0.9, True, 2.0) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(r1, r2))
    # the public ops: pairs of the relativistic form, plain criterion, and the wgan-gp means
    real, fake = O.det_fill('gan.real', (6, 1), 2.0), O.det_fill('gan.fake', (6, 1), 2.0)
    for fn_hip, fn_ref in ((E.ragan_pair_d, R.ragan_d), (E.ragan_pair_g, R.ragan_g)):
        r, f = real.to(DEV).requires_grad_(), fake.to(DEV).requires_grad_()
        fn_hip(r, f, gan_type).backward()
        r64, f64 = real.double().requires_grad_(), fake.double().requires_grad_()
        v64 = fn_ref(r64, f64, gan_type)
        v64.backward()
        assert abs(float(fn_hip(r, f, gan_type)) - float(v64)) < 1e-6 * max(1.0, abs(float(v64)))
        assert rel_err(f.grad, f64.grad) < 1e-6
        if fn_hip is E.ragan_pair_g:
            assert r.grad is None and r64.grad is None           # the real predictions are detached: the gradient goes to pred_fake only
        else:
            assert rel_err(r.grad, r64.grad) < 1e-6
    crit = E.GANLoss(gan_type, 0.9, 0.1)
    for is_real in (True, False):
        assert abs(float(crit(real.to(DEV), is_real)) - float(R.criterion(real.double(), is_real, gan_type, 0.9, 0.1))) < 1e-6
        assert abs(float(E.GANLoss('wgan-gp')(real.to(DEV), is_real)) - float(R.criterion(real.double(), is_real, 'wgan-gp'))) < 1e-6


# ---- the dense head -------------------------------------------------------------------------------------------------------------- #

HEAD_CASES = [(1, 512, 3), (2, 512, 4), (5, 512, 3), (33, 512, 4), (2, 64, 1), (3, 64, 2)]


def _head_tensors(B, C, S, H=100):
    K = C * S * S
    tag = 'dhead.%d.%d.%d' % (B, C, S)
    return (O.det_fill(tag + '.x', (B, C, S, S), 1.0), O.det_fill(tag + '.w0', (H, K), 0.05), O.det_fill(tag + '.b0', (H,), 0.1),
            O.det_fill(tag + '.w1', (1, H), 0.3), O.det_fill(tag + '.b1', (1,), 0.1), O.det_fill(tag + '.dy', (B, 1), 1.0))


def _head_hip(x, w0, b0, w1, b1, dy):
    from sradsgan_amd.model import esrgan as E
    leaves = [dev_nhwc(x).requires_grad_()] + [t.to(DEV).requires_grad_() for t in (w0, b0, w1, b1)]
    y = E.dhead(*leaves)
    hidden = y.grad_fn.saved_tensors[1]
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return [y.detach().cpu(), hidden.detach().cpu()] + [t.grad.cpu() for t in leaves]


@pytest.mark.parametrize('B,C,S', HEAD_CASES)
def test_head_matches_fp64_within_the_summation_bound(B, C, S):
    """|s - s64| <= (n + 2) 2^-24 sum |terms| for an fp32 sum of n products in any order, plus what the operands' own errors
    contribute: derived, not measured.  hidden: n = K, and the LeakyReLU adds one rounding and the fp32 value of the slope (0.2f is
    0.2 (1 + 0.25 u)): 2 u |h|; y: n = H, its operand hidden carries e_h; dz = dy w1 mask: two roundings and the slope's 0.25 u;
    dw1, db1: n = B; db0, dw0: n = B and dx: n = H, with dz's 2.25 u folded into the factor (n + 5)."""
    from sradsgan_amd import ops
    x, w0, b0, w1, b1, dy = _head_tensors(B, C, S)
    K, H = C * S * S, 100
    with ops.conv_math('fp32'):
        got = _head_hip(x, w0, b0, w1, b1, dy)
        again = _head_hip(x, w0, b0, w1, b1, dy)
    with ops.conv_math('bf16x3'):
        other = _head_hip(x, w0, b0, w1, b1, dy)
    for u, v, w in zip(got, again, other):
        assert torch.equal(u, v) and torch.equal(u, w)             # equal bits run to run and in both conv modes
    y, hidden, dx, dw0, db0, dw1, db1 = [t.double() for t in got]
    x64, w064, b064, w164, b164, dy64 = [t.double() for t in (x, w0, b0, w1, b1, dy)]
    xf = x64.flatten(1)                                            # NCHW order, as the reference's view
    z64 = xf @ w064.t() + b064
    h64 = torch.where(z64 > 0, z64, 0.2 * z64)
    y64 = h64 @ w164.t() + b164
    e_h = (K + 2) * U * (xf.abs() @ w064.abs().t() + b064.abs()) + 2 * U * h64.abs()
    assert bool(((hidden - h64).abs() <= e_h).all()), float(((hidden - h64).abs() / e_h).max())
    e_y = (H + 2) * U * (h64.abs() @ w164.abs().t() + b164.abs()) + e_h @ w164.abs().t()
    assert bool(((y - y64).abs() <= e_y).all()), float(((y - y64).abs() / e_y).max())
    dz64 = dy64 * w164 * torch.where(z64 > 0, 1.0, 0.2)            # [B, H]
    checks = [('dw1', dw1, dy64.t() @ h64, (B + 2) * U * (dy64.abs().t() @ h64.abs()) + dy64.abs().t() @ e_h),
              ('db1', db1, dy64.sum(0), (B + 2) * U * dy64.abs().sum(0)),
              ('db0', db0, dz64.sum(0), (B + 5) * U * dz64.abs().sum(0)),
              ('dw0', dw0, dz64.t() @ xf, (B + 5) * U * (dz64.abs().t() @ xf.abs())),
              ('dx', dx.flatten(1), dz64 @ w064, (H + 5) * U * (dz64.abs() @ w064.abs()))]
    worst = {}
    for name, g, want, bound in checks:
        err = (g.reshape(want.shape) - want).abs()
        worst[name] = float((err / bound.clamp_min(1e-300)).max())
        assert bool((err <= bound).all()), (name, worst[name])
    print('head B %d C %d S %d: worst error / bound %s' % (B, C, S, {k: round(v, 3) for k, v in worst.items()}))


@pytest.mark.parametrize('C,S', [(512, 4), (512, 3), (64, 2)])
def test_head_reads_the_nchw_flatten_order_index_for_index(C, S):
    """x[b, c, p] = k + 10000 b with k = c S S + p (exact in fp32) and weight row j one-hot at k_j: hidden[b, j] must be x's value at
    flat index k_j of the NCHW view."""
    from sradsgan_amd.model import esrgan as E
    B, H, K = 2, 100, C * S * S
    x = (torch.arange(K, dtype=torch.float32).view(1, C, S, S) + 1.0 + 10000.0 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1))
    ks = [(j * 83 + 7) % K for j in range(H)]
    w0 = torch.zeros(H, K)
    w0[torch.arange(H), torch.tensor(ks)] = 1.0
    y = E.dhead(dev_nhwc(x).requires_grad_(), w0.to(DEV), torch.zeros(H, device=DEV), torch.ones(1, H, device=DEV), torch.zeros(1, device=DEV))
    hidden = y.grad_fn.saved_tensors[1].cpu()
    assert torch.equal(hidden, x.flatten(1)[:, ks])


# ---- the input normalisation ----------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('shape', [(2, 3, 96, 96), (1, 3, 7, 5), (3, 3, 1, 1)])
def test_input_normalisation_is_exact(shape):
    from sradsgan_amd.model import esrgan as E
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    x, g = O.det_fill('norm.x', shape, 0.5, 0.5), O.det_fill('norm.g', shape, 1.0)
    xl = dev_nhwc(x).requires_grad_()
    y = E.input_norm(xl, mean.to(DEV), std.to(DEV))
    y.backward(dev_nhwc(g))
    assert torch.equal(y.detach().cpu(), (x - mean) / std)          # IEEE subtraction and division: the same bits
    assert torch.equal(xl.grad.cpu(), g / std)


# ---- rrdb_step ------------------------------------------------------------------------------------------------------------------- #

@functools.lru_cache(maxsize=None)
def _rrdb_reference():
    blk = O.det_init_(R.Rrdb(), prefix='rrdb.')
    blk64 = blk.double()
    x = O.det_fill('rrdb.x', (2, 64, 13, 11), 1.0)
    r = O.det_fill('rrdb.r', (2, 64, 13, 11), 1.0)
    x64 = x.double().requires_grad_()
    y64 = blk64(x64)
    (y64 * r.double()).sum().backward()
    return blk64, x, r, y64.detach(), x64.grad, {k: p.grad for k, p in blk64.named_parameters()}


@pytest.mark.parametrize('mode', MODES)
def test_rrdb_step_matches_fp64_and_chaining_keeps_the_bits(mode):
    from sradsgan_amd import ops
    from sradsgan_amd.model import esrgan as E
    blk64, x, r, y64, dx64, refg = _rrdb_reference()
    hip = E.RRDB(64)
    hip.load_state_dict({k: v.float() for k, v in blk64.state_dict().items()}, strict=True)
    hip.to(DEV)
    tol = 1e-5 if mode == 'fp32' else 1e-4
    with ops.conv_math(mode):
        xl = dev_nhwc(x).requires_grad_()
        y = hip(xl, chain=True)                                     # the result lands in a dense-block buffer
        (y * r.to(DEV)).sum().backward()
        assert y.stride()[3] == 192 and y._srhip_dense_buf.data_ptr() == y.data_ptr()
        fills = ops.dense_stats.fills
        with torch.no_grad():
            y2 = hip(y, chain=False)                                # (y itself: the buffer tag does not survive detach())
        assert ops.dense_stats.fills == fills                       # the next block adopts the buffer instead of copying
        plain = hip(dev_nhwc(x), chain=False)
        assert plain.stride()[3] == 64
        assert torch.equal(plain.cpu(), y.detach().cpu())           # chained and unchained: equal bits
        assert torch.equal(hip(plain.detach(), chain=False).cpu(), y2.cpu())
    assert rel_err(y, y64) < tol and rel_err(xl.grad, dx64) < tol
    for k, p in hip.named_parameters():
        assert rel_err(p.grad, refg[k]) < 10 * tol, k


def _aten_names(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages() if e.key.startswith('aten::')}


BANNED = ('aten::cat', 'aten::upsample_nearest', 'aten::_upsample_nearest', 'aten::leaky_relu')


def test_rrdb_chain_and_generator_run_no_aten_cat_upsample_leaky_relu_or_add():
    from sradsgan_amd.model import esrgan as E
    ref = ref_generator(4)
    G = hip_generator(ref, 4)
    x = dev_nhwc(O.det_fill('rrdb.prof.x', (2, 64, 12, 10), 1.0))
    g = dev_nhwc(O.det_fill('rrdb.prof.g', (2, 64, 12, 10), 1.0))
    blocks = G.rrdbs

    def chain():
        xl = x.clone().requires_grad_()
        t = xl
        for k, blk in enumerate(blocks):
            t = blk(t, chain=k < len(blocks) - 1)
        t.backward(g)

    def whole():
        y = G(R.gen_input(4).to(DEV))
        y.backward(torch.ones_like(y))

    for fn in (chain, whole):
        fn()                                                        # warm-up: weight packing
        G.zero_grad(set_to_none=True)                               # a first gradient is stored, not added
        names = _aten_names(fn)
        print(sorted(names))
        assert not [n for n in names if n.startswith(BANNED)], names
        adds = sum(c for n, c in names.items() if n in ('aten::add', 'aten::add_'))
        # the chain runs none; in the generator the autograd engine sums the two gradients of the head conv's output (it feeds the
        # trunk and the shortcut) -- one add, outside any RRDB
        assert adds == (0 if fn is chain else 1), names


# ---- RRDBNet --------------------------------------------------------------------------------------------------------------------- #

@functools.lru_cache(maxsize=None)
def _generator_reference(scale):
    """fp64 gradients of the fixed functional, and the count of LeakyReLU inputs within roundoff of 0"""
    ref64 = ref_generator(scale, dtype=torch.float64)
    near = []
    hooks = [m.register_forward_hook(lambda m, i, o: near.append(int((i[0].abs() < 1e-5 * i[0].abs().max()).sum())))
             for m in ref64.modules() if isinstance(m, torch.nn.LeakyReLU)]
    (ref64(R.gen_input(scale).double()) * R.gen_functional(scale).double()).sum().backward()
    for h in hooks:
        h.remove()
    return {k: p.grad for k, p in ref64.named_parameters()}, sum(near)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scale', R.SCALES)
def test_generator_matches_reference_vectors_and_fp64_gradients(mode, scale):
    from sradsgan_amd import ops
    g = golden('gen')
    G = hip_generator(ref_generator(scale), scale)
    refg, near = _generator_reference(scale)
    last = 'model.%d.' % (len(G.model) - 1)
    with ops.conv_math(mode):
        fills = ops.dense_stats.fills
        y = G(R.gen_input(scale).to(DEV))
        assert ops.dense_stats.fills == fills              # every dense block's input was written into its buffer by its producer
        (y * R.gen_functional(scale).to(DEV)).sum().backward()
    assert tuple(y.shape) == (2, 3, 12 * scale, 10 * scale)
    want = g['y_x%d' % scale]
    err = np.abs(R.out_digest(y.detach().cpu()) - want)
    print('x%d %s: output digest error %.2e' % (scale, mode, err[:-2].max() if err.size > 4096 else err.max()))
    if err.size > 4096:                                    # sampled values, then [sum, 2-norm]
        assert err[:-2].max() < 1e-4 and err[-2] < 1e-4 * y.numel() and err[-1] < 1e-3
    else:
        assert err.max() < 1e-4
    errs = {k: rel_err(p.grad, refg[k]) for k, p in G.named_parameters()}
    norm_errs = {k: float((p.grad.cpu().double() - refg[k]).norm() / refg[k].norm().clamp_min(1e-30)) for k, p in G.named_parameters()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print('x%d %s: LeakyReLU inputs within 1e-5 of 0: %d; worst max-norm gradient error %s %.2e, worst 2-norm error %.2e'
          % (scale, mode, near, worst[0], worst[1], max(norm_errs.values())))
    # tests/test_ndsrgan_gpu.py's accounting for the same kernels: a LeakyReLU input within roundoff of 0 can take the other branch on
    # the device; exact fp32 stays at roundoff everywhere, split-bf16 gets the wider bar only where the fp64 run HAS near-ties to flip,
    # and the last conv (no LeakyReLU behind it) is held to roundoff in both modes
    if mode == 'bf16x3' and (worst[1] > 2e-2 or max(norm_errs.values()) > 1e-2):
        assert near > 0
    for k in errs:
        assert errs[k] < (1e-4 if mode == 'fp32' else 2e-1) and norm_errs[k] < (1e-4 if mode == 'fp32' else 3e-2), (k, errs[k], norm_errs[k])
        if k.startswith(last):
            assert errs[k] < 1e-4, (k, errs[k])


@pytest.mark.parametrize('mode', MODES)
def test_full_depth_generator_matches_reference_vector(mode):
    from sradsgan_amd import ops
    G = hip_generator(ref_generator(4, nb=23, tag='23'), 4, nb=23)
    with ops.conv_math(mode), torch.no_grad():
        y = G(O.det_fill('esrgan.deep.x', R.DEEP_SHAPE, 0.5, 0.5).to(DEV))
    err = np.abs(R.out_digest(y.cpu()) - golden('gen')['y_deep']).max()
    print('nb 23 %s: output error %.2e' % (mode, err))
    assert tuple(y.shape) == (1, 3, 32, 32) and err < 1e-4


def test_pixelshuffle_generator_matches_fp64():
    from sradsgan_amd.model import esrgan as E
    ref = R.fill_generator(R.Generator(1, 4, upsample_mode='pixelshuffle'), tag='ps')
    G = E.RRDBNet(3, 3, 64, 1, upscale=4, upsample_mode='pixelshuffle')
    G.load_state_dict(ref.state_dict(), strict=True)
    G.to(DEV)
    x = R.gen_input(4)
    with torch.no_grad():
        assert rel_err(G(x.to(DEV)), ref.double()(x.double())) < 1e-4


# ---- the discriminators ------------------------------------------------------------------------------------------------------------ #

class _DeviceSideLeaky(torch.nn.Module):
    """The fp64 referee's LeakyReLU(.2) with the branch the device took.  The function is continuous and its derivative is not: an
    input within roundoff of 0 can fall on either side in any fp32 evaluation (the reference's own fp32 run of Discriminator_VGG_256
    differs from its fp64 run by 3e-2 in the input gradient for that reason alone), and the one-sided derivative on the device's
    side is the exact answer to compare with.  Only near-ties may be overridden: `worst` records the largest |z| / max |z| where
    the given mask and the sign disagree, and the test holds it to roundoff."""

    def __init__(self, mask):
        super().__init__()
        self.mask, self.worst, self.flips = mask, 0.0, 0

    def forward(self, z):
        zd = z.detach()
        off = self.mask != (zd > 0)
        self.flips = int(off.sum())
        if self.flips:
            self.worst = float(zd[off].abs().max() / zd.abs().max())
        return torch.where(self.mask, z, 0.2 * z)


def _discriminator_reference(size, masks, hidden_mask):
    """fp64 output, input gradient and parameter gradients with the device's LeakyReLU branches; per conv that feeds a BatchNorm the
    per-channel sum of |gradient| at its output (the scale of its bias gradient, which is 0 in exact arithmetic)."""
    D64 = ref_discriminator(size, torch.float64)
    acts = [i for i, m in enumerate(D64.features) if isinstance(m, torch.nn.LeakyReLU)]
    assert len(acts) == len(masks)
    for i, mask in zip(acts, masks):
        D64.features[i] = _DeviceSideLeaky(mask)
    scales = {}
    for i, m in enumerate(D64.features):
        if isinstance(m, torch.nn.Conv2d) and isinstance(D64.features[i + 1], torch.nn.BatchNorm2d):
            m.register_full_backward_hook(lambda mod, gi, go, i=i: scales.__setitem__('features.%d.bias' % i, go[0].abs().sum(dim=(0, 2, 3))))
    x64 = R.d_input(size).double().requires_grad_()
    c = D64.classifier
    head_act = _DeviceSideLeaky(hidden_mask)
    out = torch.nn.functional.linear(head_act(torch.nn.functional.linear(D64.features(x64).flatten(1), c[0].weight, c[0].bias)),
                                     c[2].weight, c[2].bias)
    out.sum().backward()
    leaks = [D64.features[i] for i in acts] + [head_act]
    return out.detach(), x64.grad, {k: p.grad for k, p in D64.named_parameters()}, scales, leaks


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('size', R.D_SIZES)
def test_discriminator_matches_fp64_and_reference_buffers(mode, size):
    from sradsgan_amd import ops
    g = golden('disc')
    D = hip_discriminator(ref_discriminator(size), size)
    masks = []
    hooks = [D.features[conv_at if bn_at is None else bn_at].register_forward_hook(lambda m, i, o: masks.append((o.detach() > 0).cpu().contiguous()))
             for conv_at, bn_at in D._blocks]
    x = dev_nhwc(R.d_input(size)).requires_grad_()
    with ops.conv_math(mode):
        out = D(x)
        hidden_mask = (out.grad_fn.saved_tensors[1] > 0).cpu()      # (before the backward frees the node's saved tensors)
        out.sum().backward()
    for h in hooks:
        h.remove()
    out64, dx64, refg, scales, leaks = _discriminator_reference(size, masks, hidden_mask)
    tol = 1e-5 if mode == 'fp32' else 5e-5
    bn_biases = set(scales)                                # exact gradient 0 (the BatchNorm removes the mean): no relative error
    errs = {k: rel_err(p.grad, refg[k]) for k, p in D.named_parameters() if k not in bn_biases}
    bias_errs = {k: float(((dict(D.named_parameters())[k].grad.cpu().double() - refg[k]).abs() / scales[k]).max()) for k in bn_biases}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print('D_%d %s: output %.2e (vs reference fp32 %.2e), dx %.2e, worst parameter gradient %s %.2e, worst bias-before-BN gradient / sum '
          '|dz| %.2e; LeakyReLU branches taken from the device at %d near-ties (largest |z| / max |z| %.1e)'
          % (size, mode, rel_err(out, out64), float(np.abs(out.detach().cpu().numpy() - g['out_%d' % size]).max()), rel_err(x.grad, dx64),
             worst[0], worst[1], max(bias_errs.values()), sum(m.flips for m in leaks), max(m.worst for m in leaks)))
    assert tuple(out.shape) == (2, 1)
    assert max(m.worst for m in leaks) < 1e-4              # the device's branch replaced the sign only within roundoff of the kink
    for k, b in R.bn_buffers(D):
        want = g['buf_%d__%s' % (size, k.replace('.', '__'))]
        assert np.abs(b.cpu().numpy() - want).max() < 1e-4 * max(1.0, np.abs(want).max()), k
    assert rel_err(out, out64) < tol and rel_err(x.grad, dx64) < tol
    for k in errs:
        assert errs[k] < tol, (k, errs[k])
    for k in bias_errs:                                    # a sum of n h w terms that cancel: held against the sum of their magnitudes
        assert bias_errs[k] < tol, (k, bias_errs[k])


def test_discriminator_refuses_another_input_size_on_the_device():
    from sradsgan_amd.model import esrgan as E
    D = E.Discriminator_VGG_96(3, 64).to(DEV)
    with pytest.raises(ValueError, match=r'\(96, 128, 192, 256\)'):
        D(torch.zeros(2, 3, 128, 128, device=DEV))


# ---- the perceptual extractor ------------------------------------------------------------------------------------------------------ #

def _extractor_inputs(size):
    return O.det_fill('vggfx.x.%d' % size, (2, 3, size, size), 0.5, 0.5), O.det_fill('vggfx.r.%d' % size, (2, 512, size // 16, size // 16), 1.0)


def _extractor_reference(size, acts):
    """fp64 features and input gradient with the device's branches (see _DeviceSideLeaky): a ReLU passes where the device's output is
    positive, a max pool routes through the element the device's values select -- both continuous in the value, so only the
    one-sided derivative changes, and only within roundoff of a tie (`worst`: the largest value, relative to the layer's largest,
    that a branch taken from the device moved).  acts: the device's 16 conv outputs (ReLU applied but for the last), on the CPU."""
    F64 = ref_extractor(torch.float64)
    x, r = _extractor_inputs(size)
    x64 = x.double().requires_grad_()
    h = (x64 - F64.mean) / F64.std
    ci, worst = 0, 0.0
    for m in F64.features:
        if isinstance(m, torch.nn.Conv2d):
            h = m(h)
            ci += 1
        elif isinstance(m, torch.nn.ReLU):
            mask = acts[ci - 1] > 0
            off = mask != (h.detach() > 0)
            if bool(off.any()):
                worst = max(worst, float(h.detach()[off].abs().max() / h.detach().abs().max()))
            h = torch.where(mask, h, torch.zeros_like(h))
        else:
            _, idx = torch.nn.functional.max_pool2d(acts[ci - 1].double(), 2, return_indices=True)
            picked = h.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            worst = max(worst, float((torch.nn.functional.max_pool2d(h.detach(), 2) - picked.detach()).abs().max() / h.detach().abs().max()))
            h = picked
    (h * r.double()).sum().backward()
    return h.detach(), x64.grad, worst


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('size', [96, 128])
def test_extractor_matches_fp64(mode, size):
    """conv5_4 sits behind 16 convs, the depth of an RRDB (15): the block's bars for the output, 1e-5 (fp32) / 1e-4 (split-bf16); the
    input gradient passes 16 data gradients, 15 ReLU masks and 4 pool routings on the way back and gets the block's parameter-gradient
    bars, 10 x that."""
    from sradsgan_amd import ops
    x, r = _extractor_inputs(size)
    Fx = hip_extractor(ref_extractor())
    acts = []
    hooks = [m.register_forward_hook(lambda m, i, o: acts.append(o.detach().cpu().contiguous())) for m in Fx.features
             if isinstance(m, torch.nn.Conv2d)]
    with ops.conv_math(mode):
        xl = dev_nhwc(x).requires_grad_()
        f = Fx(xl)
        (f * r.to(DEV)).sum().backward()
    for h in hooks:
        h.remove()
    assert len(acts) == 16
    f64, dx64, worst = _extractor_reference(size, acts)
    tol = 1e-5 if mode == 'fp32' else 1e-4
    print('extractor %d %s: output %.2e, input gradient %.2e; branches taken from the device moved at most %.1e of a layer\'s largest value'
          % (size, mode, rel_err(f, f64), rel_err(xl.grad, dx64), worst))
    assert tuple(f.shape) == (2, 512, size // 16, size // 16)
    assert worst < 1e-4                                    # the device's branch replaced the fp64 one only within roundoff of a tie
    assert rel_err(f, f64) < tol and rel_err(xl.grad, dx64) < 10 * tol
    assert all(p.grad is None for p in Fx.parameters())


# ---- the step ---------------------------------------------------------------------------------------------------------------------- #

def _params_err(net, ref):
    refp = dict(ref.named_parameters())
    return np.concatenate([(p.detach().cpu().double() - refp[k].detach()).abs().flatten().numpy() for k, p in net.named_parameters()])


@pytest.mark.parametrize('gan_type,relative', R.STEP_CASES)
def test_two_training_iterations_match_fixtures_restatement_and_adam(gan_type, relative):
    from sradsgan_amd import ops
    from sradsgan_amd.model import esrgan as E
    g, tag = golden('step'), case_tag(gan_type, relative)
    x, t = R.step_inputs()
    refs = ref_generator(R.STEP_SCALE, dtype=torch.float64), ref_discriminator(R.STEP_D, torch.float64), ref_extractor(torch.float64)
    ref_opt_G = torch.optim.Adam(refs[0].parameters(), lr=R.ADAM_LR, betas=(0.9, 0.999))
    ref_opt_D = torch.optim.Adam(refs[1].parameters(), lr=R.ADAM_LR, betas=(0.9, 0.999))
    steps = {}
    for mode in MODES:
        nets = (hip_generator(ref_generator(R.STEP_SCALE), R.STEP_SCALE), hip_discriminator(ref_discriminator(R.STEP_D), R.STEP_D),
                hip_extractor(ref_extractor()))
        steps[mode] = (nets, E.TrainStep(*nets, lr=R.ADAM_LR, gan_type=gan_type, relative=relative, **R.WEIGHTS))
    names = ('loss_G', 'loss_D', 'pixel', 'content', 'loss_gan')
    for it in range(2):
        want = R.train_iteration(*refs, ref_opt_G, ref_opt_D, x.double(), t.double(), gan_type, relative, **R.WEIGHTS)
        for mode in MODES:
            (G, D, _), step = steps[mode]
            with ops.conv_math(mode):
                out = step(x.to(DEV), t.to(DEV))
            assert sorted(out) == sorted(names) and all(v.dim() == 0 and v.is_cuda for v in out.values())
            got = np.array([float(out[k]) for k in names])
            print(tag, mode, it, got, 'vs restatement %.2e, vs fixture %.2e'
                  % (np.abs(got - np.array([want[k] for k in names])).max(), np.abs(got - g[tag][it]).max()))
            for j, k in enumerate(names):
                assert abs(got[j] - want[k]) < 1e-4 and abs(got[j] - g[tag][it][j]) < 1e-4, (mode, it, k, got[j], want[k], g[tag][it][j])
            for net, ref in ((G, refs[0]), (D, refs[1])):
                d = _params_err(net, ref)
                # Adam turns a gradient whose sign is roundoff into a full +-lr step; the bulk must agree closely
                assert d.max() <= 2 * R.ADAM_LR * (it + 1) + 1e-6 and np.median(d) < 1e-6, (mode, it, d.max(), np.median(d))
            refb = dict(R.bn_buffers(refs[1]))
            for k, b in R.bn_buffers(D):
                assert rel_err(b, refb[k]) < (1e-4 if it == 0 else 1e-2), (mode, it, k)
            assert step.arena_G.check_views() and step.arena_D.check_views()


def test_step_clamps_the_discriminator_only_when_asked():
    from sradsgan_amd.model import esrgan as E
    x, t = R.step_inputs()
    nets = (hip_generator(ref_generator(R.STEP_SCALE), R.STEP_SCALE), hip_discriminator(ref_discriminator(R.STEP_D), R.STEP_D),
            hip_extractor(ref_extractor()))
    step = E.TrainStep(*nets, lr=R.ADAM_LR, clip_value=0.01)
    assert (step.lr_G, step.lr_D) == (R.ADAM_LR, R.ADAM_LR)
    before = max(float(p.abs().max()) for p in nets[1].parameters())
    step(x.to(DEV), t.to(DEV))
    assert before > 0.01 and max(float(p.abs().max()) for p in nets[1].parameters()) <= 0.01
    assert max(float(p.abs().max()) for p in nets[0].parameters()) > 0.01          # the generator is never clamped


def test_default_config_batch16_step_is_finite_and_deterministic():
    from sradsgan_amd.model import esrgan as E
    refs = ref_generator(4, nb=23, tag='23'), ref_discriminator(128), ref_extractor()
    x = O.det_fill('esrgan.b16.x', (16, 3, 32, 32), 0.5, 0.5).to(DEV)
    t = O.det_fill('esrgan.b16.t', (16, 3, 128, 128), 0.5, 0.5).to(DEV)
    runs = []
    for _ in range(2):
        G, D, Fx = hip_generator(refs[0], 4, nb=23), hip_discriminator(refs[1], 128), hip_extractor(refs[2])
        out = E.TrainStep(G, D, Fx, lr=1e-4, weight_pixel=1e-2, weight_content=1.0, weight_gan=5e-3)(x, t)
        runs.append(([out[k].cpu() for k in sorted(out)], G.model[0].weight.detach().cpu(), D.classifier[0].weight.detach().cpu()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.isfinite(a) and torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ---- existing entry points, end to end --------------------------------------------------------------------------------------------- #

def test_scene_and_self_ensemble_take_the_new_generator():
    from sradsgan_amd import ensemble, scene
    G = hip_generator(ref_generator(4), 4).eval()
    u8 = (O.det_fill('esrgan.scene', (40, 36, 3), 0.5, 0.5) * 255).to(torch.uint8)
    out = scene.super_resolve_scene(G, u8, 4, 16, 4)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (160, 144, 3)
    with torch.no_grad():                                            # composed by hand: the plan, the tiles, the blender
        plan = scene.ScenePlan(40, 36, 4, 16, 4)
        by_hand = scene.run_plan(plan, u8.to(DEV).contiguous(), G, 16).out
    assert torch.equal(out, by_hand)
    lr = R.gen_input(4).to(DEV)
    got = ensemble.self_ensemble(G, lr)
    with torch.no_grad():                                            # by hand: the views in the ensemble's two batches, then the merge
        outs = [None] * 8
        for transposing in (0, 1):
            idx = [op for op in range(8) if op & 1 == transposing]
            sr = G(torch.cat([lr if op == 0 else ensemble.dihedral(lr, op) for op in idx], dim=0))
            for q, op in enumerate(idx):
                outs[op] = sr[q * 2:(q + 1) * 2]
        want = ensemble.merge(outs, list(range(8)))
    assert tuple(got.shape) == (2, 3, 48, 40) and torch.equal(got, want)


def test_esrgan_trainer_end_to_end(tmp_path):
    import os
    from sradsgan_amd.model import esrgan as E
    g = torch.Generator().manual_seed(34)
    train = [torch.randint(0, 256, (2, 96, 96, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    hr = torch.rand(2, 3, 96, 96, generator=g)
    test = [(torch.nn.functional.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]
    args = E.default_args(num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=96, hr_height=96, hr_width=96,
                          sample_interval=1, nb=1)
    net = E.ESRGAN(args, train_loader=train, test_loader=test)
    hist = net.train()
    assert isinstance(net.generator, E.RRDBNet) and net.generator.nb == 1 and type(net.discriminator) is E.Discriminator_VGG_96
    assert isinstance(net.feature_extractor, E.VGGFeatureExtractor) and isinstance(net.step, E.TrainStep)
    assert (net.step.gan_type, net.step.relative, net.step.clip_value, net.step.weight_pixel) == ('vanilla', True, None, 1e-2)
    assert len(hist) == 1 and all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
    files = sorted(os.listdir(os.path.join(str(tmp_path), 'model')))
    assert files == ['discriminator_param.pkl', 'discriminator_param_epoch_1.pkl', 'generator_param.pkl', 'generator_param_epoch_1.pkl']
    psnr, ssim, ergas, lpips = net.mfeNew_validate(epoch=1, modelpath=os.path.join(str(tmp_path), 'model', 'generator_param_epoch_1.pkl'))
    assert abs(psnr - hist[-1]['psnr']) < 1e-9 and lpips != lpips
    assert 'esrgan_psnr:' in open(os.path.join(str(tmp_path), 'val_log.txt')).read().splitlines()[-1]
    # resume: epoch != 0 loads the epoch files strictly, the generator through RRDBNet.load_state_dict
    net2 = E.ESRGAN(E.default_args(**dict(vars(args), epoch=1, num_epochs=1)), train_loader=train, test_loader=test)
    net2._build()
    for (k, a), (_, b) in zip(net.generator.state_dict().items(), net2.generator.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k
