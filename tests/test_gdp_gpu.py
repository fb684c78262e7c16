"""The GDP diffusion sampler on the device (sradsgan_amd/model/gdp.py, csrc/diffusion.hip) against float64 on the same inputs: the
new kernels one by one, the conv routes at the U-Net's widths, the small U-Net and the six-step sampling loop against vectors recorded
from the reference (tools/make_golden_gdp.py) and against the restatement (tests/gdp_ref.py), and gdp_super_resolve end to end.

Measured on the MI355X (each test prints its own figures with -s): see DESIGN 9."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O
from tests import conv_emulation as E
from tests import gdp_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODES = ('fp32', 'bf16x3')
NET_BAR = {'fp32': 1e-4, 'bf16x3': 1e-3}


def rel_err(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def attention_bar(e32):
    """The bar of the attention output: 4 x the error of the fp32 restatement, never below 1e-5."""
    return max(1e-5, 4 * e32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- GroupNorm / SiLU ------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize('n,p,c', [(3, 35, 32), (2, 9, 96), (2, 4, 2048), (1, 729, 1024)])
def test_group_norm_scale_shift_silu_matches_fp64(n, p, c):
    from sradsgan_amd.model import gdp
    tag = 'gdp.gn.%d.%d.%d' % (n, p, c)
    x = O.det_fill(tag + '.x', (n, p, c), 2.0, 1.5)
    g, b = O.det_fill(tag + '.g', (c,), 0.5, 1.0), O.det_fill(tag + '.b', (c,), 0.5)
    sc, sh = O.det_fill(tag + '.sc', (n, c), 0.5), O.det_fill(tag + '.sh', (n, c), 0.5)
    wide = torch.zeros(n, p, c + 8)
    wide[..., 4:c + 4] = x
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    mod = torch.cat([sc, sh], dim=1).to(DEV)                                # the emb_layers row: scale | shift
    wd = wide.to(DEV)
    odd = torch.zeros(n, p, c + 6)
    odd[..., 3:c + 3] = x                                                   # rows that start off a 16-byte boundary: the scalar loads
    od = odd.to(DEV)
    base64 = F.group_norm(x.double().permute(0, 2, 1), 32, g.double(), b.double(), 1e-5).permute(0, 2, 1)
    worst = 0.0
    for with_mod in (False, True):
        for act in (False, True):
            want = base64 * (1 + sc.double()[:, None]) + sh.double()[:, None] if with_mod else base64
            want = F.silu(want) if act else want
            args = (mod[:, :c], mod[:, c:]) if with_mod else (None, None)
            y = gdp.group_norm_act(xd, gd, bd, *args, silu=act)
            e = rel_err(y, want)
            worst = max(worst, e)
            assert e < 2e-6, (with_mod, act, e)
            assert torch.equal(bits(y), bits(gdp.group_norm_act(xd, gd, bd, *args, silu=act)))               # re-run
            assert torch.equal(bits(y), bits(gdp.group_norm_act(wd[..., 4:c + 4], gd, bd, *args, silu=act)))  # ldx > C
            assert torch.equal(bits(y), bits(gdp.group_norm_act(od[..., 3:c + 3], gd, bd, *args, silu=act)))
            y1 = gdp.group_norm_act(xd[:1], gd, bd, *((a[:1] for a in args) if with_mod else args), silu=act)
            assert torch.equal(bits(y1[0]), bits(y[0]))                       # sample 0 alone and in the batch
    print('gdp group norm %s: worst rel err %.2e (bar 2e-6)' % ((n, p, c), worst))


def test_group_norm_refuses_bad_widths():
    from sradsgan_amd import _hip
    from sradsgan_amd.model import gdp
    for c in (48, 2080):
        with pytest.raises(_hip.HipLibraryError):
            gdp.group_norm_act(torch.zeros(1, 4, c, device=DEV), torch.ones(c, device=DEV), torch.zeros(c, device=DEV))


# ---- average pool ---------------------------------------------------------------------------------------------------------------- #
def test_avg_pool_matches_aten_and_refuses_odd_sizes():
    from sradsgan_amd import _hip
    from sradsgan_amd.model import gdp
    x = O.det_fill('gdp.pool.x', (2, 36, 10, 14), 3.0)
    y = gdp.avg_pool2x2(x.to(DEV).contiguous(memory_format=torch.channels_last)).cpu()
    a, b, c, d = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
    assert torch.equal(y, (((a + b) + c) + d) * 0.25)                          # the kernel's fixed four-term order, exactly
    ref = F.avg_pool2d(x, 2)
    ulp = (y.contiguous().view(torch.int32).long() - ref.contiguous().view(torch.int32).long()).abs().max()
    print('gdp avg pool: %d ulp from F.avg_pool2d' % int(ulp))
    assert int(ulp) <= 1
    for shape in ((1, 32, 5, 4), (1, 32, 4, 7)):
        with pytest.raises(_hip.HipLibraryError, match='even'):
            gdp.avg_pool2x2(torch.zeros(shape, device=DEV))


# ---- attention ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('n,heads,ch,t', [(2, 4, 32, 36), (1, 2, 64, 65), (2, 16, 64, 729), (1, 1, 64, 1)])
def test_attention_matches_fp64(n, heads, ch, t):
    from sradsgan_amd.model import gdp
    qkv = O.det_fill('gdp.attn.%d.%d.%d.%d' % (n, heads, ch, t), (n, t, heads * 3 * ch), 6.0)
    as_ref = qkv.permute(0, 2, 1)                                             # the reference's [n, width, T]
    want = R.attention(as_ref.double(), heads).permute(0, 2, 1)
    e32 = rel_err(R.attention(as_ref.contiguous(), heads).permute(0, 2, 1), want)
    q, k, _ = as_ref.double().reshape(n * heads, 3 * ch, t).split(ch, dim=1)
    top = float(torch.einsum('bct,bcs->bts', q, k).max() / math.sqrt(ch))
    got = gdp.qkv_attention(qkv.to(DEV), heads)
    e = rel_err(got, want)
    bar = attention_bar(e32)
    print('gdp attention %s: rel err %.2e, fp32 restatement %.2e, bar %.2e, largest logit %.1f' % ((n, heads, ch, t), e, e32, bar, top))
    if t >= 36:
        assert top > 30                                                       # the running-maximum rescale is exercised
    assert tuple(got.shape) == (n, t, heads * ch) and e <= bar
    assert torch.equal(bits(got), bits(gdp.qkv_attention(qkv.to(DEV), heads)))


def test_attention_refuses_other_head_widths():
    from sradsgan_amd import _hip
    from sradsgan_amd.model import gdp
    with pytest.raises(_hip.HipLibraryError, match='32 or 64'):
        gdp.qkv_attention(torch.zeros(1, 4, 3 * 48, device=DEV), 1)


# ---- sampler update -------------------------------------------------------------------------------------------------------------- #
def test_sampler_update_matches_fp64_and_keeps_the_condition():
    from sradsgan_amd.model import gdp
    c1, c2, lv = R.posterior(R.betas64('linear', 1000))
    shape = (2, 7, 9, 3)
    x0 = O.det_fill('gdp.step.x0', shape, 1.6)                                # beyond [-1, 1]: the clamp is live
    xt, z = O.det_fill('gdp.step.xt', shape, 2.0), O.det_fill('gdp.step.z', shape, 2.5)
    cond = O.det_fill('gdp.step.cond', shape, 1.0)
    for i in (0, 1, 999):
        buf = torch.cat([xt, cond], dim=-1).to(DEV)
        gdp.sampler_step(x0.to(DEV), buf[..., :3], buf[..., :3], c1[i], c2[i], lv[i], i > 0, noise=z.to(DEV))
        want = float(c1[i]) * x0.double().clamp(-1, 1) + float(c2[i]) * xt.double()
        if i > 0:
            want = want + math.exp(0.5 * float(lv[i])) * z.double()
        e = rel_err(buf[..., :3], want)
        print('gdp sampler step t=%d: rel err %.2e (bar 2e-6)' % (i, e))
        assert e < 2e-6
        assert torch.equal(bits(buf[..., 3:]), bits(cond))                    # channels 3..5 untouched, bit for bit
    # t = 0 adds no noise, whatever is passed
    out = torch.empty(shape, device=DEV)
    gdp.sampler_step(x0.to(DEV), xt.to(DEV), out, c1[0], c2[0], lv[0], False, noise=None, seed=3, step=1)
    assert rel_err(out, float(c1[0]) * x0.double().clamp(-1, 1) + float(c2[0]) * xt.double()) < 2e-6


def test_philox_draws_are_reproducible_and_normal():
    from sradsgan_amd.model import gdp
    a = gdp.randn_rows(torch.empty(1 << 18, 4, device=DEV), 11, 5)
    b = gdp.randn_rows(torch.empty(1 << 18, 4, device=DEV), 11, 5)
    c = gdp.randn_rows(torch.empty(1 << 18, 4, device=DEV), 11, 6)
    assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c))
    wide = torch.zeros(1 << 18, 6, device=DEV)
    gdp.randn_rows(wide[:, :4], 11, 5)
    assert torch.equal(bits(wide[:, :4]), bits(a)) and float(wide[:, 4:].abs().max()) == 0       # strided: same bits, nothing else written
    mean, var = float(a.double().mean()), float(a.double().var(unbiased=False))
    print('gdp philox: 2^20 draws, mean %.2e, var - 1 %.2e' % (mean, var - 1))
    assert abs(mean) < 4.9e-3 and abs(var - 1) < 6.9e-3
    ref = R.philox_normal(11, 5, 4096)
    assert np.abs(a.cpu().numpy().ravel()[:4096] - ref).max() < 1e-5          # the restated generator: same stream
    # the sampler draws the same values in the kernel: x0 = xt = 0 leaves sigma * z
    zero = torch.zeros(64, 3, device=DEV)
    out = gdp.sampler_step(zero, zero, torch.empty(64, 3, device=DEV), 0.0, 0.0, 0.0, True, noise=None, seed=11, step=5)
    assert torch.equal(bits(out), bits(gdp.randn_rows(torch.empty(64, 3, device=DEV), 11, 5)))


# ---- quantisation ---------------------------------------------------------------------------------------------------------------- #
def test_quantisation_rounds_half_to_even_like_numpy():
    from sradsgan_amd.model import gdp
    ramp = np.concatenate([np.linspace(-1.5, 1.5, 30001, dtype=np.float32), np.array([0.0, -1.0, 1.0, 3.0, -7.0], np.float32)])
    ramp = ramp[:ramp.size // 3 * 3].reshape(-1, 3)
    got = gdp.quantize_u8(torch.from_numpy(ramp).to(DEV)).cpu().numpy()
    assert np.array_equal(got, R.quantize(ramp)) and got.min() == 0 and got.max() == 255
    halves = (np.arange(255, dtype=np.float32) + np.float32(0.5)).reshape(-1, 3)            # min_max (0, 255): j + 1/2 comes back exactly
    pre = (np.clip(halves, 0, 255) - np.float32(0)) / np.float32(255) * np.float32(255.0)
    ties = pre - np.floor(pre) == 0.5
    assert ties.sum() > 50
    got = gdp.quantize_u8(torch.from_numpy(halves).to(DEV), (0.0, 255.0)).cpu().numpy()
    assert np.array_equal(got, pre.round().astype(np.uint8))
    assert np.array_equal(got[ties] % 2, np.zeros(int(ties.sum()), np.uint8))                # ties went to the even byte


# ---- the existing conv route at the U-Net's widths ------------------------------------------------------------------------------- #
# case -> (shape, arithmetic expected in bf16x3 mode); fp32 mode always runs fp32.  Route choice (conv_fast_fprop.hip,
# choose_fprop_route): the split-bf16 kernels are taken from 128 output tiles on; the three shapes of 9 or 288 pixels stay far below
# that and take the register-staged kernel, whose products are fp32 in every mode, as does the 6-channel conv (Cin % 16 != 0, the
# generic kernel).  The qkv conv at the real token count (2 x 27 x 27 pixels, 288 tiles) is added so that the split-bf16 kernel is seen
# at a U-Net width too.
CONV_CASES = {'3x3-2048-1024': ((1, 2048, 3, 3, 1024, 3), 'fp32'), '1x1-1024-3072': ((1, 1024, 3, 3, 3072, 1), 'fp32'),
              '3x3-6-128': ((2, 6, 12, 12, 128, 3), 'fp32'), '1x1-1024-3072-at-729-tokens': ((2, 1024, 27, 27, 3072, 1), 'bf16x3')}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', sorted(CONV_CASES))
def test_conv_route_at_unet_widths(mode, case):
    """tests/test_conv_routes_gpu.py's bound and TAU against the emulation of the ONE arithmetic the route is expected to run, and,
    as there, the result must be at least twice as close in the 2-norm to that emulation as to the neighbouring one."""
    from sradsgan_amd import ops
    (n, cin, h, w, cout, k), expect = CONV_CASES[case]
    expect = 'fp32' if mode == 'fp32' else expect
    other = 'bf16x3' if expect == 'fp32' else 'fp32'
    tag = 'gdp.conv.%d.%d.%d' % (cin, cout, k)
    x = O.det_fill(tag + '.x', (n, cin, h, w), 1.0)
    wt = O.det_fill(tag + '.w', (cout, cin, k, k), math.sqrt(3.0 / (cin * k * k)))
    bias = O.det_fill(tag + '.b', (cout,), 0.05)
    with ops.conv_math(mode):
        got = ops.conv2d_fwd_raw(x.to(DEV).contiguous(memory_format=torch.channels_last), wt.to(DEV), bias.to(DEV), 1, k // 2).cpu()
    tau = {'fp32': 32 * E.U24, 'bf16x3': 20 * E.U24}
    ref, absref = E.epilogue(*E.conv_fwd(x, wt, 1, k // 2, expect), bias=bias)
    ref_o, _ = E.epilogue(*E.conv_fwd(x, wt, 1, k // 2, other), bias=bias)
    ratio = E.worst(got, ref, absref, tau[expect])[0]
    own, far = E.l2_dist(got, ref), E.l2_dist(got, ref_o)
    print('gdp conv %s in %s mode: %s err / bound %.3f; 2-norm distance to %s %.3e, to %s %.3e'
          % (case, mode, expect, ratio, expect, own, other, far))
    assert ratio <= 1.0
    assert 2 * own <= far


# ---- the U-Net and the loop ------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope='module')
def small():
    from sradsgan_amd.model import gdp
    net = R.init_(gdp.UNet(**R.SMALL))
    return net.to(DEV), R.state(net, torch.float64)


@pytest.mark.parametrize('mode', MODES)
def test_small_unet_matches_reference_vectors_and_fp64(small, mode):
    from sradsgan_amd import ops
    net, sd64 = small
    g = np.load(os.path.join(GOLD, 'gdp_small.npz'))
    x = R.small_input()
    for name, ts in R.SMALL_T.items():
        t = torch.tensor(ts)
        with ops.conv_math(mode):
            y = net(x.to(DEV), t)
        assert tuple(y.shape) == tuple(g['shape'])
        e_gold = rel_err(O.digest(y), g[name])
        e64 = rel_err(y, R.unet_forward(sd64, x.double(), t, R.SMALL))
        print('gdp small net %s %s: vs reference %.2e, vs fp64 %.2e (bar %.0e)' % (name, mode, e_gold, e64, NET_BAR[mode]))
        assert e64 <= NET_BAR[mode] and e_gold <= NET_BAR[mode]


@pytest.mark.parametrize('mode', MODES)
def test_six_step_loop_matches_the_reference(small, mode):
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp
    net, _ = small
    g = np.load(os.path.join(GOLD, 'gdp_loop.npz'))
    G = gdp.GaussianDiffusion(net, image_size=12, channels=3, conditional=True)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, DEV)
    cond = R.small_input()[:, 3:].contiguous().to(DEV)
    noise = torch.from_numpy(g['noise']).to(DEV)
    with ops.conv_math(mode):
        stack = G.super_resolution(cond, continous=True, noise=noise)
        final = G.super_resolution(cond, continous=False, noise=noise)
    assert tuple(stack.shape) == tuple(g['stack'].shape) and tuple(final.shape) == tuple(g['final'].shape)
    assert torch.equal(stack[:2].cpu(), cond.cpu()) and torch.equal(bits(stack[-1]), bits(final))     # the condition first, the last image last
    e_final, e_stack = rel_err(final, g['final']), rel_err(stack, g['stack'])
    print('gdp six-step loop %s: final image %.2e, whole stack %.2e (bar %.0e)' % (mode, e_final, e_stack, NET_BAR[mode]))
    assert e_final <= NET_BAR[mode]
    for k in range(7):                                                        # order: entry k of the stack is iterate k
        assert rel_err(stack[2 * k:2 * k + 2], g['stack'][2 * k:2 * k + 2]) <= 10 * NET_BAR[mode]


def test_p_sample_is_one_step_of_the_loop(small):
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp
    net, _ = small
    g = np.load(os.path.join(GOLD, 'gdp_loop.npz'))
    G = gdp.GaussianDiffusion(net, image_size=12, channels=3, conditional=True)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, DEV)
    cond = R.small_input()[:, 3:].contiguous().to(DEV)
    noise = torch.from_numpy(g['noise']).to(DEV)
    with ops.conv_math('fp32'):
        x5 = G.p_sample(noise[0], torch.full((2,), 5, dtype=torch.long), condition_x=cond, noise=noise[1])
    assert tuple(x5.shape) == (2, 3, 12, 12) and rel_err(x5, g['stack'][2:4]) <= NET_BAR['fp32']      # t = 5: the first iterate
    with pytest.raises(NotImplementedError, match='one timestep'):
        G.p_sample(noise[0], torch.tensor([5, 4]), condition_x=cond, noise=noise[1])
    with pytest.raises(NotImplementedError, match='clip_denoised'):
        G.p_sample(noise[0], torch.tensor([5, 5]), clip_denoised=False, condition_x=cond)


def test_unconditional_sample_runs_on_a_three_channel_net():
    from sradsgan_amd.model import gdp
    net = R.init_(gdp.UNet(**dict(R.SMALL, in_channel=3)), 'gdp.uncond.').to(DEV)
    G = gdp.GaussianDiffusion(net, image_size=12, channels=3, conditional=False)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, DEV)
    a, b = G.sample(2, seed=9), G.sample(2, seed=9)
    assert tuple(a.shape) == (2, 3, 12, 12) and bool(torch.isfinite(a).all()) and torch.equal(bits(a), bits(b))
    sd = {'denoise_fn.' + k: v for k, v in R.state(net, torch.float64).items()}
    # one reverse step by hand: the restated U-Net on the restated draws
    z = R.philox_noise(9, 6, 2, 3, 12, 12)
    c1, c2, lv = R.posterior(R.betas64('linear', 6))
    x0 = R.unet_forward(sd, z[0], torch.full((2,), 5), dict(R.SMALL, in_channel=3), 'denoise_fn.').clamp(-1, 1)
    want = float(c1[5]) * x0 + float(c2[5]) * z[0] + math.exp(0.5 * float(lv[5])) * z[1]
    got = G.p_sample(z[0].float().to(DEV), torch.tensor([5, 5]), seed=9, step=1)
    print('gdp unconditional step: rel err %.2e (bar %.0e)' % (rel_err(got, want), NET_BAR['bf16x3']))
    assert rel_err(got, want) <= NET_BAR['bf16x3']


def test_seeded_sampling_is_reproducible(small):
    from sradsgan_amd.model import gdp
    net, _ = small
    G = gdp.GaussianDiffusion(net, image_size=12, channels=3, conditional=True)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, DEV)
    cond = R.small_input()[:, 3:].contiguous().to(DEV)
    a, b, c = (G.super_resolution_batch(cond, seed=s) for s in (5, 5, 6))
    assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c)) and tuple(a.shape) == (2, 3, 12, 12)
    torch.manual_seed(0)
    d = G.super_resolution_batch(cond)
    torch.manual_seed(0)
    assert torch.equal(bits(d), bits(G.super_resolution_batch(cond)))         # no seed: one is drawn from torch's default generator


def test_super_resolve_bytes_match_the_composition(small):
    """gdp_super_resolve against resize_u8 -> the fp64 restatement on the device's own draws (read back) -> numpy's quantisation.
    Bytes whose value before rounding lies within 1e-3 of a half-integer may be left out, at most 1 % of them."""
    from sradsgan_amd import data as sdata, ops
    from sradsgan_amd.model import gdp
    net, sd64 = small
    G = gdp.GaussianDiffusion(net, image_size=12, channels=3, conditional=True)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, DEV)
    lr = R.sr_input()
    draws = torch.stack([gdp.randn_rows(torch.empty(2, 12, 12, 3, device=DEV), R.SR_SEED, k).permute(0, 3, 1, 2) for k in range(7)]).cpu()
    assert float((draws.double() - R.philox_noise(R.SR_SEED, 6, 2, 3, 12, 12)).abs().max()) < 1e-5
    up = sdata.resize_u8(torch.from_numpy(lr).to(DEV), 12, 12).cpu().numpy()
    from oracle import pil_resample_ref as P
    assert np.array_equal(up, np.stack([P.resize_u8(im, 12, 12, 'bicubic') for im in lr]))
    sdg = {'denoise_fn.' + k: v for k, v in sd64.items()}
    o = R.LOOP_SCHEDULE
    v = R.super_resolve_values(sdg, lr, 12, draws.double(), R.betas64(o['schedule'], o['n_timestep'], o['linear_start'], o['linear_end']),
                               R.SMALL)
    near = np.abs(v - np.floor(v) - 0.5) < 1e-3
    want = np.rint(v).astype(np.uint8)
    with ops.conv_math('fp32'):
        got = gdp.gdp_super_resolve(G, torch.from_numpy(lr).to(DEV), 12, seed=R.SR_SEED).cpu().numpy()
    assert got.shape == (2, 12, 12, 3) and got.dtype == np.uint8
    differ = got != want
    print('gdp super-resolve: %d of %d bytes differ, %d of them outside the tie window; %.2f %% of values in the window'
          % (differ.sum(), differ.size, (differ & ~near).sum(), 100 * near.mean()))
    assert near.mean() < 0.01
    assert not (differ & ~near).any()
