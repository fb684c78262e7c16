"""The GDP diffusion training path on the device (sradsgan_amd/model/gdp_train.py, the backward kernels of csrc/diffusion.hip) against
float64 autograd of the plain formulas on the CPU (tests/gdp_train_ref.py): the kernels one by one, then the small net's forward bits,
loss and gradients (also against vectors recorded from the reference, tools/make_golden_gdp_train.py), three Adam steps, sampling
after training, the checkpoint round trip, the unconditional net and training_batch.

Errors are relative to the largest reference value (rel_err of tests/test_gdp_gpu.py).  A bar max(floor, 4 e32) takes e32 as the float32
CPU run of the same formula against its float64 run, computed here.  Every test prints its figures (-s); DESIGN 9 lists them."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import gdp_ref as R
from tests import gdp_train_ref as T
from tests.test_gdp_gpu import NET_BAR, bits, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODES = ('fp32', 'bf16x3')
GRAD_FACTOR = {'fp32': 10.0, 'bf16x3': 100.0}      # x the float32 CPU restatement's own gradient score
LOSS_BAR = 1e-5


def lse_bar(e32):
    """The bar of the saved log-sum-exp: 4 x the error of the fp32 restatement, never below 2e-6."""
    return max(2e-6, 4 * e32)


def leaf(t):
    return t.detach().to(DEV).requires_grad_(True)


# ---- GroupNorm backward ---------------------------------------------------------------------------------------------------------- #
def _gn_device(x, g, b, sc, sh, act, dy):
    """(dx, dgamma, dbeta, dscale, dshift) on the device; x may be a strided device view (then it is used as the leaf)."""
    from sradsgan_amd.model import gdp_train
    xs = x.detach().requires_grad_(True) if x.is_cuda else leaf(x)
    leaves = [xs, leaf(g), leaf(b), None if sc is None else leaf(sc), None if sh is None else leaf(sh)]
    y = gdp_train.group_norm_act(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], silu=act)
    y.backward(dy.to(DEV))
    return [None if v is None else v.grad for v in leaves]


@pytest.mark.parametrize('n,p,c', [(3, 35, 32), (2, 9, 96), (2, 4, 2048), (1, 729, 1024)])
def test_group_norm_backward_matches_fp64(n, p, c):
    tag = 'gdp.gnb.%d.%d.%d' % (n, p, c)
    x = O.det_fill(tag + '.x', (n, p, c), 2.0, 1.5)
    g, b = O.det_fill(tag + '.g', (c,), 0.5, 1.0), O.det_fill(tag + '.b', (c,), 0.5)
    sc, sh = O.det_fill(tag + '.sc', (n, c), 0.5), O.det_fill(tag + '.sh', (n, c), 0.5)
    dy = O.det_fill(tag + '.dy', (n, p, c), 1.0)
    wide, odd = torch.zeros(n, p, c + 8), torch.zeros(n, p, c + 6)
    wide[..., 4:c + 4] = x
    odd[..., 3:c + 3] = x                                                    # rows off a 16-byte boundary: the scalar loads
    wd, od = wide.to(DEV), odd.to(DEV)
    names = ('dx', 'dgamma', 'dbeta', 'dscale', 'dshift')
    for with_mod in (False, True):
        for act in (False, True):
            m = (sc, sh) if with_mod else (None, None)
            want = T.gn_act_grads(x, g, b, *m, act, dy, torch.float64)
            w32 = T.gn_act_grads(x, g, b, *m, act, dy, torch.float32)
            got = _gn_device(x, g, b, *m, act, dy)
            for name, a, r, r32 in zip(names, got, want, w32):
                if r is None:
                    assert a is None
                    continue
                e, e32 = rel_err(a, r), rel_err(r32, r)
                bar = max(2e-6, 4 * e32)
                print('gdp group norm backward %s mod=%d silu=%d %-7s rel err %.2e, fp32 restatement %.2e, bar %.2e'
                      % ((n, p, c), with_mod, act, name, e, e32, bar))
                assert tuple(a.shape) == tuple(r.shape) and e <= bar, (name, with_mod, act, e, bar)
            again = _gn_device(x, g, b, *m, act, dy)
            sliced = _gn_device(wd[..., 4:c + 4], g, b, *m, act, dy)          # x is a channel slice of a wider buffer
            scalar = _gn_device(od[..., 3:c + 3], g, b, *m, act, dy)
            for name, a, r1, r2, r3 in zip(names, got, again, sliced, scalar):
                if a is not None:
                    assert torch.equal(bits(a), bits(r1)) and torch.equal(bits(a), bits(r2)) and torch.equal(bits(a), bits(r3)), name
            one = _gn_device(x[:1], g, b, *((v[:1] for v in m) if with_mod else m), act, dy[:1])
            for k in (0, 3, 4):                                               # a sample alone and inside the batch
                if got[k] is not None:
                    assert torch.equal(bits(one[k][0]), bits(got[k][0])), names[k]


@pytest.mark.parametrize('n,p,c', [(3, 35, 32), (2, 9, 96)])
def test_group_norm_backward_row_strides_of_dy_and_dx(n, p, c):
    """dy read from, and dx written into, channel slices of wider row buffers: 16-byte aligned rows (float4 path) and rows off that
    boundary (scalar path) give the dense call's bits, and nothing outside the slice of dx is written."""
    from sradsgan_amd.model import gdp_train
    tag = 'gdp.gnb.ld.%d.%d.%d' % (n, p, c)
    x, dy = O.det_fill(tag + '.x', (n, p, c), 2.0, 1.5).to(DEV), O.det_fill(tag + '.dy', (n, p, c), 1.0).to(DEV)
    g, b = O.det_fill(tag + '.g', (c,), 0.5, 1.0).to(DEV), O.det_fill(tag + '.b', (c,), 0.5).to(DEV)
    mod = O.det_fill(tag + '.mod', (n, 2 * c), 0.5).to(DEV)
    _, stats = gdp_train.group_norm_fwd_raw(x, g, b, mod, True)
    want = gdp_train.group_norm_bwd_raw(dy, x, stats, g, b, mod, True)
    for pad, off in ((8, 4), (6, 3)):
        wide_dy = torch.zeros(n, p, c + pad, device=DEV)
        wide_dy[..., off:c + off] = dy
        wide_dx = torch.full((n, p, c + pad), 7.0, device=DEV)
        got = gdp_train.group_norm_bwd_raw(wide_dy[..., off:c + off], x, stats, g, b, mod, True, out=wide_dx[..., off:c + off])
        assert got[0].data_ptr() == wide_dx[..., off:c + off].data_ptr() and got[0].stride(1) == c + pad
        for name, a, r in zip(('dx', 'dgamma', 'dbeta', 'dmod'), got, want):
            assert torch.equal(bits(a), bits(r)), (name, pad, off)
        assert float((wide_dx[..., :off] - 7.0).abs().max()) == 0 and float((wide_dx[..., c + off:] - 7.0).abs().max()) == 0
        # each stride on its own: dense dx from a strided dy, strided dx from a dense dy
        assert torch.equal(bits(gdp_train.group_norm_bwd_raw(wide_dy[..., off:c + off], x, stats, g, b, mod, True)[0]), bits(want[0]))
        wide_dx.fill_(7.0)
        gdp_train.group_norm_bwd_raw(dy, x, stats, g, b, mod, True, out=wide_dx[..., off:c + off])
        assert torch.equal(bits(wide_dx[..., off:c + off]), bits(want[0]))


@pytest.mark.parametrize('act', [False, True])
def test_group_norm_takes_the_halves_of_one_row_without_a_copy(act, monkeypatch):
    """scale and shift given as the two halves of one [n, 2 C] row reach the kernel as they lie (ldmod = 2 C): the bits of the mod=
    call, and no concatenation.  Separate tensors are concatenated and give those bits too."""
    from sradsgan_amd.model import gdp_kernels as K
    n, p, c = 2, 16, 64
    x = O.det_fill('gdp.gn.halves.x', (n, p, c), 2.0, 1.5).to(DEV)
    g, b = O.det_fill('gdp.gn.halves.g', (c,), 0.5, 1.0).to(DEV), O.det_fill('gdp.gn.halves.b', (c,), 0.5).to(DEV)
    mod = O.det_fill('gdp.gn.halves.mod', (n, 2 * c), 0.5).to(DEV)
    want = K.group_norm_act(x, g, b, silu=act, mod=mod)
    apart = K.group_norm_act(x, g, b, mod[:, :c].clone(), mod[:, c:].clone(), silu=act)
    assert K._one_row(mod[:, :c], mod[:, c:]).data_ptr() == mod.data_ptr() and K._one_row(mod[:, :c].clone(), mod[:, c:]) is None

    def no_cat(*args, **kw):
        raise AssertionError('group_norm_act concatenated the halves of one row')
    monkeypatch.setattr(torch, 'cat', no_cat)
    got = K.group_norm_act(x, g, b, mod[:, :c], mod[:, c:], silu=act)
    monkeypatch.undo()
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(apart), bits(want))
    assert got.grad_fn is None and float(want.abs().max()) > 0.1
    # halves that carry a gradient: both of them receive it
    dy = O.det_fill('gdp.gn.halves.dy', (n, p, c), 1.0).to(DEV)
    whole, halved = leaf(mod), leaf(mod)
    K.group_norm_act(x, g, b, silu=act, mod=whole).backward(dy)
    K.group_norm_act(x, g, b, halved[:, :c], halved[:, c:], silu=act).backward(dy)
    assert torch.equal(bits(halved.grad), bits(whole.grad)) and float(whole.grad[:, c:].abs().max()) > 0


def test_group_norm_backward_refuses_bad_widths():
    from sradsgan_amd import _hip
    lib = _hip.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for c in (48, 4096):
        rc = lib.srhip_diff_gn_bwd(p, c, p, c, p, p, p, None, None, 0, p, c, p, p, None, None, 0, p, buf.numel() * 4, 1, 4, c, 1, st)
        with pytest.raises(_hip.HipLibraryError, match='C % 32 == 0 and C <= 2048'):
            _hip.check(rc, 'diff_gn_bwd')
    rc = lib.srhip_diff_gn_bwd(p, 32, p, 32, p, p, p, p, p, 32, p, 32, p, p, None, None, 0, p, buf.numel() * 4, 1, 4, 32, 1, st)
    with pytest.raises(_hip.HipLibraryError, match='dscale and dshift'):
        _hip.check(rc, 'diff_gn_bwd')


# ---- SiLU / average pool --------------------------------------------------------------------------------------------------------- #
def test_silu_backward_matches_fp64():
    from sradsgan_amd.model import gdp_train
    x, dy = O.det_fill('gdp.silub.x', (3, 515), 9.0), O.det_fill('gdp.silub.dy', (3, 515), 1.0)

    def ref(dt):
        v = x.to(dt).requires_grad_(True)
        (torch.nn.functional.silu(v) * dy.to(dt)).sum().backward()
        return v.grad
    want, w32 = ref(torch.float64), ref(torch.float32)
    xd = leaf(x)
    gdp_train.silu(xd).backward(dy.to(DEV))
    e, e32 = rel_err(xd.grad, want), rel_err(w32, want)
    bar = max(2e-6, 4 * e32)
    print('gdp silu backward: rel err %.2e, fp32 restatement %.2e, bar %.2e' % (e, e32, bar))
    assert e <= bar


def test_avg_pool_backward_is_a_quarter_of_dy_and_refuses_odd_sizes():
    from sradsgan_amd import _hip
    from sradsgan_amd.model import gdp_train
    x, dy = O.det_fill('gdp.poolb.x', (2, 36, 10, 14), 3.0), O.det_fill('gdp.poolb.dy', (2, 36, 5, 7), 3.0)
    xd = leaf(x)
    gdp_train.avg_pool2x2(xd).backward(dy.to(DEV))
    want = dy.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) * 0.25
    assert tuple(xd.grad.shape) == (2, 36, 10, 14) and torch.equal(xd.grad.cpu(), want)
    assert torch.equal(gdp_train.avg_pool2x2_bwd(dy.to(DEV), (2, 36, 10, 14)).cpu(), want)
    for shape in ((1, 32, 5, 4), (1, 32, 4, 7)):
        with pytest.raises(_hip.HipLibraryError, match='even'):
            gdp_train.avg_pool2x2_bwd(torch.zeros(1, 32, shape[2] // 2, shape[3] // 2, device=DEV), shape)


# ---- attention ------------------------------------------------------------------------------------------------------------------- #
ATTN_CASES = [(2, 4, 32, 36, 6.0), (1, 2, 64, 65, 6.0), (2, 16, 64, 729, 6.0), (1, 1, 64, 1, 6.0), (2, 4, 32, 36, 1.0)]


@pytest.mark.parametrize('n,heads,ch,t,amp', ATTN_CASES)
def test_attention_backward_matches_fp64(n, heads, ch, t, amp):
    """amp 6: sharp soft-maxes (logits of several tens, as the forward's test); amp 1: a mild case."""
    from sradsgan_amd.model import gdp, gdp_train
    tag = 'gdp.attn.%d.%d.%d.%d' % (n, heads, ch, t)                            # amp 6: the forward test's own inputs
    qkv = O.det_fill(tag, (n, t, heads * 3 * ch), amp)
    dout = O.det_fill(tag + '.dout', (n, t, heads * ch), 1.0)
    out64, lse64, want = T.attention_grad(qkv, heads, dout, torch.float64)
    _, lse32, w32 = T.attention_grad(qkv, heads, dout, torch.float32)
    if amp > 1 and t >= 36:
        assert float(lse64.max()) > 30
    qd = leaf(qkv)
    got_out = gdp_train.qkv_attention(qd, heads)
    got_out.backward(dout.to(DEV))
    e, e32 = rel_err(qd.grad, want), rel_err(w32, want)
    bar = max(1e-5, 4 * e32)
    _, out_lse, lse = gdp_train.attention_fwd_lse(qkv.to(DEV), heads)
    el, el32 = rel_err(lse, lse64), rel_err(lse32, lse64)
    lbar = lse_bar(el32)
    print('gdp attention backward %s amp %g: dqkv rel err %.2e, fp32 restatement %.2e, bar %.2e; lse %.2e, fp32 %.2e, bar %.2e (largest %.1f)'
          % ((n, heads, ch, t), amp, e, e32, bar, el, el32, lbar, float(lse64.max())))
    assert tuple(qd.grad.shape) == tuple(qkv.shape) and e <= bar
    assert tuple(lse.shape) == (n, heads, t) and el <= lbar
    plain = gdp.qkv_attention(qkv.to(DEV), heads)
    assert torch.equal(bits(out_lse), bits(plain)) and torch.equal(bits(got_out), bits(plain))      # the lse variant: same `out` bits
    q2 = leaf(qkv)
    gdp_train.qkv_attention(q2, heads).backward(dout.to(DEV))
    assert torch.equal(bits(q2.grad), bits(qd.grad))


def test_attention_backward_refuses_other_head_widths():
    from sradsgan_amd import _hip
    from sradsgan_amd.model import gdp_train
    with pytest.raises(_hip.HipLibraryError, match='32 or 64'):
        gdp_train.qkv_attention(torch.zeros(1, 4, 3 * 48, device=DEV, requires_grad=True), 1)
    lib = _hip.lib()
    buf = torch.zeros(4096, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    with pytest.raises(_hip.HipLibraryError, match='32 or 64'):
        _hip.check(lib.srhip_diff_attn_bwd(p, p, p, p, p, p, 4096 * 4, 1, 4, 1, 48, None), 'diff_attn_bwd')


# ---- forward diffusion ----------------------------------------------------------------------------------------------------------- #
def test_q_sample_matches_fp64_and_keeps_the_condition():
    from sradsgan_amd.model import gdp, gdp_train
    a, b = T.q_coefficients(T.TRAIN_SCHEDULE)
    shape = (4, 7, 9, 3)
    x0, z, cond = O.det_fill('gdp.q.x0', shape, 1.0), O.det_fill('gdp.q.z', shape, 2.5), O.det_fill('gdp.q.cond', shape, 1.0)
    t = torch.tensor([0, 999, 500, 3])                                         # both ends and two values between, in one batch
    buf = torch.cat([torch.full(shape, 7.0), cond], dim=-1).to(DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    gdp_train.q_sample_rows(x0.to(DEV), t.to(DEV), ad, bd, buf[..., :3], noise=z.to(DEV))
    want = a[t].double().reshape(-1, 1, 1, 1) * x0.double() + b[t].double().reshape(-1, 1, 1, 1) * z.double()
    e = rel_err(buf[..., :3], want)
    print('gdp q_sample: rel err %.2e (bar 2e-6)' % e)
    assert e < 2e-6
    assert torch.equal(bits(buf[..., 3:]), bits(cond))                          # channels 3..5 untouched, bit for bit
    # the draws taken in the kernel are randn_rows(seed, step)'s
    drawn = torch.cat([torch.zeros(shape), cond], dim=-1).to(DEV)
    gdp_train.q_sample_rows(x0.to(DEV), t.to(DEV), ad, bd, drawn[..., :3], noise=None, seed=11, step=5)
    eps = gdp.randn_rows(torch.empty(shape, device=DEV), 11, 5)
    gdp_train.q_sample_rows(x0.to(DEV), t.to(DEV), ad, bd, buf[..., :3], noise=eps)
    assert torch.equal(bits(drawn), bits(buf)) and float(eps.std()) > 0.9
    # the module's method: logical [B, C, H, W], the reference's formula
    G = gdp_train.TrainableDiffusion(None, image_size=9)
    G.set_new_noise_schedule(T.TRAIN_SCHEDULE, DEV)
    xt = G.q_sample(x0.permute(0, 3, 1, 2).to(DEV), t, noise=z.permute(0, 3, 1, 2).to(DEV))
    assert tuple(xt.shape) == (4, 3, 7, 9) and rel_err(xt, T.q_sample(x0.permute(0, 3, 1, 2).double(), t, z.permute(0, 3, 1, 2).double(),
                                                                       T.TRAIN_SCHEDULE)) < 2e-6
    with pytest.raises(TypeError, match='int64 device tensor'):
        gdp_train.q_sample_rows(x0.to(DEV), t, ad, bd, buf[..., :3], noise=z.to(DEV))


# ---- the small net --------------------------------------------------------------------------------------------------------------- #
def small_diffusion(conditional=True, prefix='gdp.'):
    from sradsgan_amd.model import gdp_train
    cfg = R.SMALL if conditional else dict(R.SMALL, in_channel=3)
    net = R.init_(gdp_train.TrainableUNet(**cfg), prefix)
    G = gdp_train.TrainableDiffusion(net, image_size=12, channels=3, loss_type='l2', conditional=conditional)
    return G


def small_opt(root, resume=None, phase='train'):
    return {'phase': phase, 'path': {'checkpoint': str(root), 'resume_state': resume},
            'model': {'which_model_G': 'gdp', 'finetune_norm': False, 'beta_schedule': {'train': T.TRAIN_SCHEDULE, 'val': R.LOOP_SCHEDULE}},
            'train': {'optimizer': {'lr': T.LR_ADAM}}}


def named_grads(net):
    return {k: p.grad for k, p in net.named_parameters()}


def state64(net):
    return R.state(net, torch.float64)


@pytest.fixture(scope='module')
def small():
    G = small_diffusion().to(DEV)
    G.set_loss(DEV)
    G.set_new_noise_schedule(T.TRAIN_SCHEDULE, DEV)
    return G, state64(G.denoise_fn)


@pytest.fixture(scope='module')
def floor(small):
    """The float32 CPU restatement's own gradient score against float64, at TRAIN_T and at the fixture's t: what the bars scale."""
    _, sd64 = small
    hr, sr = T.train_inputs()
    g = np.load(os.path.join(GOLD, 'gdp_train.npz'))
    out = {}
    for name, (t, noise) in (('fp64', T.step_inputs(0)), ('fixture', (torch.from_numpy(g['t']), torch.from_numpy(g['noise'])))):
        l64, g64 = T.loss_and_grads(sd64, hr, sr, t, noise, torch.float64)
        _, g32 = T.loss_and_grads(sd64, hr, sr, t, noise, torch.float32)
        out[name] = (t, noise, l64, g64, T.grad_score(g32, g64)[0])
    return out


@pytest.mark.parametrize('mode', MODES)
def test_grad_enabled_forward_has_the_sampler_bits(small, mode):
    """One walk: the frozen gdp.UNet, the same net adopted by TrainableUNet without grad, and with grad enabled, give the same bits."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp, gdp_train
    G, _ = small
    net = G.denoise_fn
    twin = R.init_(gdp.UNet(**R.SMALL)).to(DEV)
    x = ops.nhwc(R.small_input().to(DEV))
    emb = gdp.timestep_embedding(torch.tensor(T.TRAIN_T), 64).to(DEV)
    with ops.conv_math(mode):
        with torch.enable_grad():
            y = net.forward_embedded(x, emb)
        want = twin.forward_embedded(x, emb)
        with torch.no_grad():
            quiet = net.forward_embedded(x, emb)
    assert y.requires_grad and not want.requires_grad and not quiet.requires_grad
    assert torch.equal(bits(y), bits(want)) and torch.equal(bits(quiet), bits(want))
    assert not any(p.requires_grad for p in twin.parameters())
    assert want.grad_fn is None and quiet.grad_fn is None
    adopted = gdp_train.TrainableUNet.adopt(twin)
    with ops.conv_math(mode):
        with torch.no_grad():
            quiet2 = adopted.forward_embedded(x, emb)
        with torch.enable_grad():
            y2 = adopted.forward_embedded(x, emb)
    assert quiet2.grad_fn is None and not quiet2.requires_grad and y2.requires_grad
    assert torch.equal(bits(quiet2), bits(want)) and torch.equal(bits(y2), bits(want))


@pytest.mark.parametrize('mode', MODES)
def test_loss_and_gradients_match_fp64_and_the_reference(small, floor, mode):
    from sradsgan_amd import ops
    G, _ = small
    net = G.denoise_fn
    hr, sr = T.train_inputs()
    x_in = {'HR': hr.to(DEV), 'SR': sr.to(DEV)}
    fix = np.load(os.path.join(GOLD, 'gdp_train.npz'))
    for name in ('fp64', 'fixture'):
        t, noise, l64, g64, s32 = floor[name]
        bar = GRAD_FACTOR[mode] * s32
        for p in net.parameters():
            p.grad = None
        with ops.conv_math(mode):
            loss = G(x_in, noise.to(DEV), t=t.to(DEV))
            (loss / hr.numel()).backward()
        loss = loss.detach()
        got = named_grads(net)
        assert len(got) == 144 and all(v is not None and float(v.abs().max()) > 0 for v in got.values())
        dl = abs(float(loss) / hr.numel() - l64)
        score, key = T.grad_score(got, g64)
        print('gdp p_losses %s %s: loss / numel %.6f, |d| vs fp64 %.2e (bar %.0e); gradient score %.2e at %s, fp32 restatement %.2e, bar %.2e'
              % (name, mode, float(loss) / hr.numel(), dl, LOSS_BAR, score, key, s32, bar))
        assert dl <= LOSS_BAR and score <= bar
        if name == 'fixture':                                                   # the reference's own float32 vectors
            dref = abs(float(loss) / hr.numel() - float(fix['loss']) / int(fix['numel']))
            sref, kref = T.digest_score(got, fix)
            print('gdp p_losses vs the reference %s: loss %.2e (bar %.0e), gradient score %.2e at %s (bar %.2e)'
                  % (mode, dref, LOSS_BAR, sref, kref, bar))
            assert dref <= LOSS_BAR and sref <= bar
    for p in net.parameters():
        p.grad = None


def test_half_mode_is_replaced_by_bf16x3_for_the_whole_step(small, tmp_path):
    """Under conv arithmetic `half` the U-Net runs `bf16x3`, backward included: loss and every gradient of a bare
    p_losses(...).backward() are bit-equal to the bf16x3 run's, the caller's mode is `half` again afterwards, and a DDPM step leaves
    the parameters and gradients of the bf16x3 step."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp_train
    G, _ = small
    net = G.denoise_fn
    hr, sr = T.train_inputs()
    x_in = {'HR': hr.to(DEV), 'SR': sr.to(DEV)}
    t, noise = T.step_inputs(0)
    runs = {}
    for mode in ('bf16x3', 'half'):
        for p in net.parameters():
            p.grad = None
        with ops.conv_math(mode):
            loss = G(x_in, noise.to(DEV), t=t.to(DEV))
            assert ops.get_conv_math() == mode
            loss.backward()
            assert ops.get_conv_math() == mode                                  # put back when the backward pass ended
        runs[mode] = (loss.detach().clone(), {k: v.clone() for k, v in named_grads(net).items()})
    for p in net.parameters():
        p.grad = None
    assert torch.equal(bits(runs['half'][0]), bits(runs['bf16x3'][0]))
    for k, v in runs['bf16x3'][1].items():
        assert torch.equal(bits(runs['half'][1][k]), bits(v)), k
    after = {}
    for mode in ('bf16x3', 'half'):
        with ops.conv_math(mode):
            model = gdp_train.DDPM(small_opt(tmp_path), netG=small_diffusion())
            model.feed_data({'HR': hr, 'SR': sr, 'LR': sr})
            model.optimize_parameters(noise.to(DEV), t=t.to(DEV))
            assert ops.get_conv_math() == mode
        after[mode] = (model.arena.flat_p.clone(), model.arena.flat_g.clone())
    assert torch.equal(bits(after['half'][0]), bits(after['bf16x3'][0])) and torch.equal(bits(after['half'][1]), bits(after['bf16x3'][1]))


def test_p_losses_draws_t_and_noise_when_none_are_given(small):
    from sradsgan_amd import ops
    G, _ = small
    hr, sr = T.train_inputs()
    x_in = {'HR': hr.to(DEV), 'SR': sr.to(DEV), 'LR': sr.to(DEV)}
    torch.manual_seed(5)
    a = G(x_in)
    torch.manual_seed(5)
    b = G(x_in)
    c = G(x_in)
    assert a.dim() == 0 and bool(torch.isfinite(a)) and torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c))
    t, noise = T.step_inputs(0)
    G.loss_type = 'l1'
    try:
        G.set_loss(DEV)
        with ops.conv_math('fp32'):
            l1 = G(x_in, noise.to(DEV), t=t.to(DEV)).detach()
    finally:
        G.loss_type = 'l2'
        G.set_loss(DEV)
    _, sd64 = small
    want, _ = T.loss_and_grads(sd64, hr, sr, t, noise, loss='l1')
    print('gdp p_losses l1: loss / numel %.6f, |d| vs fp64 %.2e (bar %.0e)' % (float(l1) / hr.numel(), abs(float(l1) / hr.numel() - want), LOSS_BAR))
    assert abs(float(l1) / hr.numel() - want) <= LOSS_BAR


# ---- three Adam steps, then sampling ---------------------------------------------------------------------------------------------- #
def _f32(v):
    return float(np.float32(v))


@pytest.fixture(scope='module', params=MODES)
def trained(request, tmp_path_factory):
    """Three optimize_parameters() steps with fixed (t, noise) per step; records what the tests below assert on."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp_train
    mode = request.param
    hr, sr = T.train_inputs()
    with ops.conv_math(mode):
        model = gdp_train.DDPM(small_opt(tmp_path_factory.mktemp('gdp_train_' + mode)), netG=small_diffusion())
        net = model.netG.denoise_fn
        names = [k for k, _ in net.named_parameters()]
        params = [p for _, p in net.named_parameters()]
        start = state64(net)
        hyper = dict(lr=_f32(T.LR_ADAM), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8))     # what the kernel receives (floats)
        q64 = [start[k].clone().requires_grad_(True) for k in names]
        q32 = [start[k].float().clone().requires_grad_(True) for k in names]
        o64, o32 = torch.optim.Adam(q64, **hyper), torch.optim.Adam(q32, **hyper)
        model.feed_data({'HR': hr, 'SR': sr, 'LR': sr})
        rec = []
        for k in range(3):
            t, noise = T.step_inputs(k)
            before = state64(net)
            model.optimize_parameters(noise.to(DEV), t=t.to(DEV))
            grads = {n: p.grad.detach().cpu().clone() for n, p in zip(names, params)}
            after = state64(net)
            prev64, prev32 = [q.detach().clone() for q in q64], [q.detach().clone() for q in q32]
            for q, d, n in zip(q64, q32, names):
                q.grad, d.grad = grads[n].double(), grads[n].clone()
            o64.step()
            o32.step()
            a = model.arena
            adam = {'dp': [0.0, 0.0], 'm': [0.0, 0.0], 'v': [0.0, 0.0]}
            mmax = max(float(o64.state[q]['exp_avg'].abs().max()) for q in q64)
            vmax = max(float(o64.state[q]['exp_avg_sq'].abs().max()) for q in q64)
            for n, p, o, q, d, p64, p32 in zip(names, a.params, a.offsets, q64, q32, prev64, prev32):
                view = lambda flat: flat[o:o + p.numel()].view(p.shape).cpu().double()
                step64 = q.detach() - p64
                adam['dp'][0] = max(adam['dp'][0], float(((after[n] - before[n]) - step64).abs().max()) / hyper['lr'])
                adam['dp'][1] = max(adam['dp'][1], float(((d.detach() - p32).double() - step64).abs().max()) / hyper['lr'])
                for key, flat, slot, top in (('m', a.exp_avg, 'exp_avg', mmax), ('v', a.exp_avg_sq, 'exp_avg_sq', vmax)):
                    adam[key][0] = max(adam[key][0], float((view(flat) - o64.state[q][slot]).abs().max()) / top)
                    adam[key][1] = max(adam[key][1], float((o32.state[d][slot].double() - o64.state[q][slot]).abs().max()) / top)
            rec.append(dict(t=t, noise=noise, before=before, after=after, grads=grads, loss=float(model.log_dict['l_pix']), adam=adam,
                            views=a.check_views(), log_is_device_scalar=model.log_dict['l_pix'].is_cuda and model.log_dict['l_pix'].dim() == 0))
    return mode, model, start, rec


def test_adam_steps_follow_torch_adam_on_the_device_gradients(trained):
    mode, model, _, rec = trained
    for k, r in enumerate(rec):
        for key in ('dp', 'm', 'v'):
            e, yard = r['adam'][key]
            print('gdp train %s step %d adam %-2s: err %.3e, torch fp32 on the same gradients %.3e, bar %.3e' % (mode, k + 1, key, e, yard, 4 * yard))
            assert e <= 4 * yard, (k, key, e, yard)
        assert r['views'] and r['log_is_device_scalar']
    assert model.steps == 3 and float(model.arena.step_state[0]) == 3.0


def test_step_losses_match_fp64_at_the_device_parameters(trained):
    """Each step's loss against the restatement evaluated at the device's parameters BEFORE that step: a stale packed weight (the
    forward reading last step's image of a weight) shows here."""
    mode, _, _, rec = trained
    hr, sr = T.train_inputs()
    for k, r in enumerate(rec):
        want, _ = T.loss_and_grads(r['before'], hr, sr, r['t'], r['noise'])
        print('gdp train %s step %d: loss %.6f, |d| vs fp64 %.2e (bar %.0e)' % (mode, k + 1, r['loss'], abs(r['loss'] - want), LOSS_BAR))
        assert abs(r['loss'] - want) <= LOSS_BAR
    assert abs(rec[0]['loss'] - rec[2]['loss']) > 1e-4


def test_second_step_gradients_are_of_that_step_alone(trained):
    """Step 2's gradients at step 2's parameters: one that was not zeroed carries step 1's on top."""
    mode, _, _, rec = trained
    hr, sr = T.train_inputs()
    r = rec[1]
    _, g64 = T.loss_and_grads(r['before'], hr, sr, r['t'], r['noise'], torch.float64)
    _, g32 = T.loss_and_grads(r['before'], hr, sr, r['t'], r['noise'], torch.float32)
    s32 = T.grad_score(g32, g64)[0]
    score, key = T.grad_score(r['grads'], g64)
    print('gdp train %s step 2: gradient score %.2e at %s, fp32 restatement %.2e, bar %.2e' % (mode, score, key, s32, GRAD_FACTOR[mode] * s32))
    assert score <= GRAD_FACTOR[mode] * s32


def test_sampling_after_training_sees_the_updated_weights(trained):
    from sradsgan_amd import ops
    mode, model, start, rec = trained
    g = np.load(os.path.join(GOLD, 'gdp_loop.npz'))
    noise = torch.from_numpy(g['noise'])
    _, sr = T.train_inputs()
    o = R.LOOP_SCHEDULE
    betas = R.betas64(o['schedule'], o['n_timestep'], o['linear_start'], o['linear_end'])
    now = state64(model.netG.denoise_fn)
    want = R.sample(now, sr.double(), noise, betas, R.SMALL, prefix='')[-1]
    old = R.sample(start, sr.double(), noise, betas, R.SMALL, prefix='')[-1]
    model.set_new_noise_schedule(o, schedule_phase='val')
    with ops.conv_math(mode):
        model.test(noise=noise.to(DEV))
    e, moved = rel_err(model.SR, want), rel_err(model.SR, old)
    print('gdp train %s then sample: vs fp64 at the current weights %.2e (bar %.0e), vs the untrained weights %.2e' % (mode, e, NET_BAR[mode], moved))
    assert tuple(model.SR.shape) == (3, 12, 12) and e <= NET_BAR[mode] and moved > 10 * NET_BAR[mode]
    vis = model.get_current_visuals()
    assert sorted(vis) == ['HR', 'INF', 'LR', 'SR'] and not vis['SR'].is_cuda
    assert model.arena.check_views()


# ---- checkpoint -------------------------------------------------------------------------------------------------------------------- #
def test_checkpoint_resumes_bit_equal_and_loads_into_torch_adam(tmp_path):
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp_train
    hr, sr = T.train_inputs()
    data = {'HR': hr, 'SR': sr, 'LR': sr}
    (t0, z0), (t1, z1) = T.step_inputs(0), T.step_inputs(1)
    with ops.conv_math('fp32'):
        a = gdp_train.DDPM(small_opt(tmp_path), netG=small_diffusion())
        a.feed_data(data)
        a.optimize_parameters(z0.to(DEV), t=t0.to(DEV))
        gen_path, opt_path = a.save_network(7, 123)
        assert os.path.basename(gen_path) == 'I123_E7_gen.pth' and os.path.basename(opt_path) == 'I123_E7_opt.pth'
        a.optimize_parameters(z1.to(DEV), t=t1.to(DEV))
        # a fresh model with OTHER initial weights: everything must come from the files
        b = gdp_train.DDPM(small_opt(tmp_path, resume=os.path.join(str(tmp_path), 'I123_E7')), netG=small_diffusion(prefix='gdp.other.'))
        assert (b.begin_step, b.begin_epoch, b.steps) == (123, 7, 1) and b.arena.check_views()
        b.feed_data(data)
        b.optimize_parameters(z1.to(DEV), t=t1.to(DEV))
    for (k, p), (_, q) in zip(a.netG.named_parameters(), b.netG.named_parameters()):
        assert torch.equal(bits(p), bits(q)), k
    assert torch.equal(bits(a.arena.exp_avg), bits(b.arena.exp_avg)) and torch.equal(bits(a.arena.exp_avg_sq), bits(b.arena.exp_avg_sq))
    assert torch.equal(bits(a.log_dict['l_pix']), bits(b.log_dict['l_pix']))
    # the optimiser file: the reference's dict around torch.optim.Adam's own state dict
    saved = torch.load(opt_path, map_location='cpu')
    assert sorted(saved) == ['epoch', 'iter', 'optimizer', 'scheduler'] and saved['scheduler'] is None and (saved['epoch'], saved['iter']) == (7, 123)
    shaped = [torch.nn.Parameter(torch.zeros(p.shape)) for p in a.netG.parameters()]
    opt = torch.optim.Adam(shaped, lr=T.LR_ADAM)
    opt.load_state_dict(saved['optimizer'])
    c = gdp_train.DDPM(small_opt(tmp_path, resume=os.path.join(str(tmp_path), 'I123_E7')), netG=small_diffusion(prefix='gdp.other.'))
    for q, p, o in zip(shaped, c.arena.params, c.arena.offsets):
        st = opt.state[q]
        assert float(st['step']) == 1.0
        assert torch.equal(st['exp_avg'], c.arena.exp_avg[o:o + p.numel()].view(p.shape).cpu())
        assert torch.equal(st['exp_avg_sq'], c.arena.exp_avg_sq[o:o + p.numel()].view(p.shape).cpu())
    # and the other way round: what torch.optim.Adam saves loads into the arena
    m1, v1 = c.arena.exp_avg.clone(), c.arena.exp_avg_sq.clone()
    c.arena.exp_avg.fill_(3.0)
    c.steps = 0
    c.load_optimizer_state_dict(opt.state_dict())
    assert c.steps == 1 and float(c.arena.step_state[0]) == 1.0
    assert torch.equal(bits(c.arena.exp_avg), bits(m1)) and torch.equal(bits(c.arena.exp_avg_sq), bits(v1))
    gen = torch.load(gen_path, map_location='cpu')
    assert sorted(gen) == sorted(a.netG.state_dict()) and 'betas' in gen and 'denoise_fn.out.2.weight' in gen


def test_a_net_that_was_sampled_from_trains_on_fresh_packed_weights(tmp_path):
    """A frozen gdp.UNet that has run (its weights are packed as static images, outside the per-step re-pack), adopted and trained:
    the second step's loss must be the restatement's at the UPDATED parameters, and every conv / linear weight must be registered."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp, gdp_train
    hr, sr = T.train_inputs()
    frozen = R.init_(gdp.UNet(**R.SMALL)).to(DEV)
    emb = gdp.timestep_embedding(torch.tensor(T.TRAIN_T), 64).to(DEV)
    with ops.conv_math('fp32'):
        frozen.forward_embedded(ops.nhwc(R.small_input().to(DEV)), emb)
        assert all(hasattr(p, '_srhip_packed') and p._srhip_static for p in frozen.parameters() if p.dim() >= 2)
        net = gdp_train.TrainableUNet.adopt(frozen)
        model = gdp_train.DDPM(small_opt(tmp_path), netG=gdp_train.TrainableDiffusion(net, image_size=12, channels=3, conditional=True))
        model.feed_data({'HR': hr, 'SR': sr, 'LR': sr})
        for k in range(2):
            t, noise = T.step_inputs(k)
            before = state64(net)
            model.optimize_parameters(noise.to(DEV), t=t.to(DEV))
            want, _ = T.loss_and_grads(before, hr, sr, t, noise)
            got = float(model.log_dict['l_pix'])
            print('gdp adopted net step %d: loss %.6f, |d| vs fp64 at the current weights %.2e (bar %.0e)' % (k + 1, got, abs(got - want), LOSS_BAR))
            assert abs(got - want) <= LOSS_BAR
    registered = {id(ent[0]()) for ent in ops._registry.entries}
    assert all(id(p) in registered for p in net.parameters() if p.dim() >= 2)
    assert model.arena.check_views()


def test_mark_trainable_undoes_mark_static_on_a_net_that_has_run():
    """ops.mark_trainable on a net that was sampled from: no packed image and no static mark stay on its parameters, no live registry
    entry refers to them, and the next forward packs them again and registers them for the per-step re-pack."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp
    net = R.init_(gdp.UNet(**R.SMALL)).to(DEV)
    x = ops.nhwc(R.small_input().to(DEV))
    emb = gdp.timestep_embedding(torch.tensor(T.TRAIN_T), 64).to(DEV)
    weights = [p for p in net.parameters() if p.dim() >= 2]
    registered = lambda: {id(ent[0]()) for ent in ops._registry.entries}
    with ops.conv_math('fp32'):
        want = net.forward_embedded(x, emb)
        assert all(hasattr(p, '_srhip_packed') and p._srhip_static for p in weights)
        assert not any(id(p) in registered() for p in weights)                  # static: packed once, outside the re-pack
        ops.mark_trainable(net)
        assert not any(hasattr(p, '_srhip_packed') or hasattr(p, '_srhip_static') for p in net.parameters())
        assert not any(id(p) in registered() for p in net.parameters())
        again = net.forward_embedded(x, emb)
        assert all(hasattr(p, '_srhip_packed') for p in weights) and all(id(p) in registered() for p in weights)
        assert torch.equal(bits(again), bits(want))
        ops.mark_trainable(net)                                                  # a net with registered images: they leave the registry
        assert not any(id(p) in registered() for p in net.parameters()) and ops._registry.dirty


# ---- unconditional, and the batch helper ------------------------------------------------------------------------------------------- #
def test_unconditional_net_trains_reproducibly():
    G = small_diffusion(conditional=False, prefix='gdp.uncond.').to(DEV)
    G.set_loss(DEV)
    G.set_new_noise_schedule(T.TRAIN_SCHEDULE, DEV)
    hr, _ = T.train_inputs()
    t = torch.tensor(T.TRAIN_T).to(DEV)
    from sradsgan_amd import ops
    runs = []
    for _ in range(2):
        for p in G.parameters():
            p.grad = None
        with ops.conv_math('fp32'):
            loss = G({'HR': hr.to(DEV)}, t=t, seed=9)
            loss.backward()
        runs.append((loss.detach().clone(), [p.grad.clone() for p in G.parameters()]))
    assert bool(torch.isfinite(runs[0][0])) and torch.equal(bits(runs[0][0]), bits(runs[1][0]))
    assert all(torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all()) for a, b in zip(runs[0][1], runs[1][1]))
    other = G({'HR': hr.to(DEV)}, t=t, seed=10)
    assert not torch.equal(bits(other), bits(runs[0][0]))
    # against the restatement on the restated draws
    z = torch.from_numpy(R.philox_normal(9, 0, hr.numel()).reshape(2, 12, 12, 3).transpose(0, 3, 1, 2).copy())
    want, _ = T.loss_and_grads(state64(G.denoise_fn), hr, None, t.cpu(), z, cfg=dict(R.SMALL, in_channel=3))
    print('gdp unconditional p_losses: |d| vs fp64 %.2e (bar %.0e)' % (abs(float(runs[0][0]) / hr.numel() - want), LOSS_BAR))
    assert abs(float(runs[0][0]) / hr.numel() - want) <= LOSS_BAR


def test_training_batch_bytes_match_the_composition():
    from oracle import pil_resample_ref as P
    from sradsgan_amd.model import gdp_train
    hr = (O.det_fill('gdp.train.u8', (2, 12, 12, 3), 0.5, 0.5).numpy() * 255).round().astype(np.uint8)
    out = gdp_train.training_batch(torch.from_numpy(hr).to(DEV), 3)
    lr = np.stack([P.resize_u8(im, 3, 3, 'bicubic') for im in hr])
    sr = np.stack([P.resize_u8(im, 12, 12, 'bicubic') for im in lr])
    assert sorted(out) == ['HR', 'LR', 'SR']
    for key, want in (('HR', hr), ('LR', lr), ('SR', sr)):
        got = out[key]
        assert tuple(got.shape) == (2, 3) + want.shape[1:3] and got.dtype == torch.float32
        back = ((got.cpu().double() + 1) / 2 * 255).round().permute(0, 2, 3, 1).numpy().astype(np.uint8)
        assert np.array_equal(back, want), key
        ref = (torch.from_numpy(want).float() / 255.0 * 2.0 + (-1.0)).permute(0, 3, 1, 2)
        assert float((got.cpu() - ref).abs().max()) <= 2 ** -23, key
    assert len(np.unique(sr)) > 16
