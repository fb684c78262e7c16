"""HAT on the HIP path (sradsgan_amd.model.hat, csrc/hat.hip) in split-bf16 and exact-fp32 conv arithmetic: LayerNorm, GELU, window
self-attention with and without the shift, overlapping cross-attention (border windows included), the bias-table gradient and the
HAB combine with CAB's 96-channel attention, each against fp64 torch and rerun bit-identically; the generator against the reference's
vectors (tests/golden/hat_*.npz) and its gradients against the fp64 restatement (tests/hat_ref.py); the default 6 x 6 configuration
at x8, crop 216, B = 2 against fp64 on the device; two train_step iterations against the restatement plus Adam; a train-mode step
with replayed drop-path factors; a forward in 'half' arithmetic; x9 at window 9 refused, x9 at window 8 trained."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O
from tests import hat_ref as R
from tests.test_hat_cpu import CASES, DEPTHS, build, digest, golden, rel, unique_names

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CL = torch.channels_last
MODES = ['bf16x3', 'fp32']


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def dev(t):
    return t.to(DEV).contiguous(memory_format=CL)


def hip_model(G, **kw):
    from sradsgan_amd.model import hat as H
    args = dict(upscale=G.upscale, window_size=G.window_size, depths=tuple(len(l.residual_group.blocks) for l in G.layers),
                num_heads=(6,) * len(G.layers), img_size=G.patch_embed.img_size)
    args.update(kw)
    M = H.GeneratorResNet(**args)
    M.load_state_dict(G.state_dict(), strict=True)
    return M.to(DEV).eval()                  # drop path off (the fixtures come from eval mode); the drop-path test calls train()


def grad_score(hip, sd64):
    """worst |dg| over max(|g| of the parameter, 1e-2 |g| of the network) (tests/test_drcan_gpu.py)"""
    hp = dict(hip.named_parameters())
    gnet = max(float(sd64[k].grad.abs().max()) for k in hp)
    worst, wk = 0.0, None
    for k, p in hp.items():
        g = sd64[k].grad
        d = float((p.grad.detach().cpu().double() - g.detach().cpu().double()).abs().max())
        s = d / max(float(g.abs().max()), 1e-2 * gnet)
        if s > worst:
            worst, wk = s, k
    return worst, wk


def twice(fn):
    """run fn twice; the results (tuples of tensors) must be bit-identical"""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        if u is not None:
            assert torch.equal(u, v)
    return a


# ---- kernels ------------------------------------------------------------------------------------------------------------------ #

def test_layer_norm_and_gelu_match_fp64_and_rerun_bit_identically():
    from sradsgan_amd import ops
    x = dev(O.det_fill('hatk.ln.x', (2, 96, 9, 18), 1.0, 0.3))
    g = O.det_fill('hatk.ln.g', (96,), 0.2, 1.0).to(DEV)
    b = O.det_fill('hatk.ln.b', (96,), 0.1).to(DEV)
    r = dev(O.det_fill('hatk.ln.r', (2, 96, 9, 18), 1.0))

    def run():
        xs, gs, bs = [t.detach().clone().requires_grad_() for t in (x, g, b)]
        y = ops.layer_norm(xs, gs, bs)
        (y * r).sum().backward()
        return y, xs.grad, gs.grad, bs.grad
    y, dx, dg, db = twice(run)
    x64, g64, b64 = [t.detach().cpu().double().requires_grad_() for t in (x, g, b)]
    y64 = F.layer_norm(x64.permute(0, 2, 3, 1), (96,), g64, b64, 1e-5).permute(0, 3, 1, 2)
    (y64 * r.cpu().double()).sum().backward()
    for got, want in ((y, y64), (dx, x64.grad), (dg, g64.grad), (db, b64.grad)):
        assert rel_err(got, want) < 2e-6

    z = dev(O.det_fill('hatk.gelu.x', (2, 32, 9, 18), 4.0))

    def run_g():
        zs = z.detach().clone().requires_grad_()
        y = ops.gelu(zs)
        (y * r[:, :32]).sum().backward()
        return y, zs.grad
    yg, dz = twice(run_g)
    z64 = z.detach().cpu().double().requires_grad_()
    yg64 = F.gelu(z64)
    (yg64 * r[:, :32].cpu().double()).sum().backward()
    assert rel_err(yg, yg64) < 2e-6 and rel_err(dz, z64.grad) < 2e-6


def attn_ref64(qkv, table, kind, ws, shift):
    """the reference's WindowAttention (hat.py:174-199, with HAB's roll / partition / reverse) or OCAB's attention (:357-405) on
    qkv [n, 288, h, w], fp64, up to the proj Linear"""
    n, _, h, w = qkv.shape
    c, heads = 96, 6
    t = qkv.permute(0, 2, 3, 1)
    if kind == 0:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift else t
        tw = R.window_partition(t, ws).view(-1, ws * ws, 3 * c)
        b_, nq, _ = tw.shape
        p = tw.reshape(b_, nq, 3, heads, 16).permute(2, 0, 3, 1, 4)
        q, k, v = p[0] * 0.25, p[1], p[2]
        rpi, nk = R.rpi_sa(ws), nq
    else:
        ows = ws + ws // 2
        q = R.window_partition(t[..., :c].contiguous(), ws).view(-1, ws * ws, c)
        kv = F.unfold(torch.cat((qkv[:, c:2 * c], qkv[:, 2 * c:]), 1), (ows, ows), stride=ws, padding=(ows - ws) // 2)
        nw = kv.shape[-1]
        kv = kv.view(n, 2, c, ows * ows, nw).permute(1, 0, 4, 3, 2).reshape(2, n * nw, ows * ows, c)
        b_, nq, _ = q.shape
        nk = ows * ows
        q = q.reshape(b_, nq, heads, 16).permute(0, 2, 1, 3) * 0.25
        k = kv[0].reshape(b_, nk, heads, 16).permute(0, 2, 1, 3)
        v = kv[1].reshape(b_, nk, heads, 16).permute(0, 2, 1, 3)
        rpi = R.rpi_oca(ws)
    a = q @ k.transpose(-2, -1) + table[rpi.view(-1)].view(nq, nk, -1).permute(2, 0, 1).unsqueeze(0)
    if kind == 0 and shift:
        m = R.shift_mask(h, w, ws, shift).to(a.dtype)
        nw = m.shape[0]
        a = (a.view(b_ // nw, nw, heads, nq, nk) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, nq, nk)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(b_, nq, c)
    o = R.window_reverse(o.view(-1, ws, ws, c), ws, h, w)
    if kind == 0 and shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.permute(0, 3, 1, 2)


@pytest.mark.parametrize('kind,ws,shift,hw', [(0, 9, 0, (18, 27)), (0, 9, 4, (18, 27)), (0, 8, 4, (16, 24)), (0, 9, 4, (9, 9)),
                                              (1, 9, 0, (18, 27)), (1, 8, 0, (16, 24)), (1, 9, 0, (9, 9))])
def test_window_attention_matches_fp64_and_reruns_bit_identically(kind, ws, shift, hw):
    from sradsgan_amd import ops
    tn = (2 * ws - 1) ** 2 if kind == 0 else (ws + (ws + ws // 2) - 1) ** 2
    qkv = dev(O.det_fill('hatk.attn.qkv.%d.%d' % (kind, ws), (2, 288, hw[0], hw[1]), 1.5))
    tab = O.det_fill('hatk.attn.tab.%d.%d' % (kind, ws), (tn, 6), 0.5).to(DEV)
    r = dev(O.det_fill('hatk.attn.r', (2, 96, hw[0], hw[1]), 1.0))

    def run():
        qs, ts = qkv.detach().clone().requires_grad_(), tab.detach().clone().requires_grad_()
        o = ops.window_attention(qs, ts, kind, ws, shift)
        (o * r).sum().backward()
        return o, qs.grad, ts.grad
    o, dq, dt = twice(run)
    q64, t64 = qkv.detach().cpu().double().requires_grad_(), tab.detach().cpu().double().requires_grad_()
    o64 = attn_ref64(q64, t64, kind, ws, shift)
    (o64 * r.cpu().double()).sum().backward()
    e = (rel_err(o, o64), rel_err(dq, q64.grad), rel_err(dt, t64.grad))
    print('attention kind %d ws %d shift %d %s: out %.1e dqkv %.1e dtable %.1e' % ((kind, ws, shift, hw) + e))
    assert max(e) < 1e-5
    if kind == 1:      # border windows: keys in the zero padding get no gradient, every table row gets one
        assert (t64.grad != 0).all()


@pytest.mark.parametrize('kb', [None, 'drop'])
def test_hab_combine_with_96_channel_attention_matches_fp64(kb):
    from sradsgan_amd import ops
    shape = (3, 96, 9, 18)
    x, a, u = [dev(O.det_fill('hatk.cmb.%s' % s, shape, 1.0)) for s in 'xau']
    w1 = O.det_fill('hatk.cmb.w1', (3, 96, 1, 1), 0.3).to(DEV)
    b1 = O.det_fill('hatk.cmb.b1', (3,), 0.1).to(DEV)
    w2 = O.det_fill('hatk.cmb.w2', (96, 3, 1, 1), 0.3).to(DEV)
    b2 = O.det_fill('hatk.cmb.b2', (96,), 0.1).to(DEV)
    k = None if kb is None else torch.tensor([1 / 0.9, 0.0, 1 / 0.9], device=DEV)
    r = dev(O.det_fill('hatk.cmb.r', shape, 1.0))
    leaves = (x, a, u, w1, b1, w2, b2)

    def run():
        ls = [t.detach().clone().requires_grad_() for t in leaves]
        y = ops.hab_combine(ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], ls[6], kb=k)
        y2 = ops.hab_combine(y, ls[1], kb=k)                        # the MLP branch form
        (y2 * r).sum().backward()
        return (y2,) + tuple(t.grad for t in ls)
    got = twice(run)
    l64 = [t.detach().cpu().double().requires_grad_() for t in leaves]
    x6, a6, u6, w16, b16, w26, b26 = l64
    s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(u6.mean((2, 3), keepdim=True), w16, b16)), w26, b26))
    kk = torch.ones(3, dtype=torch.float64) if k is None else k.cpu().double()
    y = x6 + kk.view(-1, 1, 1, 1) * a6 + (u6 * s) * 0.01
    y2 = y + kk.view(-1, 1, 1, 1) * a6
    (y2 * r.cpu().double()).sum().backward()
    want = (y2,) + tuple(t.grad for t in l64)
    for gt, wt in zip(got, want):
        assert rel_err(gt, wt) < 1e-5


# ---- the generator ------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_generator_matches_reference_vectors_and_fp64_gradients(mode, name):
    from sradsgan_amd import ops
    g = golden(name)
    scale, ws, shape = CASES[name]
    ref = build(name)
    G = hip_model(ref)
    x, t = R.inputs(name, shape, scale, ws)
    with ops.conv_math(mode):
        y = G(dev(x))
        l1 = ops.l1_mean(y, dev(t))
        mse = ops.mse_mean(y, dev(t))
        l1.backward()
    torch.cuda.synchronize()
    e_y = rel(O.digest(y, full_max=4096, nsample=4096), g['y'])
    print('hat %s %s: output %.2e l1 %.2e mse %.2e' % (name, mode, e_y, abs(l1.item() - float(g['l1'])),
                                                       abs(mse.item() - float(g['mse']))))
    assert e_y < 1e-4
    assert abs(l1.item() - float(g['l1'])) < 1e-5 and abs(mse.item() - float(g['mse'])) < 1e-5
    sd = R.state(ref, torch.float64)
    F.l1_loss(R.forward(sd, x.double(), R.config(scale, ws, DEPTHS)), t.double()).backward()
    score, k = grad_score(G, sd)
    print('hat %s %s: worst gradient score %.2e (%s)' % (name, mode, score, k))
    assert score < 2e-3
    hp = dict(G.named_parameters())
    assert rel(np.concatenate([digest(hp[k].grad) for k in unique_names(G)]), g['grads']) < 2e-2


@pytest.mark.parametrize('mode', MODES)
def test_default_configuration_at_x8_crop_216_matches_fp64_on_device(mode):
    """GeneratorResNet(upscale=8, img_size=27) as the trainer builds it (6 RHAGs x 6 HABs, window 9), B = 2, 27 -> 216: output and
    every parameter gradient of one backward against the fp64 restatement on the same device."""
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    ref = R.init_(H.GeneratorResNet(upscale=8, img_size=27))
    G = hip_model(ref)
    x = O.det_fill('hat.big.x', (2, 3, 27, 27), 0.5, 0.5)
    r = O.det_fill('hat.big.r', (2, 3, 216, 216), 1.0)
    with ops.conv_math(mode):
        y = G(dev(x))
        (y * dev(r)).sum().backward()
    torch.cuda.synchronize()
    sd = R.state(ref, torch.float64, DEV)
    y64 = R.forward(sd, x.double().to(DEV), R.config(8, 9, (6,) * 6, 27))
    (y64 * r.double().to(DEV)).sum().backward()
    e = rel_err(y, y64)
    score, k = grad_score(G, sd)
    print('hat 6x6 x8 %s: output %.2e, worst gradient score %.2e (%s)' % (mode, e, score, k))
    assert e < 1e-4
    assert score < (1e-2 if mode == 'bf16x3' else 5e-3)


def _adam64(sd, names, lr, betas):
    return torch.optim.Adam([sd[k] for k in names], lr=lr, betas=betas)


def test_two_train_steps_match_the_restatement_with_adam():
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    name = 'x4'
    scale, ws, shape = CASES[name]
    ref = build(name)
    G = hip_model(ref)
    G.eval()                                                             # drop path off: the steps are deterministic
    x, t = R.inputs(name, shape, scale, ws)
    opt = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.99))
    sd = R.state(ref, torch.float64)
    names = unique_names(G)
    opt64 = _adam64(sd, names, 2e-4, (0.9, 0.99))
    cfg = R.config(scale, ws, DEPTHS)
    for it in range(2):
        with ops.conv_math('fp32'):
            loss = H.train_step(G, opt, dev(x), dev(t))
        opt64.zero_grad()
        l64 = F.l1_loss(R.forward(sd, x.double(), cfg), t.double())
        l64.backward()
        opt64.step()
        torch.cuda.synchronize()
        assert loss.dim() == 0 and loss.is_cuda
        assert abs(loss.item() - l64.item()) < 1e-5, (it, loss.item(), l64.item())
    hp = dict(G.named_parameters())
    worst = max(rel_err(hp[k], sd[k]) for k in names)
    print('hat two steps: worst parameter rel err %.2e' % worst)
    assert worst < 1e-4


def test_train_mode_drop_path_replays_against_fp64():
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    ref = R.init_(H.GeneratorResNet(upscale=2, window_size=9, depths=(4, 4), num_heads=(6, 6), drop_path_rate=0.5))
    G = hip_model(ref, drop_path_rate=0.5)
    G.train()
    x = O.det_fill('hat.dp.x', (4, 3, 18, 18), 0.5, 0.5)
    r = O.det_fill('hat.dp.r', (4, 3, 36, 36), 1.0)
    torch.manual_seed(3)
    with ops.conv_math('fp32'):
        y = G(dev(x))
        (y * dev(r)).sum().backward()
    factors = {i: tuple(None if f is None else f.cpu() for f in hab.last_drop_factors) for i, hab in enumerate(G.habs)}
    drawn = torch.cat([f for fs in factors.values() for f in fs if f is not None])
    assert (drawn == 0).any() and (drawn > 1).any()                     # both outcomes occur at rate up to 0.5
    assert factors[0] == (None, None)
    sd = R.state(ref, torch.float64)
    y64 = R.forward(sd, x.double(), R.config(2, 9, (4, 4)), factors=factors)
    (y64 * r.double()).sum().backward()
    score, k = grad_score(G, sd)
    print('hat train-mode drop path: output %.2e, gradient score %.2e (%s)' % (rel_err(y, y64), score, k))
    assert rel_err(y, y64) < 1e-4 and score < 5e-3
    # replay: the same factors again give the same output bit for bit
    for i, hab in enumerate(G.habs):
        hab.replay_drop_factors = tuple(None if f is None else f.to(DEV) for f in hab.last_drop_factors)
    with torch.no_grad(), ops.conv_math('fp32'):
        y2 = G(dev(x))
    assert torch.equal(y.detach(), y2)


def test_half_mode_forward():
    from sradsgan_amd import ops
    ref = build('x4')
    G = hip_model(ref)
    x, _ = R.inputs('x4', CASES['x4'][2], 4, 9)
    with torch.no_grad():
        with ops.conv_math('half'):
            y = G(dev(x))
        with ops.conv_math('fp32'):
            y32 = G(dev(x))
    sd = R.state(ref, torch.float64)
    with torch.no_grad():
        y64 = R.forward(sd, x.double(), R.config(4, 9, DEPTHS))
    e, e32 = rel_err(y, y64), rel_err(y, y32)
    print('hat half mode forward: %.2e against fp64, %.2e against fp32' % (e, e32))
    assert torch.isfinite(y).all() and e < 5e-3 and e32 < 5e-3


def test_x9_at_window_9_is_refused_and_at_window_8_trains():
    from sradsgan_amd import ops
    from sradsgan_amd.model import hat as H
    x = dev(O.det_fill('hat.x9.x', (2, 3, 24, 24), 0.5, 0.5))
    t = dev(O.det_fill('hat.x9.t', (2, 3, 216, 216), 0.5, 0.5))
    G9 = H.GeneratorResNet(upscale=9, window_size=9, depths=(2,), num_heads=(6,), img_size=24).to(DEV)
    opt = torch.optim.Adam(G9.parameters(), lr=2e-4, betas=(0.9, 0.99))
    with pytest.raises(ValueError):
        H.train_step(G9, opt, x, t)
    G8 = H.GeneratorResNet(upscale=9, window_size=8, depths=(2,), num_heads=(6,), img_size=24).to(DEV)
    opt = torch.optim.Adam(G8.parameters(), lr=2e-4, betas=(0.9, 0.99))
    w0 = G8.conv_last.weight.detach().clone()
    with ops.conv_math('bf16x3'):
        losses = [H.train_step(G8, opt, x, t).item() for _ in range(2)]
    assert all(np.isfinite(losses)) and not torch.equal(w0, G8.conv_last.weight.detach())
