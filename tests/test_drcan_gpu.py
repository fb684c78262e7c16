"""DRCAN on the HIP path (sradsgan_amd.model.drcan) in split-bf16 and exact-fp32 conv arithmetic: the channel attention with biased
1x1 convs against fp64 torch (bit-identical reruns, NULL biases identical to the bias-free kernels); RCAN against the reference's
vectors (tests/golden/drcan_x*.npz) and its gradients against the fp64 restatement (tests/drcan_ref.py); the trainer's 10 x 20
configuration at the training crop against fp64 on the device; two WGAN-GP iterations through TrainStep against the oracle's step on
fp64 copies of the same networks; DRCAN(args).train() end to end; one forward in 'half' arithmetic."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import drcan_ref as R
from tests.test_drcan_cpu import CASES, build_ref, digest, golden, inputs, rel

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CL = torch.channels_last
MODES = ['bf16x3', 'fp32']


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def dev(t):
    return t.to(DEV).contiguous(memory_format=CL)


def hip_model(scale, reduction=16, groups=2, blocks=2, ref=None):
    from sradsgan_amd.model import drcan as H
    G = H.RCAN(n_resgroups=groups, n_resblocks=blocks, reduction=reduction, scale=scale)
    G.load_state_dict((ref if ref is not None else build_ref(scale, reduction, groups, blocks)).state_dict(), strict=True)
    return G.to(DEV)


def grad_score(hip, ref):
    """worst |dg| over max(|g| of the parameter, 1e-2 |g| of the network) (tests/test_amssrn_gpu.py)"""
    hp, rp = dict(hip.named_parameters()), dict(ref.named_parameters())
    gnet = max(float(p.grad.abs().max()) for p in rp.values())
    worst, wk = 0.0, None
    for k, p in rp.items():
        d = float((hp[k].grad.detach().cpu().double() - p.grad.detach().cpu().double()).abs().max())
        s = d / max(float(p.grad.abs().max()), 1e-2 * gnet)
        if s > worst:
            worst, wk = s, k
    return worst, wk


# ---- channel attention with biases ------------------------------------------------------------------------------------------- #

def ca_ref64(u, x, fc1, b1, fc2, b2):
    leaves = [t.detach().cpu().double().requires_grad_() for t in (u, x, fc1, b1, fc2, b2)]
    u, x, fc1, b1, fc2, b2 = leaves
    m = u.mean(dim=(2, 3), keepdim=True)
    F = torch.nn.functional
    s = torch.sigmoid(F.conv2d(torch.relu(F.conv2d(m, fc1, b1)), fc2, b2))
    return s * u + x, leaves


def ca_operands(tag, n, h, w, hidden):
    u = dev(O.det_fill(tag + '.u', (n, 64, h, w), 1.0, 0.1))
    x = dev(O.det_fill(tag + '.x', (n, 64, h, w), 1.0))
    fc1 = O.det_fill(tag + '.fc1', (hidden, 64, 1, 1), 0.3).to(DEV)
    b1 = O.det_fill(tag + '.b1', (hidden,), 0.2).to(DEV)          # mixed signs: some hidden units clipped by the ReLU
    fc2 = O.det_fill(tag + '.fc2', (64, hidden, 1, 1), 0.3).to(DEV)
    b2 = O.det_fill(tag + '.b2', (64,), 0.5).to(DEV)
    r = dev(O.det_fill(tag + '.r', (n, 64, h, w), 1.0))
    return u, x, fc1, b1, fc2, b2, r


@pytest.mark.parametrize('hidden', [4, 16])
@pytest.mark.parametrize('shape', [(1, 7, 9), (3, 5, 5), (2, 33, 31)])
def test_biased_ca_residual_matches_fp64_and_is_bit_identical(hidden, shape):
    from sradsgan_amd import ops
    u, x, fc1, b1, fc2, b2, r = ca_operands('bca', *shape, hidden)
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_() for t in (u, x, fc1, b1, fc2, b2)]
        out = ops.ca_residual(leaves[0], leaves[1], leaves[2], leaves[4], None, leaves[3], leaves[5])
        (out * r).sum().backward()
        torch.cuda.synchronize()
        runs.append([out.detach().cpu()] + [t.grad.cpu() for t in leaves])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                           # deterministic, bit for bit
    want, leaves64 = ca_ref64(u, x, fc1, b1, fc2, b2)
    (want * r.cpu().double()).sum().backward()
    errs = [rel_err(runs[0][0], want)] + [rel_err(got, leaf.grad) for got, leaf in zip(runs[0][1:], leaves64)]
    print('biased CA hidden %d %s: out %.1e du %.1e dx %.1e dfc1 %.1e db1 %.1e dfc2 %.1e db2 %.1e' % ((hidden, shape) + tuple(errs)))
    assert errs[0] < 1e-6 and max(errs[1:]) < 1e-5


@pytest.mark.parametrize('hidden', [4, 16])
@pytest.mark.parametrize('shape', [(1, 12, 10), (2, 27, 25), (2, 54, 54)])
def test_conv_pool_epilogue_feeds_the_biased_attention(hidden, shape):
    """RCAB's conv2 (64 -> 64, 3x3) leaves the channel sums; the attention from them matches the stand-alone pooling pass's and
    fp64, forward and every gradient."""
    from sradsgan_amd import ops
    n, h, w = shape
    t = dev(O.det_fill('cpb.t', (n, 64, h, w), 1.0))
    wc = O.det_fill('cpb.w', (64, 64, 3, 3), 0.04).to(DEV)
    bc = O.det_fill('cpb.b', (64,), 0.01).to(DEV)
    _, x, fc1, b1, fc2, b2, r = ca_operands('cpb', n, h, w, hidden)
    grads = []
    for use_pool in (True, False):
        leaves = [p.clone().requires_grad_() for p in (fc1, b1, fc2, b2)]
        with ops.conv_math('bf16x3'):
            assert ops.pool_epilogue_ok(t, wc)
            u, pool = ops.conv2d_pool(t, wc, bc)
            assert pool is not None
            u = u.detach().requires_grad_()
            out = ops.ca_residual(u, x, leaves[0], leaves[2], pool if use_pool else None, leaves[1], leaves[3])
            (out * r).sum().backward()
        grads.append((out.detach(), u.grad, [p.grad for p in leaves], u.detach()))
    want, leaves64 = ca_ref64(grads[1][3], x, fc1, b1, fc2, b2)
    (want * r.cpu().double()).sum().backward()
    for out, du, pg, _ in grads:
        assert rel_err(out, want) < 1e-6 and rel_err(du, leaves64[0].grad) < 1e-5
        for got, leaf in zip(pg, (leaves64[2], leaves64[3], leaves64[4], leaves64[5])):
            assert rel_err(got, leaf.grad) < 1e-5


@pytest.mark.parametrize('hidden', [4, 16])
def test_null_biases_are_the_bias_free_kernels_bit_for_bit(hidden):
    from sradsgan_amd import _hip, ops
    lib, p, st = _hip.lib(), ops._p, ops._stream
    n, h, w = 3, 11, 13
    u, x, fc1, _, fc2, _, g = ca_operands('nb', n, h, w, hidden)
    f32 = dict(device=DEV, dtype=torch.float32)
    nseg = lib.srhip_ca_segments()
    psum = torch.empty(n * nseg * 64, **f32)
    _hip.check(lib.srhip_ca_pool_sum(p(u), p(psum), n, h * w, 64, st()), 'pool')
    fwd = []
    for biased in (False, True):
        avg, s, hid = torch.empty(n, 64, **f32), torch.empty(n, 64, **f32), torch.empty(n, hidden, **f32)
        if biased:
            rc = lib.srhip_ca_mlp_fwd_bias(p(psum), nseg, p(fc1), None, p(fc2), None, p(avg), p(hid), p(s), n, h * w, 64, hidden, st())
        else:
            rc = lib.srhip_ca_mlp_fwd(p(psum), nseg, p(fc1), p(fc2), p(avg), p(hid), p(s), n, h * w, 64, hidden, st())
        _hip.check(rc, 'mlp_fwd')
        fwd.append((avg, hid, s))
    for a, b in zip(*fwd):
        assert torch.equal(a, b)
    avg, hid, s = fwd[0]
    part = torch.empty(n * nseg * 64, **f32)
    _hip.check(lib.srhip_ca_bwd_partial(p(g), p(u), p(part), n, h * w, 64, st()), 'partial')
    bwd = []
    for biased in (False, True):
        dmean, dfc1, dfc2 = torch.empty(n, 64, **f32), torch.empty(hidden, 64, **f32), torch.empty(64, hidden, **f32)
        ws = torch.empty(lib.srhip_ca_mlp_bwd_workspace(n, hidden) // 4, **f32)
        if biased:
            rc = lib.srhip_ca_mlp_bwd_bias(p(part), p(avg), p(hid), p(s), p(fc1), p(fc2), p(dmean), p(dfc1), None, p(dfc2), None,
                                           p(ws), ws.numel() * 4, n, h * w, 64, hidden, st())
        else:
            rc = lib.srhip_ca_mlp_bwd(p(part), p(avg), p(hid), p(s), p(fc1), p(fc2), p(dmean), p(dfc1), p(dfc2), p(ws), ws.numel() * 4,
                                      n, h * w, 64, hidden, st())
        _hip.check(rc, 'mlp_bwd')
        bwd.append((dmean, dfc1, dfc2))
    torch.cuda.synchronize()
    for a, b in zip(*bwd):
        assert torch.equal(a, b)
    # and one bias present, the other absent: the present one acts, the gradient of the absent one is not asked for
    _, _, fc1, b1, fc2, b2, r = ca_operands('nb1', n, h, w, hidden)
    leaves = [t.clone().requires_grad_() for t in (u, fc1, fc2, b2)]
    out = ops.ca_residual(leaves[0], x, leaves[1], leaves[2], None, None, leaves[3])
    (out * r).sum().backward()
    want, l64 = ca_ref64(u, x, fc1, torch.zeros_like(b1), fc2, b2)
    (want * r.cpu().double()).sum().backward()
    assert rel_err(out, want) < 1e-6 and rel_err(leaves[3].grad, l64[5].grad) < 1e-5 and rel_err(leaves[1].grad, l64[2].grad) < 1e-5


# ---- the generator --------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scale,reduction', CASES)
def test_generator_matches_reference_vectors_and_fp64_gradients(mode, scale, reduction):
    from sradsgan_amd import ops
    g = golden(scale, reduction)
    ref = build_ref(scale, reduction)
    G = hip_model(scale, reduction, ref=ref)
    x, t = inputs(scale)
    with ops.conv_math(mode):
        y = G(dev(x))
        l1 = ops.l1_mean(y, dev(t))
        mse = ops.mse_mean(y, dev(t))
        l1.backward()
    torch.cuda.synchronize()
    e_y = rel(O.digest(y, full_max=4096, nsample=4096), g['y'])
    print('drcan x%d r%d %s: output %.2e l1 %.2e mse %.2e' % (scale, reduction, mode, e_y, abs(l1.item() - float(g['l1'])),
                                                              abs(mse.item() - float(g['mse']))))
    assert e_y < 1e-4
    assert abs(l1.item() - float(g['l1'])) < 1e-5 and abs(mse.item() - float(g['mse'])) < 1e-5
    r64 = ref.double()
    R.loss(r64(x.double()), t.double()).backward()
    score, k = grad_score(G, r64)
    print('drcan x%d r%d %s: worst gradient score %.2e (%s)' % (scale, reduction, mode, score, k))
    assert score < 2e-3
    assert rel(np.concatenate([digest(p.grad) for _, p in G.named_parameters()]), g['grads']) < 2e-2


@pytest.mark.parametrize('mode', MODES)
def test_training_configuration_at_tile_size_matches_fp64_on_device(mode):
    """The trainer's RCAN (10 groups x 20 RCABs, reduction 16), x4, 54 -> 216, B = 2: output and every parameter gradient of one
    backward against the fp64 restatement on the same device."""
    from sradsgan_amd import ops
    ref = build_ref(4, 16, 10, 20)
    G = hip_model(4, 16, 10, 20, ref=ref)
    x = O.det_fill('drcan.big.x', (2, 3, 54, 54), 0.5, 0.5)
    r = O.det_fill('drcan.big.r', (2, 3, 216, 216), 1.0)
    with ops.conv_math(mode):
        y = G(dev(x))
        (y * dev(r)).sum().backward()
    torch.cuda.synchronize()
    r64 = ref.double().to(DEV)
    y64 = r64(x.double().to(DEV))
    (y64 * r.double().to(DEV)).sum().backward()
    e = rel_err(y, y64)
    refg = dict(r64.named_parameters())
    rows = []
    gnet = max(float(p.grad.abs().max()) for p in refg.values())
    for k, p in G.named_parameters():
        d = float((p.grad.detach().double() - refg[k].grad).abs().max())
        rows.append((d / max(float(refg[k].grad.abs().max()), 1e-2 * gnet), d / float(refg[k].grad.abs().max().clamp_min(1e-30)), k))
    rows.sort(reverse=True)
    print('drcan 10x20 %s: output %.2e; worst gradient scores %s' % (mode, e, ', '.join('%s %.1e (own %.1e)' % (k, s, o)
                                                                                      for s, o, k in rows[:5])))
    assert e < 1e-4
    # tail, body conv and the last group's conv lie downstream of every ReLU: their gradients carry the forward's roundoff only.
    # Upstream of a ReLU whose input is within roundoff of 0 the branch can differ from fp64's, and 200 blocks of split-bf16 /
    # fp32 data gradients accumulate: there the gradients are held to the network's scale (the score of tests/test_amssrn_gpu.py)
    for s, own, k in rows:
        if k.startswith(('tail.', 'body.10.', 'body.9.body.20.')):
            assert own < 1e-4, (k, own)
    assert rows[0][0] < (1e-2 if mode == 'bf16x3' else 5e-3), rows[0]


def test_half_mode_forward():
    from sradsgan_amd import ops
    ref = build_ref(4)
    G = hip_model(4, ref=ref)
    x = O.det_fill('drcanH.x', (2, 3, 54, 54), 0.5, 0.5)
    with torch.no_grad():
        with ops.conv_math('half'):
            y = G(dev(x))
        with ops.conv_math('fp32'):
            y32 = G(dev(x))
        y64 = ref.double()(x.double())
    e, e32 = rel_err(y, y64), rel_err(y, y32)
    print('drcan half mode forward: %.2e against fp64, %.2e against fp32' % (e, e32))
    assert torch.isfinite(y).all() and e < 5e-3 and e32 < 5e-3


# ---- the WGAN-GP step ------------------------------------------------------------------------------------------------------ #

def _gan_nets():
    from sradsgan_amd.model import FeatureExtractor
    from sradsgan_amd.model.base_networks import Discriminator
    og, od, of = build_ref(4, 16, 2, 2), O.Discriminator(attention=False), O.FeatureExtractor()
    O.det_init_(od, prefix='D.'), O.det_init_(of, prefix='F.')
    hg = hip_model(4, 16, 2, 2, ref=og)
    hd, hf = Discriminator(norm_type='batch', use_spectralnorm=False, attention=False), FeatureExtractor()
    hd.load_state_dict(od.state_dict(), strict=True)
    hf.load_state_dict(of.state_dict(), strict=True)
    return (hg, hd.to(DEV), hf.to(DEV)), (og, od, of)


def _batch(it):
    lr = O.det_fill('drcan.gan.lr.%d' % it, (2, 3, 12, 12), 0.5, 0.5)
    hr = O.det_fill('drcan.gan.hr.%d' % it, (2, 3, 48, 48), 0.5, 0.5)
    alpha = O.det_fill('drcan.gan.alpha.%d' % it, (2, 1, 1, 1), 0.5, 0.5)
    return lr, hr, alpha


SCALARS = ('loss_G', 'loss_D', 'pixel', 'content', 'loss_gan', 'gp')


def _hip_steps(nets, its, on_step=None, sink=None):
    """TrainStep over the batches `its`; the scalars of each iteration go to `sink` (a list) before on_step(it) runs."""
    from sradsgan_amd.train_step import TrainStep
    step = TrainStep(*nets)
    outs = sink if sink is not None else []
    for it in its:
        lr, hr, alpha = _batch(it)
        got = step(lr.to(DEV), hr.to(DEV), alpha.to(DEV))
        torch.cuda.synchronize()
        outs.append({k: float(got[k]) for k in SCALARS})
        if on_step is not None:
            on_step(it)
    return [] if sink is not None else outs


def test_two_gan_iterations_match_the_oracle_step_in_fp64_and_rerun_bit_identically():
    """G = RCAN (2 x 2, reduction 16, x4), D = base_networks' Discriminator(norm_type='batch', attention=False), VGG features[:12];
    B = 2, 12 x 12 -> 48 x 48.  The oracle (oracle/sradsgan_ref.train_step) runs fp64 copies of the same networks: the restatement
    RCAN, the oracle's Discriminator(attention=False) and FeatureExtractor."""
    from tests.parity_util import grad_score as net_grad_score
    (hg, hd, hf), (og, od, of) = _gan_nets()
    g64, d64, f64 = (copy.deepcopy(m).double() for m in (og, od, of))
    oG = torch.optim.Adam(g64.parameters(), lr=2e-4, betas=(0.9, 0.999))
    oD = torch.optim.Adam(d64.parameters(), lr=2e-4, betas=(0.9, 0.999))

    def check(it):
        lr, hr, alpha = _batch(it)
        want = O.train_step(g64, d64, f64, oG, oD, lr.double(), hr.double(), alpha.double())
        diffs = {k: abs(outs[it][k] - want[k]) for k in SCALARS}
        print('drcan GAN it %d: %s' % (it, ' '.join('%s %.2e' % kv for kv in diffs.items())))
        assert max(diffs.values()) < 1e-3
        if it == 0:
            # gradients of the first iteration (identical weights on both sides): bars of tests/parity_util.train_parity vs fp64
            sg, kg = net_grad_score((hg,), (g64,), verbose=True)
            sd, kd = net_grad_score((hd,), (d64,), verbose=True)
            print('drcan GAN it 0 gradients: G %.2e (%s), D %.2e (%s)' % (sg, kg, sd, kd))
            assert sg < 5e-3 and sd < 2e-2

    outs = []
    _hip_steps((hg, hd, hf), range(2), on_step=check, sink=outs)
    lr_ = 2e-4
    for net, ref in ((hg, g64), (hd, d64)):
        for (k, a), (_, b) in zip(net.state_dict().items(), ref.state_dict().items()):
            a, b = a.detach().cpu().double(), b.detach().cpu().double()
            d = float((a - b).abs().max())
            if 'running_' in k:
                assert d <= 5e-3 * max(1.0, float(b.abs().max())), (k, d)
            elif 'num_batches' not in k:
                assert d <= 2 * lr_ * 2 * 1.01 + 1e-7, (k, d)        # Adam moves an element by about lr per step on either side
    (hg2, hd2, hf2), _ = _gan_nets()
    outs2 = _hip_steps((hg2, hd2, hf2), range(2))
    assert outs2 == outs
    for a, b in ((hg, hg2), (hd, hd2)):
        for (k, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(p, q), k


def test_drcan_trainer_end_to_end(tmp_path):
    from sradsgan_amd.model import drcan as H
    g = torch.Generator().manual_seed(33)
    train = [torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    hr = torch.rand(2, 3, 32, 32, generator=g)
    test = [(torch.nn.functional.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]
    args = H.default_args(num_epochs=1, batch_size=2, test_batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32,
                          hr_width=32, sample_interval=1, n_resgroups=2, n_resblocks=1)
    net = H.DRCAN(args, train_loader=train, test_loader=test)
    hist = net.train()
    assert isinstance(net.generator, H.RCAN) and len(net.generator.res_groups) == 2
    assert type(net.discriminator).__name__ == 'Discriminator' and net.discriminator.norm_type == 'batch'
    assert len(hist) == 1 and all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
    files = sorted(os.listdir(os.path.join(str(tmp_path), 'model')))
    assert files == ['discriminator_param.pkl', 'discriminator_param_epoch_1.pkl', 'generator_param.pkl', 'generator_param_epoch_1.pkl']
    psnr, ssim, ergas, lpips = net.mfeNew_validate(epoch=1, modelpath=os.path.join(str(tmp_path), 'model', 'generator_param_epoch_1.pkl'))
    assert abs(psnr - hist[-1]['psnr']) < 1e-9 and lpips != lpips
    assert 'drcan_psnr:' in open(os.path.join(str(tmp_path), 'val_log.txt')).read().splitlines()[-1]
    # resume: epoch != 0 loads the epoch files strictly, the generator through RCAN.load_state_dict
    net2 = H.DRCAN(H.default_args(**dict(vars(args), epoch=1, num_epochs=1)), train_loader=train, test_loader=test)
    net2._build()
    for (k, a), (_, b) in zip(net.generator.state_dict().items(), net2.generator.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k
