"""LPIPS on the device (sradsgan_amd/lpips.py, csrc/lpips.hip) against the fp64 restatement of tests/lpips_ref.py and the golden recorded
from the reference: the stem conv, the 3x3 stride-2 max pool and the head kernel on their own, the metric end to end in every conv-math
mode, and its way through validate.evaluate, GraphedEvaluator and the trainer.

Bounds.  Stem: conv_emulation's element bound with the tau of the fp32 conv routes (tests/test_conv_routes_gpu.py: 32 * 2^-24).  Head and
end to end in fp32: the same arithmetic as the restatement run in fp32 on the CPU, in another summation order, so the bar is
max(8 x that run's own distance from fp64, 2e-6 |ref|).  bf16x3: the restatement with convs 2-5 through conv_emulation's split-bf16
contraction lies e away from exact fp64; the kernels must lie within 4 e + 2e-6 |ref|.

Every test prints its figures (error over bar, e and the kernels' distance) before it asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_emulation as E
from tests import lpips_ref as R

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
    """name -> (sr, hr, fp64 restatement [N], its fp32 run's distance from it [N]); computed once, never modified."""
    lin = [G['lin%d' % k] for k in range(5)]
    out = {}
    for name in ('s0', 's1', 's2', 'big'):
        sr, hr = R.big_inputs() if name == 'big' else (torch.from_numpy(G[name + '_sr']), torch.from_numpy(G[name + '_hr']))
        ref = R.lpips(sr, hr, sd, lin)
        dev32 = (R.lpips(sr, hr, sd, lin, dtype=torch.float32).double() - ref).abs()
        out[name] = (sr, hr, ref, dev32)
    return out


def _bar(ref, dev32):
    return torch.maximum(8 * dev32, 2e-6 * ref.abs())


# ---- stem --------------------------------------------------------------------------------------------------------------------------- #
def _stem(x, sd):
    from sradsgan_amd import ops
    w = sd['features.0.weight'].to(DEV)
    return ops.lpips_stem_raw(x.to(DEV), w.permute(2, 3, 1, 0).contiguous(), sd['features.0.bias'].to(DEV)).cpu()


def _stem_ref(x, sd):
    xs = R.scaled(x.double())
    ref, absref = E.conv_fwd(xs, sd['features.0.weight'], 4, 2, 'fp32')
    return E.epilogue(ref, absref, bias=sd['features.0.bias'], slope=0.0)


@pytest.mark.parametrize('hw', [(31, 31), (35, 47), (34, 45), (33, 44)])
def test_stem_conv(sd, hw):
    """all four residues of (H - 7) mod 4, non-square images, tiles cut by the image edge"""
    x = R.hash_image((2, 3) + hw, 40 + hw[0])
    got = _stem(x, sd)
    ref, absref = _stem_ref(x, sd)
    assert tuple(got.shape) == (2, 64, (hw[0] - 7) // 4 + 1, (hw[1] - 7) // 4 + 1)
    ratio = E.assert_conv_close(got, ref, absref, TAU_FP32, what='lpips stem %dx%d' % hw)
    print('stem %dx%d: err / bound %.3f, %.0f %% of outputs positive' % (hw + (ratio, 100.0 * float((ref > 0).double().mean()))))
    assert float((ref > 0).double().mean()) > 0.2                       # the ReLU leaves a live tensor to compare


def test_stem_pads_in_the_scaled_space(sd):
    """a constant 0.5 image is 0 after 2x - 1 and -shift / scale after the scaling layer: the interior is constant per channel and the
    border, whose windows reach the zero padding, differs.  Folding the affine into the weights would make them equal."""
    x = torch.full((1, 3, 79, 79), 0.5)
    got = _stem(x, sd)
    ref, absref = _stem_ref(x, sd)
    E.assert_conv_close(got, ref, absref, TAU_FP32, what='lpips stem, constant image')
    pre = E.conv_fwd(R.scaled(x.double()), sd['features.0.weight'], 4, 2, 'fp32')[0] + sd['features.0.bias'].double().view(1, -1, 1, 1)
    live = ((pre[0, :, 5, 5] > 0.05) & ((pre[0, :, 0, 0] - pre[0, :, 5, 5]).abs() > 0.05)).nonzero().flatten()
    assert len(live) > 4
    assert torch.equal(got[0, :, 5, 5], got[0, :, 9, 12])
    assert bool(((got[0, live, 0, 0] - got[0, live, 5, 5]).abs() > 0.04).all())


# ---- max pool ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('shape', [(2, 8, 11, 64), (1, 53, 53, 64), (2, 26, 26, 192), (1, 3, 3, 64)])
def test_maxpool3x3s2_is_bit_equal_to_aten(shape):
    from sradsgan_amd import ops
    n, h, w, c = shape
    x = (R.hash16(n * c * h * w, 7 + h) * 4).float().reshape(n, c, h, w)
    assert float(x.min()) < -1 and float(x.max()) > 1
    got = ops.max_pool3x3s2_raw(x.to(DEV)).cpu()
    assert torch.equal(got, F.max_pool2d(x, 3, 2))
    with pytest.raises(ValueError):
        ops.max_pool3x3s2_raw(torch.zeros(1, 64, 2, 5, device=DEV))


# ---- head --------------------------------------------------------------------------------------------------------------------------- #
def _head(f, pairs, w):
    from sradsgan_amd import _hip, ops
    pt = torch.tensor(pairs, dtype=torch.int32, device=DEV)
    partial = torch.empty(1, len(pairs), _hip.lib().srhip_lpips_blocks(), device=DEV, dtype=torch.float64)
    ops.lpips_head_raw(f.to(DEV), pt, w.to(DEV), partial[0])
    return ops.lpips_finish_raw(partial, [f.shape[2] * f.shape[3]]).cpu()


@pytest.mark.parametrize('c', [64, 192, 384, 256])
@pytest.mark.parametrize('hw', [(1, 2), (3, 5), (12, 12), (53, 53)])
def test_head(c, hw):
    h, w = hw
    f = F.relu(R.hash16(6 * c * h * w, c + h).float().reshape(6, c, h, w) + 0.1) * 3
    f[0, :, 0, 0] = 0                                          # a pixel that is all zero in both images of pair (0, 1) ...
    f[1, :, 0, 0] = 0
    f[2, :, 0, w - 1] = 0                                      # ... and one that is zero in one image only
    f[5] = f[3]
    lw = (R.hash16(c, 3 * c) + 0.5).float()
    pairs = [(0, 1), (0, 2), (2, 0), (1, 1), (3, 4), (3, 5), (4, 2)]          # shared indices, a self pair, a pair of equal copies
    got = _head(f, pairs, lw)
    again = _head(f, pairs, lw)
    ref = torch.stack([R.head(f[i:i + 1].double(), f[j:j + 1].double(), lw.double())[0] for i, j in pairs])
    ref32 = torch.stack([R.head(f[i:i + 1], f[j:j + 1], lw)[0] for i, j in pairs]).double()
    bar = _bar(ref, (ref32 - ref).abs())
    err = (got - ref).abs()
    print('head C=%d %dx%d: worst err / bar %.3f (err %.2e, CPU fp32 %.2e)' % (c, h, w, float((err / bar.clamp_min(1e-300)).max()),
                                                                                float(err.max()), float((ref32 - ref).abs().max())))
    assert torch.isfinite(got).all() and float(ref[0]) > 0
    assert got[3] == 0.0 and got[5] == 0.0                     # identical inputs: exactly zero
    assert bool((err <= bar).all())
    assert torch.equal(got, again)                              # deterministic reduction
    assert abs(float(got[1] - got[2])) <= float(bar[1])         # (a - b)^2 is symmetric up to the fp32 rounding of the operands


# ---- end to end --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('name', ['s0', 's1', 's2', 'big'])
def test_fp32_end_to_end(model, cases, G, name):
    from sradsgan_amd import ops
    sr, hr, ref, dev32 = cases[name]
    with ops.conv_math('fp32'):
        got = model(sr.to(DEV), hr.to(DEV)).cpu()
        singles = torch.cat([model(sr[i:i + 1].to(DEV), hr[i:i + 1].to(DEV)) for i in range(sr.shape[0])]).cpu()
    bar = _bar(ref, dev32)
    want = torch.from_numpy(G[name + '_lpips'])
    print('%s fp32: |gpu - fp64| %.2e, CPU fp32 restatement %.2e, bar %.2e; vs golden %.2e relative' % (
        name, float((got - ref).abs().max()), float(dev32.max()), float(bar.min()), float(((got - want).abs() / want).max())))
    assert got.dtype == torch.float64 and tuple(got.shape) == (sr.shape[0],)
    assert bool(((got - ref).abs() <= bar).all())
    assert bool(((got - want).abs() <= 5e-6 * want.abs()).all())
    assert bool(((got - singles).abs() <= bar).all())           # the batched pairs form against one call per image


@pytest.mark.parametrize('name', ['s0', 's2', 'big'])
def test_bf16x3_end_to_end_and_half_is_the_same_number(model, cases, G, sd, name):
    from sradsgan_amd import ops
    sr, hr, ref, _ = cases[name]
    lin = [G['lin%d' % k] for k in range(5)]
    emu = lambda x, w, b, s, p: E.conv_fwd(x, w, s, p, arith='bf16x3', with_abs=False)[0] + b.double().view(1, -1, 1, 1)
    e = (R.lpips(sr, hr, sd, lin, conv=emu) - ref).abs()
    with ops.conv_math('bf16x3'):
        got = model(sr.to(DEV), hr.to(DEV)).cpu()
    with ops.conv_math('half'):
        half = model(sr.to(DEV), hr.to(DEV)).cpu()
        assert ops.get_conv_math() == 'half'
    d = (got - ref).abs()
    print('%s bf16x3: emulation e = %.3e (%.2e relative), gpu distance %.3e (%.2e relative)' % (
        name, float(e.max()), float((e / ref).max()), float(d.max()), float((d / ref).max())))
    assert bool((d <= 4 * e + 2e-6 * ref.abs()).all())
    assert torch.equal(half, got)


def test_shapes_and_indices_are_checked(model):
    x = torch.rand(2, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match='at least 31'):
        model(x[:, :, :30], x[:, :, :30])
    with pytest.raises(ValueError, match='index'):
        model.pairs(x, [(0, 2)])
    with pytest.raises(ValueError, match='shape mismatch'):
        model(x, x[:1])


# ---- evaluate and the trainer ------------------------------------------------------------------------------------------------------- #
def _tiny_trainer(tmp_path, **kw):
    from sradsgan_amd import trainer as T
    g = torch.Generator().manual_seed(21)
    hr = torch.rand(2, 3, 32, 32, generator=g)
    hr2 = torch.rand(2, 3, 32, 32, generator=g)
    test = [(F.avg_pool2d(hr, 4), hr, (hr * 0.9 + 0.05).clamp(0, 1), ['a', 'b']), (F.avg_pool2d(hr2, 4), hr2, hr2.clamp(0.1, 0.9), ['c', 'd'])]
    args = T.default_args(scale_factor=4, save_dir=str(tmp_path), crop_size=32, hr_height=32, hr_width=32, n_residual_blocks=1,
                          n_basic_blocks=1, **kw)
    return T, T.SRADSGAN(args, test_loader=test), test


def test_evaluate_adds_lpips_and_replays_from_a_graph(model, tmp_path):
    from sradsgan_amd import validate as V
    T, net, test = _tiny_trainer(tmp_path)
    torch.manual_seed(3)
    gen = net._new_generator()
    gen.apply(T.weights_init_normal)
    gen = gen.to(DEV).eval()
    lr, hr, bc = (t.to(DEV) for t in test[0][:3])
    plain = V.evaluate(gen, lr, hr, 4, bicubic=bc)
    assert 'lpips' not in plain['sr'] and 'lpips' not in plain['bicubic'] and sorted(plain['sr']) == ['ergas', 'mse', 'psnr', 'ssim']
    out = V.evaluate(gen, lr, hr, 4, bicubic=bc, lpips=model)
    for side in ('sr', 'bicubic'):
        for k in ('mse', 'psnr', 'ssim', 'ergas'):
            assert torch.equal(out[side][k], plain[side][k]), (side, k)
        assert out[side]['lpips'].dtype == torch.float64 and tuple(out[side]['lpips'].shape) == (2,)
    # the same images in a batch of another size: the conv kernels may tile differently, so the fp32 summation-order bar applies
    for got, want in ((out['sr']['lpips'], model(out['recon'], hr)), (out['bicubic']['lpips'], model(bc, hr))):
        assert bool(((got - want).abs() <= 2e-6 * want.abs()).all())
    assert float(out['bicubic']['lpips'].min()) > 0
    only_sr = V.evaluate(gen, lr, hr, 4, lpips=model)
    assert 'bicubic' not in only_sr and bool(((only_sr['sr']['lpips'] - out['sr']['lpips']).abs() <= 2e-6 * out['sr']['lpips']).all())
    eager = {s: {k: v.clone() for k, v in out[s].items()} for s in ('sr', 'bicubic')}
    ge = V.GraphedEvaluator(gen, 4, lpips=model)
    for _ in range(2):                                           # capture, then a second replay
        rep = ge(lr, hr, bc)
        for side in ('sr', 'bicubic'):
            for k, v in eager[side].items():
                assert torch.equal(rep[side][k], v), (side, k)


def test_trainer_reports_lpips_when_configured(model, tmp_path, G, sd):
    T, net, test = _tiny_trainer(tmp_path)
    torch.manual_seed(3)
    gen = net._new_generator()
    gen.apply(T.weights_init_normal)
    path = str(tmp_path / 'g.pkl')
    torch.save(gen.state_dict(), path)
    psnr0, _, _, nan = net.mfeNew_validate(epoch=1, modelpath=path)
    assert nan != nan and 'sradsgan_lpips: nan' in open(net.val_log_path).read().splitlines()[-1]
    net.set_lpips(model)
    psnr, ssim, ergas, lp = net.mfeNew_validate(epoch=1, modelpath=path)
    net.generator.eval()
    direct, direct_bc = [], []
    with torch.no_grad():
        for lr, hr, bc, _ in test:
            direct.append(model(net.generator(lr.to(DEV)), hr.to(DEV)))
            direct_bc.append(model(bc.to(DEV), hr.to(DEV)))
    want, want_bc = float(torch.cat(direct).mean()), float(torch.cat(direct_bc).mean())
    # validation runs the backbone over [hr; recon; bicubic] in one batch, the direct calls over two: the fp32 summation-order bar
    assert psnr == psnr0 and lp == lp and 0 < lp < 10 and abs(lp - want) <= 2e-6 * want
    line = open(net.val_log_path).read().splitlines()[-1]
    assert 'sradsgan_lpips: {:.4e} '.format(lp) in line
    logged_bc = float(line.split('bicubic_lpips: ')[1].split()[0])
    assert abs(logged_bc - want_bc) <= 1e-4 * want_bc                 # four decimals in the log line
    val = net.validate(epoch=1, mode='train')
    assert val[3] == lp
    # the two state-dict paths on args configure the same model
    torch.save(sd, str(tmp_path / 'alexnet.pth'))
    torch.save(R.lin_state_dict(G), str(tmp_path / 'alex.pth'))
    _, net2, _ = _tiny_trainer(tmp_path, lpips_alexnet=str(tmp_path / 'alexnet.pth'), lpips_lin=str(tmp_path / 'alex.pth'))
    assert net2.mfeNew_validate(epoch=1, modelpath=path)[3] == lp
    net2.class_loaders = {'one': test[:1], 'two': test[1:]}
    res = net2.mfeNew_validateByClass(1, modelpath=path)
    assert abs(res['Total']['sradsgan_lpips'] - lp) <= 1e-12 * lp and abs(res['Total']['bicubic_lpips'] - want_bc) <= 2e-6 * want_bc
    with pytest.raises(ValueError, match='both'):
        T.SRADSGAN(T.default_args(lpips_lin='x.pth'))
