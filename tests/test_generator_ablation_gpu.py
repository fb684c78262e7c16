"""The generator's attention ablations (rla_mode / bla_mode / ga_mode / pool_mode / addconv, reference sradsgan.py:101-151, 215-324,
365-439) on the HIP path against the CPU oracle and the reference's record tests/golden/gen_ablation.npz: RAB, ResGroup and GAB_UP
per variant with every gradient, the seven recorded generators (forward, one training iteration, a no_grad forward bit-equal to the
grad-mode one, the fused route of csrc/attn_variants.hip against the composition, a captured evaluation graph, a reference-format state dict), the stand-alone
single-pool CLAM / SLAM with a double backward, and the trainer's switches.  Bars: rel_err < 1e-3 (test_model_gpu.TOL), generator
gradient grad_score < 5e-3 (test_model_gpu.py's training bar)."""
import argparse

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import attn_variants_ref as V
from tests.parity_util import ZERO_GRAD_KEYS, grad_score, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
TOL = 1e-3
KINK_MARGIN = 1e-6          # |LeakyReLU input| of the oracle's RAB conv1 that the chosen input keeps (split-bf16 products carry ~5e-6 relative)


def _conditioned_input(tag, ora_rabs):
    """An input whose LeakyReLU inputs (the oracle's RAB conv1 outputs, CPU) stay KINK_MARGIN away from the kink: a pre-activation
    within rounding of zero takes either slope in two correct fp32 implementations.  Judged on the oracle alone."""
    for suffix in ('', 'a', 'b', 'c', 'd', 'e', 'f', 'g'):
        x = O.det_fill('%s.x%s' % (tag, suffix), (3, 64, 10, 12), 1.0)
        with torch.no_grad():
            closest = min(float(r.conv1(x).abs().min()) for r in ora_rabs)
        if closest >= KINK_MARGIN:
            return x
    raise AssertionError('no well-conditioned input among the candidates for ' + tag)


def _against_oracle(tag, hip_mod, ora_mod, x, math):
    from sradsgan_amd import ops
    O.det_init_(ora_mod, prefix=tag + '.')
    hip_mod.load_state_dict(ora_mod.state_dict(), strict=True)
    hip_mod.to(DEV)
    xo, xh = x.clone().requires_grad_(True), x.clone().to(DEV).requires_grad_(True)
    yo = ora_mod(xo)
    dy = O.det_fill(tag + '.dy', tuple(yo.shape), 1.0)
    yo.backward(dy)
    with ops.conv_math(math):
        yh = hip_mod(xh)
        yh.backward(dy.to(DEV))
        with torch.no_grad():
            y_eval = hip_mod(xh)
    worst = [('y', rel_err(yh, yo)), ('y no_grad', rel_err(y_eval, yo)), ('dx', rel_err(xh.grad, xo.grad))]
    op = dict(ora_mod.named_parameters())
    for k, p in hip_mod.named_parameters():
        assert p.grad is not None, k
        if k.endswith(ZERO_GRAD_KEYS):           # identically zero in exact arithmetic (SGAM's key bias): the yardstick is the sibling weight's gradient
            worst.append((k, float(p.grad.abs().max()) / float(op[k.replace('bias', 'weight')].grad.abs().max())))
            continue
        worst.append((k, rel_err(p.grad, op[k].grad)))
    worst.sort(key=lambda r: -r[1])
    print('%s [%s]: worst %s %.3e' % (tag, math, worst[0][0], worst[0][1]))
    assert worst[0][1] < TOL, worst[:4]


@pytest.mark.parametrize('math', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('variant', V.VARIANTS, ids=V.variant_id)
def test_rab_and_resgroup_per_variant(variant, math):
    from sradsgan_amd import model as M
    mode, pool, addconv = variant
    kw = dict(la_mode=mode, pool_mode=pool, addconv=addconv)
    tag = 'abl_rab_' + V.variant_id(variant)
    ora = O.RAB(64, 64, **kw)
    O.det_init_(ora, prefix=tag + '.')
    _against_oracle(tag, M.RAB(64, 64, **kw), ora, _conditioned_input(tag, [ora]), math)
    gkw = dict(n_blocks=1, rla_mode=mode, bla_mode=mode, pool_mode=pool, addconv=addconv)
    tag = 'abl_grp_' + V.variant_id(variant)
    ora = O.ResGroup(O.RAB, **gkw)
    O.det_init_(ora, prefix=tag + '.')
    _against_oracle(tag, M.ResGroup(M.RAB, **gkw), ora, _conditioned_input(tag, list(ora.RG)), math)


@pytest.mark.parametrize('scale', [2, 3])
@pytest.mark.parametrize('addconv', [True, False])
@pytest.mark.parametrize('ga_mode', ['', 'CA', 'SA', 'CA-SA', 'SA-CA', 'CA|SA'], ids=lambda m: m.replace('|', '+') or 'none')
def test_gab_up_per_mode(ga_mode, addconv, scale):
    from sradsgan_amd import model as M
    tag = 'abl_gab_%s_%s_x%d' % (ga_mode.replace('|', 'p'), addconv, scale)
    x = O.det_fill('x64', (2, 64, 10, 12), 1.0)[:1, :, :6, :7] * 0.3
    _against_oracle(tag, M.GAB_UP(ga_mode, addconv, scale), O.GAB_UP(ga_mode, addconv, scale), x.contiguous(), 'bf16x3')


def _pair(cfg):
    """(HIP generator on the device, oracle generator) of a recorded configuration with the recorded weights."""
    from sradsgan_amd import model as M
    og = O.GeneratorResNet(O.ResGroup, **V.gen_kwargs(cfg))
    O.det_init_(og, prefix=V.gen_tag(cfg) + '.')
    hg = M.GeneratorResNet(M.ResGroup, **V.gen_kwargs(cfg))
    hg.load_state_dict(og.state_dict(), strict=True)
    return hg.to(DEV), og


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_generator_forward_and_gradients_against_oracle_and_reference_record(cfg, golden):
    hg, og = _pair(cfg)
    g, tag = golden('gen_ablation'), V.gen_tag(cfg)
    x = O.det_fill('abl.x', V.GEN_SHAPE, 0.5, 0.5)
    yo = og(x)
    dy = O.det_fill(tag + '.dy', tuple(yo.shape), 1.0)
    yo.backward(dy)
    yh = hg(x.to(DEV))
    yh.backward(dy.to(DEV))
    assert rel_err(yh, yo) < TOL
    want = g[tag + '/y']
    assert float(np.abs(O.digest(yh) - want).max()) <= TOL * float(np.abs(want).max())
    with torch.no_grad():                                    # the same forward kernels with nothing saved: the same bits
        y_eval = hg(x.to(DEV))
    assert torch.equal(y_eval, yh)
    score, worst = grad_score((hg,), (og,))
    print('%s: grad score %.3e (%s)' % (tag, score, worst))
    assert score < 5e-3, (score, worst)


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_fused_route_against_the_composition_route(cfg, monkeypatch):
    """The variant node of csrc/attn_variants.hip against the composition of srhip_cbam_* primitives (the route predicate forced
    off): output, input gradient and every parameter gradient within TOL of each other."""
    from sradsgan_amd import ops
    tag = V.gen_tag(cfg)
    x = O.det_fill('abl.x', V.GEN_SHAPE, 0.5, 0.5).to(DEV)
    res = []
    for fused in (True, False):
        if not fused:
            monkeypatch.setattr(ops, 'attention_variant_supported', lambda *a: False)
        hg, _ = _pair(cfg)
        xx = x.clone().requires_grad_(True)
        y = hg(xx)
        y.backward(O.det_fill(tag + '.dy', tuple(y.shape), 1.0).to(DEV))
        res.append(dict(y=y.detach(), dx=xx.grad, **{k: p.grad for k, p in hg.named_parameters()}))
    worst = sorted(((rel_err(res[0][k], res[1][k]), k) for k in res[0] if not k.endswith(ZERO_GRAD_KEYS)), reverse=True)
    print('%s: fused vs composed, worst %s %.3e' % (tag, worst[0][1], worst[0][0]))
    assert worst[0][0] < TOL, worst[:4]


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_fused_and_composition_routes_pick_the_same_indices(cfg, monkeypatch):
    """Per tail of one forward: the arg-max indices of srhip_attn_var_fwd (ops.attention_variant_gates) are torch.equal to those the
    composition's pooling primitives (srhip_cbam_pool_hw / _pool_c, what _PoolHW / _PoolC save) find in the tensor each gate pools
    there -- u, CLAM(u) for the spatial gate of CA-SA, SLAM(u) for the channel gate of SA-CA -- and the pooled statistics agree
    within TOL.  A tail that broke ties differently on the two routes would show here."""
    from sradsgan_amd import _hip, ops
    from sradsgan_amd.model import sradsgan as MS
    hg, _ = _pair(cfg)
    seen, orig = [], MS._AttentionTail._tail

    def spy(self, out, skip, emit_pp=False):
        seen.append((self, out.detach()))
        return orig(self, out, skip, emit_pp)
    monkeypatch.setattr(MS._AttentionTail, '_tail', spy)
    with torch.no_grad():
        hg(O.det_fill('abl.x', V.GEN_SHAPE, 0.5, 0.5).to(DEV))
        monkeypatch.setattr(MS._AttentionTail, '_tail', orig)
        lib, stream = _hip.lib(), torch.cuda.current_stream().cuda_stream
        assert len(seen) == V.GEN_GROUPS * (V.GEN_BLOCKS + 1)
        compared = 0
        for tail, u in seen:
            mode = tail.la_mode
            if mode not in ops.TAIL_ORDERS:
                continue
            u = ops.nhwc(u)
            n, c, h, w = u.shape
            ca, sa = getattr(tail, 'ca', None), getattr(tail, 'sa', None)
            pool = (ca if ca is not None else sa).pool_mode
            assert ops.attention_variant_supported(u, mode, ca.fc1.weight if ca is not None else None, sa.conv1.weight if sa is not None else None)
            _, _, f = ops.attention_variant_gates(u, mode, pool, ca.fc1.weight if ca is not None else None,
                                                  ca.fc2.weight if ca is not None else None, sa.conv1.weight if sa is not None else None)
            if ca is not None:
                a = ops.nhwc(sa(u)) if mode == 'SA-CA' else u                    # the composition's own gated activation
                t = torch.full((n, 2, c), float('nan'), device=DEV)
                arg = torch.full((n, c), -7, device=DEV, dtype=torch.int32)
                _hip.check(lib.srhip_cbam_pool_hw(a.data_ptr(), t.data_ptr(), arg.data_ptr(), 0, n, h * w, c, stream), 'cbam_pool_hw')
                if 'Avg' in pool:
                    assert rel_err(f['avg'], t[:, 0]) < TOL
                if 'Max' in pool:
                    assert torch.equal(f['arg'], arg), (mode, pool, (f['arg'] != arg).nonzero()[:4].tolist())
                    assert rel_err(f['mx'], t[:, 1]) < TOL
                    compared += 1
            if sa is not None:
                a = ops.nhwc(ca(u)) if mode == 'CA-SA' else u
                t = torch.full((n * h * w, 2), float('nan'), device=DEV)
                argc = torch.full((n * h * w,), -7, device=DEV, dtype=torch.int32)
                _hip.check(lib.srhip_cbam_pool_c(a.data_ptr(), t.data_ptr(), argc.data_ptr(), 0, n, h * w, c, stream), 'cbam_pool_c')
                rows = [i for i, name in enumerate(('Avg', 'Max')) if name in pool.split('|')]
                assert rel_err(f['pooled'], t[:, rows]) < TOL
                if 'Max' in pool:
                    assert torch.equal(f['argc'], argc), (mode, pool, (f['argc'] != argc).nonzero()[:4].tolist())
                    compared += 1
        torch.cuda.synchronize()
    print('%s: %d index tensors compared' % (V.gen_tag(cfg), compared))
    assert compared > 0 or 'Max' not in cfg[3] or not any(cfg[:2])


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_generator_train_step_against_oracle(cfg):
    """One TrainStep iteration against oracle.train_step: the six logged scalars within TOL (of the largest scalar), G's gradients
    under the 5e-3 bar."""
    from sradsgan_amd import model as M
    from sradsgan_amd.train_step import TrainStep
    hg, og = _pair(cfg)
    od, of = O.Discriminator(), O.FeatureExtractor()
    O.det_init_(od, prefix='D.'), O.det_init_(of, prefix='F.')
    hd, hf = M.Discriminator(), M.FeatureExtractor()
    hd.load_state_dict(od.state_dict(), strict=True)
    hf.load_state_dict(of.state_dict(), strict=True)
    step = TrainStep(hg, hd.to(DEV), hf.to(DEV))
    tag, (b, _, side, _), s = V.gen_tag(cfg), V.GEN_SHAPE, V.GEN_SCALE
    lr_img = O.det_fill(tag + '.lr', (b, 3, side, side), 0.5, 0.5)
    hr_img = O.det_fill(tag + '.hr', (b, 3, side * s, side * s), 0.5, 0.5)
    alpha = O.det_fill(tag + '.alpha', (b, 1, 1, 1), 0.5, 0.5)
    want = O.train_step(og, od, of, torch.optim.Adam(og.parameters(), lr=2e-4, betas=(0.9, 0.999)),
                        torch.optim.Adam(od.parameters(), lr=2e-4, betas=(0.9, 0.999)), lr_img, hr_img, alpha)
    got = step(lr_img.to(DEV), hr_img.to(DEV), alpha.to(DEV))
    names = ['loss_G', 'loss_D', 'pixel', 'content', 'loss_gan', 'gp']
    gv, wv = np.array([float(got[k]) for k in names]), np.array([want[k] for k in names])
    print('%s: scalars %s vs %s' % (tag, gv, wv))
    assert float(np.abs(gv - wv).max()) <= TOL * max(float(np.abs(wv).max()), 1.0)
    score, worst = grad_score((hg,), (og,), verbose=True)
    assert score < 5e-3, (score, worst)


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_graphed_evaluator_replays_equal_eager(cfg):
    from sradsgan_amd import validate
    hg, _ = _pair(cfg)
    hg.eval()
    ev = validate.GraphedEvaluator(hg, V.GEN_SCALE)
    gen = torch.Generator().manual_seed(5)
    for it in range(2):
        lr = torch.rand(2, 3, 12, 12, generator=gen).to(DEV)
        hr = torch.rand(2, 3, 24, 24, generator=gen).to(DEV)
        want = validate.evaluate(hg, lr, hr, V.GEN_SCALE)
        torch.cuda.synchronize()
        got = ev(lr, hr)
        torch.cuda.synchronize()
        assert torch.equal(got['recon'], want['recon']), it


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_reference_format_state_dict_loads_strictly(cfg, golden):
    """Keys and shapes as the reference recorded them (a single-pool SLAM's conv1 is [1, 1, 7, 7])."""
    from sradsgan_amd import model as M
    g, tag = golden('gen_ablation'), V.gen_tag(cfg)
    sd = {k: torch.zeros([int(x) for x in s.split(',') if x]) for k, s in zip(g[tag + '/keys'].tolist(), g[tag + '/shapes'].tolist())}
    hg = M.GeneratorResNet(M.ResGroup, **V.gen_kwargs(cfg))
    hg.load_state_dict(sd, strict=True)
    if cfg[3] != 'Avg|Max' and any('sa.conv1.weight' in k for k in sd):
        assert all(tuple(v.shape) == (1, 1, 7, 7) for k, v in sd.items() if k.endswith('sa.conv1.weight'))


@pytest.mark.parametrize('which,pool', [('clam', 'Avg'), ('clam', 'Max'), ('slam', 'Avg'), ('slam', 'Max')])
def test_single_pool_clam_and_slam_with_a_double_backward(which, pool):
    """The stand-alone modules through the composition of srhip_cbam_* primitives: forward, first-order gradients, and a double
    backward (the gradient of |dx|^2, as a gradient penalty asks) against the oracle."""
    from sradsgan_amd import model as M
    tag = 'abl_%s_%s' % (which, pool)
    hip, ora = (M.CLAM(64, pool_mode=pool), O.CLAM(64, pool_mode=pool)) if which == 'clam' else (M.SLAM(7, pool), O.SLAM(7, pool))
    O.det_init_(ora, prefix=tag + '.')
    hip.load_state_dict(ora.state_dict(), strict=True)
    hip.to(DEV)
    x = O.det_fill('x64', (2, 64, 10, 12), 1.0)
    dy = O.det_fill(tag + '.dy', (2, 64, 10, 12), 1.0)
    res = []
    for mod, dev in ((ora, 'cpu'), (hip, DEV)):
        xx = x.clone().to(dev).requires_grad_(True)
        y = mod(xx)
        (dx,) = torch.autograd.grad(y, xx, dy.to(dev), create_graph=True)
        pen = (dx ** 2).sum()
        pen.backward()
        res.append(dict(y=y.detach(), dx=dx.detach(), ddx=xx.grad.detach(), **{k: p.grad.detach() for k, p in mod.named_parameters()}))
        mod.zero_grad()
    for k in res[0]:
        e = rel_err(res[1][k], res[0][k])
        print('%s %s: %.3e' % (tag, k, e))
        assert e < TOL, k


def test_trainer_builds_the_requested_variant(tmp_path):
    from sradsgan_amd import model as M, trainer as T
    gen = torch.Generator().manual_seed(21)
    train = [torch.randint(0, 256, (2, 32, 32, 3), generator=gen, dtype=torch.uint8)]                        # uint8 HR tiles
    hr = torch.rand(2, 3, 32, 32, generator=gen)
    test = [(torch.nn.functional.avg_pool2d(hr, 4), hr, hr.clamp(0, 1), ['a', 'b'])]
    args = T.default_args(scale_factor=4, num_epochs=1, batch_size=2, save_dir=str(tmp_path), crop_size=32, hr_height=32, hr_width=32,
                          sample_interval=1, n_residual_blocks=2, n_basic_blocks=1, rla_mode='SA-CA', bla_mode='CA|SA', ga_mode='SA',
                          pool_mode='Max', addconv=False)
    net = T.SRADSGAN(args, train_loader=train, test_loader=test)
    hist = net.train()                                       # one epoch: the training composition and the validation's inference route
    assert len(hist) == 1 and all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
    g = net.generator
    want = M.GeneratorResNet(M.ResGroup, n_residual_blocks=2, n_basic_blocks=1, rla_mode='SA-CA', bla_mode='CA|SA', ga_mode='SA', pool_mode='Max',
                             addconv=False, upscale_factor=4)
    assert [(k, tuple(v.shape)) for k, v in g.state_dict().items()] == [(k, tuple(v.shape)) for k, v in want.state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in net._new_generator().state_dict().items()] == [(k, tuple(v.shape)) for k, v in want.state_dict().items()]
    grp = g.res_groups[0]
    assert grp.la_mode == 'SA-CA' and grp.RG[0].la_mode == 'CA|SA' and g.GAB_UP.ga_mode == 'SA' and grp.sa.pool_mode == 'Max'
    assert not grp.addconv and not hasattr(grp, 'conv') and tuple(grp.sa.conv1.weight.shape) == (1, 1, 7, 7)
    assert T.attention_ablation(argparse.Namespace())['rla_mode'] == 'CA-SA'
