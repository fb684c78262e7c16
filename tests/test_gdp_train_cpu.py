"""CPU checks of the GDP diffusion training path (sradsgan_amd/model/gdp_train.py): the fp64 restatement of p_losses and its gradients
(tests/gdp_train_ref.py) against vectors recorded from the reference (tools/make_golden_gdp_train.py), the trainable U-Net's
state-dict keys for the full configuration, the refusals, and the symbols of the backward kernels.

Measured when the fixture was generated: the fp64 restatement's loss / numel lies 4.0e-8 from the reference's float32 value (0.7378)
and its gradients score 2.17e-6 against the reference's (worst tensor input_blocks.2.0.in_layers.0.weight; tests/test_hat_gpu.py's
score, on the stored digests).  The bars below are ten times those.  The restatement's own float32 run scores 1.7e-6 against its
float64 run."""
import os

import numpy as np
import pytest
import torch

from tests import gdp_ref as R
from tests import gdp_train_ref as T
from tests.test_gdp_cpu import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
LOSS_BAR = 10 * 3.998e-08
GRAD_BAR = 10 * 2.170e-06


def test_restatement_reproduces_the_reference_loss_and_gradients():
    from sradsgan_amd.model import gdp
    g = np.load(os.path.join(GOLD, 'gdp_train.npz'))
    state = R.state(R.init_(gdp.UNet(**R.SMALL)), torch.float64)
    hr, sr = T.train_inputs()
    t, noise = torch.from_numpy(g['t']), torch.from_numpy(g['noise'])
    assert int(g['numel']) == hr.numel() and tuple(t.shape) == (2,) and int(t[0]) != int(t[1])
    loss, grads = T.loss_and_grads(state, hr, sr, t, noise, torch.float64)
    d = abs(loss - float(g['loss']) / int(g['numel']))
    score, key = T.digest_score(grads, g)
    print('gdp p_losses: fp64 restatement vs reference: loss %.3e (bar %.3e), gradient score %.3e at %s (bar %.3e)'
          % (d, LOSS_BAR, score, key, GRAD_BAR))
    assert len(grads) == 144 and sorted('grad.' + k for k in grads) == sorted(k for k in g.files if k.startswith('grad.'))
    assert d <= LOSS_BAR and score <= GRAD_BAR
    gnet = max(float(v.abs().max()) for v in grads.values())
    assert all(float(v.abs().max()) > 1e-3 * gnet for v in grads.values())       # the filler leaves no dead parameter


def test_trainable_unet_keeps_the_reference_keys_and_requires_grad():
    from sradsgan_amd.model import gdp, gdp_train
    g = np.load(os.path.join(GOLD, 'gdp_full.npz'))
    with torch.device('meta'):
        G = gdp_train.define_G(config())
    assert isinstance(G, gdp_train.TrainableDiffusion) and isinstance(G, gdp.GaussianDiffusion)
    assert isinstance(G.denoise_fn, gdp_train.TrainableUNet) and isinstance(G.denoise_fn, gdp.UNet)
    sd = G.state_dict()
    assert sorted(sd) == ['denoise_fn.' + k for k in g['keys']]
    for k, s in zip(g['keys'], g['shapes']):
        v = sd['denoise_fn.' + k]
        assert tuple(v.shape) == tuple(int(x) for x in s[:v.dim()]), k
    assert sum(p.numel() for p in G.parameters()) == int(g['params'])
    assert all(p.requires_grad and not getattr(p, '_srhip_static', False) for p in G.parameters())
    # the sampler's classes stay frozen
    with torch.device('meta'):
        frozen = gdp.define_G(config())
    assert not any(p.requires_grad for p in frozen.parameters()) and all(getattr(p, '_srhip_static', False) for p in frozen.parameters())


def test_adopt_thaws_a_sampler_net_in_place():
    from sradsgan_amd.model import gdp, gdp_train
    net = gdp.UNet(**R.SMALL)
    for p in net.parameters():
        p._srhip_packed = {0: 'stale'}
    got = gdp_train.TrainableUNet.adopt(net)
    assert got is net and isinstance(net, gdp_train.TrainableUNet)
    assert all(p.requires_grad and not hasattr(p, '_srhip_static') and not hasattr(p, '_srhip_packed') for p in net.parameters())
    with pytest.raises(TypeError):
        gdp_train.TrainableUNet.adopt(torch.nn.Linear(2, 2))


def test_adopt_takes_a_trained_nets_images_out_of_the_repack_registry():
    """A net that has trained has its packed images registered for the per-step re-pack; adopting it again drops the images, so their
    registry entries must go too (they would be re-packed every step for as long as the parameters live) and nobody else's."""
    import weakref
    from sradsgan_amd import ops
    from sradsgan_amd.model import gdp_train
    net = gdp_train.TrainableUNet(**R.SMALL)
    other = torch.nn.Parameter(torch.zeros(4, 4, 3, 3))
    entry = lambda p, mode: [weakref.ref(p), mode, None, 0, 0, None, 0, set()]      # the layout of ops._PackRegistry.entries
    kept = entry(other, 0)
    mine = []
    for p in net.parameters():
        if p.dim() >= 2:
            p._srhip_packed = {0: entry(p, 0), 1: entry(p, 1)}
            mine += list(p._srhip_packed.values())
    saved = (ops._registry.entries, ops._registry.dirty)
    try:
        ops._registry.entries = list(saved[0]) + mine[:5] + [kept] + mine[5:]
        ops._registry.dirty = False
        gdp_train.TrainableUNet.adopt(net)
        left = ops._registry.entries
        assert len(mine) > 40 and not any(any(e is m for m in mine) for e in left)
        assert any(e is kept for e in left) and len(left) == len(saved[0]) + 1 and ops._registry.dirty
    finally:
        ops._registry.entries, ops._registry.dirty = saved


def test_unbuilt_training_options_are_refused_by_name():
    from sradsgan_amd.model import gdp_train
    with torch.device('meta'), pytest.raises(NotImplementedError, match='dropout'):
        gdp_train.TrainableUNet(216, dropout=0.2)
    opt = config()
    opt['model']['unet']['dropout'] = 0.1
    with torch.device('meta'), pytest.raises(NotImplementedError, match='dropout'):
        gdp_train.define_G(opt)
    opt = config()
    opt['model']['finetune_norm'] = True
    with pytest.raises(NotImplementedError, match='finetune_norm'):
        gdp_train.DDPM(opt)
    opt = config()
    opt['model']['which_model_G'] = 'ddpm'
    with pytest.raises(NotImplementedError, match='ddpm'):
        gdp_train.define_G(opt)
    with torch.device('meta'), pytest.raises(NotImplementedError, match='use_fp16'):     # what the sampler refuses stays refused
        gdp_train.TrainableUNet(216, use_fp16=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gdp_train.DDPM(config(), device='cpu')
    G = gdp_train.TrainableDiffusion(None, image_size=12, loss_type='huber')
    with pytest.raises(NotImplementedError, match='huber'):
        G.set_loss('cpu')


def test_cpu_tensors_are_refused():
    from sradsgan_amd.model import gdp_train
    net = R.init_(gdp_train.TrainableUNet(**R.SMALL))
    G = gdp_train.TrainableDiffusion(net, image_size=12)
    G.set_loss('cpu')
    G.set_new_noise_schedule(T.TRAIN_SCHEDULE, 'cpu')
    hr, sr = T.train_inputs()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G({'HR': hr, 'SR': sr})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.q_sample(hr, torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(R.SMALL_SHAPE), torch.zeros(2, dtype=torch.long))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gdp_train.training_batch(torch.zeros(2, 12, 12, 3, dtype=torch.uint8), 3)
    for call in (lambda: gdp_train.group_norm_act(torch.zeros(1, 4, 32), torch.ones(32), torch.zeros(32)),
                 lambda: gdp_train.qkv_attention(torch.zeros(1, 4, 96), 1), lambda: gdp_train.silu(torch.zeros(4)),
                 lambda: gdp_train.avg_pool2x2(torch.zeros(1, 32, 4, 4))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_sampler_classes_still_refuse_to_train():
    from sradsgan_amd.model import gdp
    G = gdp.GaussianDiffusion(None, image_size=12)
    for call in (lambda: G({'HR': None}), lambda: G.p_losses({}), lambda: G.set_loss('cpu')):
        with pytest.raises(NotImplementedError, match='training is not built: this is the sampler'):
            call()
    with pytest.raises(NotImplementedError, match='gdp_train'):
        G.set_loss('cpu')


def test_backward_symbols_are_exported_at_abi_14():
    from sradsgan_amd import _hip
    lib = _hip.lib()
    assert lib.srhip_abi_version() == 14
    for name in ('srhip_diff_gn_stats_offset', 'srhip_diff_gn_bwd_workspace', 'srhip_diff_gn_bwd', 'srhip_diff_silu_bwd',
                 'srhip_diff_avgpool2x2_bwd', 'srhip_diff_attn_fwd_lse', 'srhip_diff_attn_bwd_workspace', 'srhip_diff_attn_bwd',
                 'srhip_diff_q_sample'):
        assert name in _hip.SIGNATURES and getattr(lib, name)
    chunks = (729 + 63) // 64
    assert lib.srhip_diff_gn_stats_offset(2, 729) == 2 * chunks * 32 * 2 * 4
    assert lib.srhip_diff_gn_workspace(2, 729) == lib.srhip_diff_gn_stats_offset(2, 729) + 2 * 32 * 2 * 4     # the statistics come last
    assert lib.srhip_diff_gn_bwd_workspace(2, 729, 96) == (2 * chunks * 96 * 2 + 2 * 96 * 2 + 2 * 32 * 2) * 4
    assert lib.srhip_diff_attn_bwd_workspace(2, 729, 16) == 2 * 16 * 729 * 4
    # argument errors come back as codes before anything is launched
    assert lib.srhip_diff_gn_bwd(None, 0, None, 0, None, None, None, None, None, 0, None, 0, None, None, None, None, 0, None, 0, 2, 4, 48, 0,
                                 None) == -1
    assert lib.srhip_diff_attn_bwd(None, None, None, None, None, None, 0, 1, 1, 1, 64, None) == -1
    assert lib.srhip_diff_avgpool2x2_bwd(None, None, 1, 3, 4, 32, None) == -1
