"""CPU checks of the GDP diffusion sampler (sradsgan_amd/model/gdp.py): the fp64 restatement (tests/gdp_ref.py) against vectors
recorded from the reference (tools/make_golden_gdp.py), the schedule buffers bit for bit, the full configuration's state-dict keys,
shapes and parameter count without allocating it, and the refusals.

Measured when the goldens were generated: the fp64 restatement lies 8.4e-7 (small net, worst of the five timestep cases) and 1.5e-6
(six-step loop, whole continous stack) from the reference's float32 vectors, relative to the largest value.  The bars below are ten
times those.  The restatement's own float32 run lies 8.4e-7 from its float64 run on the small net (the fp32 floor)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import gdp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
SMALL_BAR = 10 * 8.447e-07
LOOP_BAR = 10 * 1.508e-06


def config():
    return json.loads(re.sub(r'//.*', '', open(os.path.join(GOLD, 'gdp_test_54_216.json')).read()))


def small_net():
    from sradsgan_amd.model import gdp
    return R.init_(gdp.UNet(**R.SMALL))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope='module')
def sd64():
    return R.state(small_net(), torch.float64)


def test_restatement_reproduces_the_reference_unet(sd64):
    g = np.load(os.path.join(GOLD, 'gdp_small.npz'))
    x = R.small_input().double()
    worst = 0.0
    for name, ts in R.SMALL_T.items():
        y = R.unet_forward(sd64, x, torch.tensor(ts), R.SMALL)
        assert tuple(y.shape) == tuple(g['shape'])
        worst = max(worst, rel(O.digest(y), g[name]))
    print('gdp small net: fp64 restatement vs reference %.3e (bar %.3e)' % (worst, SMALL_BAR))
    assert worst <= SMALL_BAR
    assert float(np.abs(g['t0']).max()) > 1e-2                   # the filler leaves no zeroed conv: the output is live


def test_restatement_reproduces_the_reference_sampling_loop(sd64):
    g = np.load(os.path.join(GOLD, 'gdp_loop.npz'))
    cond = R.small_input()[:, 3:].double()
    sdg = {'denoise_fn.' + k: v for k, v in sd64.items()}
    o = R.LOOP_SCHEDULE
    kept = R.sample(sdg, cond, torch.from_numpy(g['noise']), R.betas64(o['schedule'], o['n_timestep'], o['linear_start'], o['linear_end']),
                    R.SMALL, keep=True)
    stack = torch.cat(kept, dim=0)
    assert tuple(stack.shape) == tuple(g['stack'].shape) == (14, 3, 12, 12) and tuple(g['noise'].shape) == (7, 2, 3, 12, 12)
    e = rel(stack, g['stack'])
    print('gdp six-step loop: fp64 restatement vs reference %.3e (bar %.3e)' % (e, LOOP_BAR))
    assert e <= LOOP_BAR
    assert rel(stack[-1], g['final']) <= LOOP_BAR               # continous=False: the stack's last entry, ONE image


@pytest.mark.parametrize('tag,opt', [('linear1000', dict(schedule='linear', n_timestep=1000, linear_start=1e-4, linear_end=2e-2)),
                                     ('cosine50', dict(schedule='cosine', n_timestep=50, linear_start=1e-4, linear_end=2e-2))])
def test_schedule_buffers_are_bit_equal(tag, opt):
    from sradsgan_amd.model import gdp
    g = np.load(os.path.join(GOLD, 'gdp_schedule.npz'))
    D = gdp.GaussianDiffusion(None, image_size=12)
    D.set_new_noise_schedule(opt, 'cpu')
    names = sorted(k.split('.', 1)[1] for k in g.files if k.startswith(tag + '.'))
    assert names == sorted(gdp.SCHEDULE_BUFFERS) == sorted(D.state_dict())
    for k in names:
        got = D.state_dict()[k].numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), g['%s.%s' % (tag, k)].view(np.uint32)), k
    assert D.num_timesteps == opt['n_timestep']
    for name in ('quad', 'warmup10', 'warmup50', 'const', 'jsd'):
        assert np.array_equal(gdp.make_beta_schedule(name, 20), R.betas64(name, 20))


def test_full_configuration_keys_shapes_and_strict_load():
    from sradsgan_amd.model import gdp
    g = np.load(os.path.join(GOLD, 'gdp_full.npz'))
    with torch.device('meta'):                                   # 271 M parameters: never materialised
        G = gdp.define_G(config())
    sd = G.state_dict()
    assert sorted(sd) == ['denoise_fn.' + k for k in g['keys']]
    for k, s in zip(g['keys'], g['shapes']):
        t = sd['denoise_fn.' + k]
        assert tuple(t.shape) == tuple(int(v) for v in s[:t.dim()]) and not any(s[t.dim():]), k
    assert sum(p.numel() for p in G.parameters()) == int(g['params']) == 271417731
    assert all(p.device.type == 'meta' for p in G.parameters())
    # a reference-keyed state dict (with the schedule buffers a checkpoint saved after set_new_noise_schedule carries) loads strictly
    state = {k: torch.empty(v.shape, device='meta') for k, v in sd.items()}
    for k in gdp.SCHEDULE_BUFFERS:
        state[k] = torch.empty(1000, device='meta')
    gdp.load_gen(G, state)
    assert sorted(G.state_dict()) == sorted(state)
    with pytest.raises(RuntimeError):
        gdp.load_gen(G, {k: v for k, v in state.items() if 'qkv' not in k})


def test_load_gen_round_trips_values_on_the_small_net():
    from sradsgan_amd.model import gdp
    a = gdp.GaussianDiffusion(small_net(), image_size=12)
    a.set_new_noise_schedule(R.LOOP_SCHEDULE, 'cpu')
    b = gdp.GaussianDiffusion(gdp.UNet(**R.SMALL), image_size=12)
    gdp.load_gen(b, a.state_dict())
    assert b.num_timesteps == 6
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


@pytest.mark.parametrize('kw', [dict(dims=3), dict(num_classes=10), dict(use_fp16=True), dict(use_scale_shift_norm=False),
                                dict(resblock_updown=False), dict(use_new_attention_order=True), dict(num_head_channels=16),
                                dict(num_head_channels=-1, num_heads=1)])
def test_unsupported_constructor_values_are_refused_by_name(kw):
    from sradsgan_amd.model import gdp
    with torch.device('meta'), pytest.raises(NotImplementedError, match=sorted(kw)[0]):
        gdp.UNet(216, **kw)


def test_accepted_constructor_values_build():
    from sradsgan_amd.model import gdp
    with torch.device('meta'):
        gdp.UNet(216, use_checkpoint=True, dropout=0.2, inner_channel=64, norm_groups=16, attn_res=[16], with_time_emb=False)
        gdp.UNet(216, model_channels=64, num_head_channels=-1, num_heads=2, channel_mults=(1, 2), attention_resolutions=(2,))


def test_training_entry_points_raise():
    from sradsgan_amd.model import gdp
    G = gdp.GaussianDiffusion(None, image_size=12)
    for call in (lambda: G({'HR': None}), lambda: G.p_losses({}), lambda: G.set_loss('cpu')):
        with pytest.raises(NotImplementedError, match='training is not built: this is the sampler'):
            call()
    with pytest.raises(NotImplementedError, match='ddpm'):
        opt = config()
        opt['model']['which_model_G'] = 'ddpm'
        gdp.define_G(opt)


def test_cpu_tensors_are_refused():
    from sradsgan_amd.model import gdp
    net = small_net()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(R.SMALL_SHAPE), torch.zeros(2, dtype=torch.long))
    G = gdp.GaussianDiffusion(net, image_size=12)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        G.super_resolution(torch.zeros(2, 3, 12, 12))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gdp.gdp_super_resolve(G, torch.zeros(2, 6, 6, 3, dtype=torch.uint8), 12)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gdp.group_norm_act(torch.zeros(1, 4, 32), torch.ones(32), torch.zeros(32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gdp.qkv_attention(torch.zeros(1, 4, 96), 1)


def test_seed_choice_keeps_the_restatement_clear_of_rounding_ties(sd64):
    """tests/test_gdp_gpu.py compares gdp_super_resolve's bytes with the restatement's and may leave out values within 1e-3 of a
    half-integer before rounding, up to 1 % of them.  With gdp_ref.SR_SEED the fp64 restatement alone (on the restated Philox draws)
    stays under that cap."""
    sdg = {'denoise_fn.' + k: v for k, v in sd64.items()}
    o = R.LOOP_SCHEDULE
    betas = R.betas64(o['schedule'], o['n_timestep'], o['linear_start'], o['linear_end'])
    noise = R.philox_noise(R.SR_SEED, o['n_timestep'], 2, 3, 12, 12)
    assert abs(float(noise.mean())) < 0.1 and abs(float(noise.var()) - 1) < 0.1
    v = R.super_resolve_values(sdg, R.sr_input(), 12, noise, betas, R.SMALL)
    near = np.abs(v - np.floor(v) - 0.5) < 1e-3
    print('gdp super-resolve: %.2f %% of the restatement within 1e-3 of a tie, value range %.1f .. %.1f' % (100 * near.mean(), v.min(), v.max()))
    assert near.mean() < 0.01
    assert v.max() - v.min() > 64                                # a live image, not a clamped constant
