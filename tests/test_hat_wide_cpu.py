"""HAT at its published widths (sradsgan_amd.model.hat with embed_dim 144 / 180, window 16) without a GPU: state_dict keys, parameter
names and counts against the reference's fixtures (tests/golden/hat180_*.npz, hat144_x2.npz; tools/make_golden_hat_wide.py), strict
loading of a reference-shaped state_dict of the full HAT x4, the two pinned refusals and the published triples, the index and mask
builders at window 16 (the OCA index reaches -880), the fp64-capable restatement (tests/hat_ref.py, configured by
tests/hat_wide_ref.py) against the fixtures' digests at tests/test_hat_cpu.py's own bars, and every refusal of the new entry points
with made-up addresses."""
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import hat_ref as R
from tests import hat_wide_ref as W
from tests.test_hat_cpu import digest, rel, unique_names

HERE = os.path.dirname(os.path.abspath(__file__))
PUBLISHED = {
    'HAT': dict(embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, window_size=16, compress_ratio=3, squeeze_factor=30, mlp_ratio=2.),
    'HAT-L': dict(embed_dim=180, depths=(6,) * 12, num_heads=(6,) * 12, window_size=16, compress_ratio=3, squeeze_factor=30, mlp_ratio=2.),
    'HAT-S': dict(embed_dim=144, depths=(6,) * 6, num_heads=(6,) * 6, window_size=16, compress_ratio=24, squeeze_factor=24, mlp_ratio=2.),
}


def golden(name):
    return np.load(os.path.join(HERE, 'golden', '%s.npz' % name))


def build(name, device=None):
    from sradsgan_amd.model import hat as H
    G = H.GeneratorResNet(depths=W.DEPTHS, num_heads=(6,) * len(W.DEPTHS), **W.model_kwargs(name))
    return R.init_(G if device is None else G.to(device))


@pytest.mark.parametrize('name', sorted(W.CASES))
def test_keys_names_and_parameter_counts_match_the_reference(name):
    from sradsgan_amd.model import hat as H
    g = golden(name)
    G = build(name)
    assert sorted(G.state_dict().keys()) == list(g['keys'])
    assert unique_names(G) == list(g['names'])
    with torch.device('meta'):
        full = H.GeneratorResNet(depths=(6,) * 6, num_heads=(6,) * 6, **W.model_kwargs(name))
    assert sorted(full.state_dict().keys()) == list(g['full_keys'])
    assert sum(p.numel() for p in full.parameters()) == int(g['full_params'])


def test_full_hat_x4_has_the_published_parameter_count():
    assert int(golden('hat180_x4')['full_params']) == 20624795


@pytest.mark.parametrize('name', ['hat180_x4', 'hat180_x4pad', 'hat144_x2'])
def test_index_and_mask_builders_match_the_reference_at_window_16(name):
    g = golden(name)
    G = build(name)
    shape = W.CASES[name][2]
    ws = W.WS
    assert np.array_equal(G.relative_position_index_SA.numpy(), g['rpi_sa'])
    assert np.array_equal(G.relative_position_index_OCA.numpy(), g['rpi_oca'])
    assert np.array_equal(R.rpi_sa(ws).numpy(), g['rpi_sa']) and np.array_equal(R.rpi_oca(ws).numpy(), g['rpi_oca'])
    hp, wp = shape[2] + (-shape[2]) % ws, shape[3] + (-shape[3]) % ws
    assert np.array_equal(G.calculate_mask((hp, wp)).numpy().astype(np.int8), g['mask'])
    assert np.array_equal(R.shift_mask(hp, wp, ws, ws // 2).numpy().astype(np.int8), g['mask'])
    oca = g['rpi_oca']
    assert (g['rpi_sa'].min(), g['rpi_sa'].max(), oca.shape) == (0, 960, (256, 576))
    assert (oca.min(), oca.max()) == (-880, 640)
    assert len(np.unique(np.mod(oca.astype(np.int64), 1521))) == 1521                # every table row is hit once wrapped


@pytest.mark.parametrize('name', sorted(W.CASES))
def test_restatement_reproduces_the_reference_vectors(name):
    """Bars of tests/test_hat_cpu.py::test_restatement_reproduces_the_reference_vectors: output digest 1e-5, losses 1e-6, gradient
    digests 1e-4 (the restatement runs in fp32 like the reference)."""
    g = golden(name)
    _, scale, shape, _ = W.CASES[name]
    G = build(name)
    sd = R.state(G, torch.float32)
    x, t = R.inputs(name, shape, scale, W.WS)
    y = R.forward(sd, x, W.config(name))
    assert tuple(y.shape) == tuple(g['y_shape'])
    l1 = torch.nn.functional.l1_loss(y, t)
    assert rel(O.digest(y, full_max=4096, nsample=4096), g['y']) < 1e-5
    assert abs(l1.item() - float(g['l1'])) < 1e-6
    assert abs(torch.nn.functional.mse_loss(y, t).item() - float(g['mse'])) < 1e-6
    l1.backward()
    assert rel(np.concatenate([digest(sd[k].grad) for k in unique_names(G)]), g['grads']) < 1e-4


def test_reference_shaped_state_dict_of_the_full_hat_x4_loads_strictly():
    """Keys are the reference's recorded full_keys; shapes are worked out from the published configuration by hand below, not read
    from the class under test."""
    from sradsgan_amd.model import hat as H
    g = golden('hat180_x4')
    with torch.device('meta'):
        G = H.GeneratorResNet(upscale=4, **PUBLISHED['HAT'])
    own = G.state_dict()
    assert sorted(own.keys()) == list(g['full_keys'])
    expect = {'layers.0.residual_group.blocks.0.attn.qkv.weight': (540, 180),
              'layers.0.residual_group.blocks.0.attn.relative_position_bias_table': (961, 6),
              'layers.5.residual_group.overlap_attn.relative_position_bias_table': (1521, 6),
              'layers.0.residual_group.blocks.0.conv_block.cab.0.weight': (60, 180, 3, 3),
              'layers.0.residual_group.blocks.0.conv_block.cab.3.attention.1.weight': (6, 180, 1, 1),
              'layers.0.residual_group.blocks.0.mlp.fc1.weight': (360, 180),
              'relative_position_index_SA': (256, 256), 'relative_position_index_OCA': (256, 576),
              'conv_first.weight': (180, 3, 3, 3), 'conv_before_upsample.0.weight': (64, 180, 3, 3)}
    for k, shp in expect.items():
        assert tuple(own[k].shape) == shp, k
    sd = {k: torch.empty(v.shape, dtype=v.dtype, device='meta') for k, v in own.items()}
    G.load_state_dict(sd, strict=True, assign=True)
    # a real (CPU) load of the two-group network keeps every value
    small = build('hat180_x4')
    sd = {k: v.clone() for k, v in small.state_dict().items()}
    H2 = H.GeneratorResNet(depths=W.DEPTHS, num_heads=(6, 6), **W.model_kwargs('hat180_x4'))
    H2.load_state_dict(sd, strict=True)
    for k, v in H2.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize('name', sorted(PUBLISHED))
@pytest.mark.parametrize('upscale', [2, 3, 4, 8, 9])
def test_published_configurations_construct(name, upscale):
    from sradsgan_amd.model import hat as H
    with torch.device('meta'):
        G = H.GeneratorResNet(upscale=upscale, **PUBLISHED[name])
    assert len(G.habs) == 6 * len(PUBLISHED[name]['depths'])
    assert [h.shift_size for h in G.habs[:4]] == [0, 8, 0, 8]
    assert G.habs[0].attn.relative_position_bias_table.shape == (961, 6)


def test_mlp_ratio_4_and_other_depths_construct():
    from sradsgan_amd.model import hat as H
    with torch.device('meta'):
        G = H.GeneratorResNet(upscale=4, embed_dim=180, depths=(1, 3), num_heads=(6, 6), window_size=16, mlp_ratio=4.)
    assert G.habs[0].mlp.fc1.weight.shape == (720, 180)


@pytest.mark.parametrize('kw', [dict(embed_dim=180), dict(window_size=16), dict(embed_dim=144), dict(embed_dim=180, window_size=8),
                                dict(embed_dim=96, window_size=16), dict(embed_dim=120, window_size=16),
                                dict(embed_dim=180, window_size=16, num_heads=(4, 4)), dict(embed_dim=180, window_size=16, num_heads=(5, 5)),
                                dict(embed_dim=180, window_size=16, overlap_ratio=0.25), dict(embed_dim=180, window_size=16, ape=True),
                                dict(embed_dim=180, window_size=16, qk_scale=0.25), dict(embed_dim=180, window_size=16, squeeze_factor=5),
                                dict(embed_dim=180, window_size=16, resi_connection='identity')])
def test_everything_between_and_beside_the_two_families_stays_refused(kw):
    """The first two are the refusals tests/test_hat_cpu.py pins (embed_dim 180 at window 9, window 16 at embed_dim 96)."""
    from sradsgan_amd.model import hat as H
    args = dict(upscale=4, depths=W.DEPTHS, num_heads=(6, 6))
    args.update(kw)
    with pytest.raises(NotImplementedError) as e:
        H.GeneratorResNet(**args)
    if set(kw) <= {'embed_dim', 'window_size', 'num_heads'}:
        assert '96' in str(e.value) and '144 / 180' in str(e.value)           # the message names the two families


def test_refusals_of_the_new_entry_points_need_no_device():
    """Every call of hat_wide_ref.refusals with made-up addresses returns its error code with a message: the checks run on the host
    before anything is launched."""
    from sradsgan_amd import _hip
    lib = _hip.lib()
    p = {k: 0x10000000 + 0x1000000 * i for i, k in enumerate('abcdefghijkl')}
    p['ws'] = 0x40000000
    p['ws_bytes'] = 4 << 21
    calls = W.refusals(lib, p)
    assert len(calls) > 100
    bad = []
    for label, code, call in calls:
        rc = call()
        if rc != code or not lib.srhip_last_error():
            bad.append((label, rc))
    assert not bad, bad


def test_workspace_of_the_attention_backward_holds_no_pair_array():
    """At the timing configuration (16 images of 64 x 64, C = 180): the table partials by row, delta, and OCA's slabs -- against the
    2 x 64 x 6 x 256 x 576 x 4 B = 453 MB that two per-(query, key) arrays per block would take."""
    from sradsgan_amd import _hip
    lib = _hip.lib()
    tokens, nwin = 16 * 64 * 64, 256
    up = lambda b: (b + 255) // 256 * 256
    sa = lib.srhip_hatw_attn_bwd_workspace(0, 16, 64, 64, 180, 6, 16)
    oca = lib.srhip_hatw_attn_bwd_workspace(1, 16, 64, 64, 180, 6, 16)
    assert sa == up(6 * 64 * 961 * 4) + up(tokens * 6 * 4)
    assert oca == up(6 * 64 * 1521 * 4) + up(tokens * 6 * 4) + nwin * 576 * 360 * 4
    for bad in ((0, 16, 64, 64, 180, 6, 8), (2, 16, 64, 64, 180, 6, 16), (0, 0, 64, 64, 180, 6, 16), (0, 16, 60, 64, 180, 6, 16),
                (0, 16, 64, 64, 180, 7, 16)):
        assert lib.srhip_hatw_attn_bwd_workspace(*bad) == 0
