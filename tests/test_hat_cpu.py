"""HAT (sradsgan_amd.model.hat) without a GPU: state_dict keys, parameter names and counts against the reference's fixtures
(tests/golden/hat_*.npz, tools/make_golden_hat.py), strict loading of a reference-shaped state_dict, every refusal, the index and
mask builders against the reference's values (negative OCA indices included), and the fp32 restatement (tests/hat_ref.py) against
the fixtures' digests."""
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from tests import hat_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTHS = (2, 2)
# name -> (scale, window, input shape), as tools/make_golden_hat.py
CASES = {
    'x2': (2, 9, (2, 3, 18, 27)),
    'x3': (3, 9, (2, 3, 18, 27)),
    'x4': (4, 9, (2, 3, 18, 27)),
    'x8': (8, 9, (2, 3, 18, 27)),
    'x3w8': (3, 8, (2, 3, 16, 24)),
    'x9w8': (9, 8, (2, 3, 16, 24)),
    'x4pad': (4, 9, (1, 3, 13, 14)),
}


def golden(name):
    return np.load(os.path.join(HERE, 'golden', 'hat_%s.npz' % name))


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def build(name, **kw):
    from sradsgan_amd.model import hat as H
    scale, ws, _ = CASES[name]
    return R.init_(H.GeneratorResNet(upscale=scale, window_size=ws, depths=DEPTHS, num_heads=(6,) * len(DEPTHS), **kw))


def unique_names(G):
    seen, out = set(), []
    for k, p in G.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append(k)
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_keys_names_and_parameter_counts_match_the_reference(name):
    from sradsgan_amd.model import hat as H
    g = golden(name)
    G = build(name)
    assert sorted(G.state_dict().keys()) == list(g['keys'])
    assert unique_names(G) == list(g['names'])
    scale, ws, _ = CASES[name]
    full = H.GeneratorResNet(upscale=scale, window_size=ws)
    assert sorted(full.state_dict().keys()) == list(g['full_keys'])
    assert sum(p.numel() for p in full.parameters()) == int(g['full_params'])


def test_full_x4_generator_has_the_reference_parameter_count():
    from sradsgan_amd.model import hat as H
    assert sum(p.numel() for p in H.GeneratorResNet(upscale=4).parameters()) == 7584299


@pytest.mark.parametrize('name', ['x4', 'x3w8'])
def test_index_and_mask_builders_match_the_reference(name):
    g = golden(name)
    G = build(name)
    scale, ws, shape = CASES[name]
    assert np.array_equal(G.relative_position_index_SA.numpy(), g['rpi_sa'])
    assert np.array_equal(G.relative_position_index_OCA.numpy(), g['rpi_oca'])
    assert np.array_equal(R.rpi_sa(ws).numpy(), g['rpi_sa']) and np.array_equal(R.rpi_oca(ws).numpy(), g['rpi_oca'])
    hp, wp = shape[2] + (-shape[2]) % ws, shape[3] + (-shape[3]) % ws
    assert np.array_equal(G.calculate_mask((hp, wp)).numpy().astype(np.int8), g['mask'])
    assert np.array_equal(R.shift_mask(hp, wp, ws, ws // 2).numpy().astype(np.int8), g['mask'])
    oca = g['rpi_oca']
    table = (2 * ws - 1 + ws // 2) ** 2
    if ws == 9:
        assert (oca.min(), oca.max(), table, int((oca < 0).sum())) == (-242, 198, 441, 7938)
    else:
        assert (oca.min(), oca.max(), table) == (-200, 160, 361)
    assert len(np.unique(np.mod(oca, table))) == table                # every table row is hit once wrapped


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_the_reference_vectors(name):
    g = golden(name)
    scale, ws, shape = CASES[name]
    G = build(name)
    sd = R.state(G, torch.float32)
    x, t = R.inputs(name, shape, scale, ws)
    y = R.forward(sd, x, R.config(scale, ws, DEPTHS))
    assert tuple(y.shape) == tuple(g['y_shape'])
    l1 = torch.nn.functional.l1_loss(y, t)
    assert rel(O.digest(y, full_max=4096, nsample=4096), g['y']) < 1e-5
    assert abs(l1.item() - float(g['l1'])) < 1e-6
    assert abs(torch.nn.functional.mse_loss(y, t).item() - float(g['mse'])) < 1e-6
    l1.backward()
    assert rel(np.concatenate([digest(sd[k].grad) for k in unique_names(G)]), g['grads']) < 1e-4


def test_reference_shaped_state_dict_loads_strictly():
    G = build('x4')
    sd = {k: v.clone() for k, v in G.state_dict().items()}
    from sradsgan_amd.model import hat as H
    H2 = H.GeneratorResNet(upscale=4, window_size=9, depths=DEPTHS, num_heads=(6, 6))
    H2.load_state_dict(sd, strict=True)
    for k, v in H2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert tuple(sd['layers.0.residual_group.blocks.0.attn.qkv.weight'].shape) == (288, 96)
    assert tuple(sd['layers.0.residual_group.overlap_attn.relative_position_bias_table'].shape) == (441, 6)


def test_drop_path_rates_and_shift_semantics():
    from sradsgan_amd.model import hat as H
    G = H.GeneratorResNet(upscale=8, img_size=27)
    habs = G.habs
    assert len(habs) == 36
    assert isinstance(habs[0].drop_path, torch.nn.Identity)
    rates = [h.drop_path.drop_prob for h in habs[1:]]
    assert np.allclose(rates, torch.linspace(0, 0.1, 36)[1:].tolist())
    assert [h.shift_size for h in habs[:4]] == [0, 4, 0, 4]
    small = H.GeneratorResNet(upscale=8, img_size=9, depths=(2,), num_heads=(6,))
    assert [h.shift_size for h in small.habs] == [0, 0] and small.habs[1].window_size == 9
    assert len(G.res_groups) == 6


@pytest.mark.parametrize('kw', [dict(ape=True), dict(drop_rate=0.1), dict(attn_drop_rate=0.1), dict(upsampler='pixelshuffledirect'),
                                dict(resi_connection='identity'), dict(use_checkpoint=True), dict(in_chans=1), dict(embed_dim=180),
                                dict(num_heads=(4, 4)), dict(window_size=7), dict(window_size=16), dict(qk_scale=0.5)])
def test_unsupported_options_raise(kw):
    from sradsgan_amd.model import hat as H
    args = dict(upscale=4, depths=DEPTHS, num_heads=(6, 6))
    args.update(kw)
    with pytest.raises(NotImplementedError):
        H.GeneratorResNet(**args)


def test_cpu_tensors_are_refused():
    from sradsgan_amd.model import hat as H
    G = H.GeneratorResNet(upscale=2, depths=(2,), num_heads=(6,))
    with pytest.raises(Exception):
        G(torch.zeros(1, 3, 18, 18))
