"""LPIPS, host side: the fp64 restatement (tests/lpips_ref.py) against the golden recorded from the reference's PerceptualLoss
(tools/make_golden_lpips.py), the two state-dict forms of sradsgan_amd.lpips.LPIPS, and the no-CPU-fallback rule.  No GPU call."""
import os

import numpy as np
import pytest
import torch

from tests import lpips_ref as R

REL = 5e-6            # restatement vs the reference's fp32 run: measured 7.2e-7, the margin covers BLAS summation order


@pytest.fixture(scope='module')
def G():
    return np.load(R.GOLDEN)


@pytest.fixture(scope='module')
def sd():
    return R.alexnet_state_dict()


def test_generated_backbone_is_the_one_the_golden_was_recorded_with(G, sd):
    assert sum(v.numel() for v in sd.values()) == 2469696
    assert np.array_equal(R.weights_checksum(sd), G['backbone_checksum'])
    assert [G['lin%d' % k].shape[0] for k in range(5)] == list(R.CHANNELS) and all(G['lin%d' % k].min() >= 0 for k in range(5))


@pytest.mark.parametrize('case', ['s0', 's1', 's2', 'big'])
def test_restatement_matches_the_reference(G, sd, case):
    sr, hr = R.big_inputs() if case == 'big' else (torch.from_numpy(G[case + '_sr']), torch.from_numpy(G[case + '_hr']))
    lin = [G['lin%d' % k] for k in range(5)]
    total, taps = R.lpips(sr, hr, sd, lin, per_tap=True)
    want, want_taps = torch.from_numpy(G[case + '_lpips']), torch.from_numpy(G[case + '_taps'])
    rel = float(((total - want).abs() / want.abs()).max())
    # the reference sums the layers in place into res[0] (networks_basic.py:85-87), so row 0 of its per-layer list is the total
    assert torch.equal(want_taps[0], want)
    rel_taps = float(((taps[1:] - want_taps[1:]).abs() / want_taps[1:].abs()).max())
    print('%s: restatement vs reference %.2e relative (taps %.2e)' % (case, rel, rel_taps))
    assert tuple(want.shape) == (sr.shape[0],) and float(want.min()) > 1e-3            # a live metric, not zeros
    assert rel <= REL and rel_taps <= REL


def test_both_state_dict_forms_load_and_unknown_shapes_are_rejected(G, sd):
    from sradsgan_amd.lpips import LPIPS
    m = LPIPS()
    assert not any(p.requires_grad for p in m.parameters())
    init = {k: v.clone() for k, v in m.state_dict().items()}
    assert all(torch.equal(v, LPIPS().state_dict()[k]) for k, v in init.items())        # deterministic init
    tv = dict(sd)
    tv.update({'classifier.1.weight': torch.zeros(4096, 9216), 'features.0.num_batches_tracked': torch.zeros(())})   # ignored keys
    m.load_torchvision_alexnet(tv)
    lin = R.lin_state_dict(G)
    m.load_lin(lin)
    own = m.state_dict()
    assert sorted(own) == sorted(list(sd) + list(lin))
    for k, v in list(sd.items()) + list(lin.items()):
        assert torch.equal(own[k], v), k
    bad = dict(sd)
    bad['features.3.weight'] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match='features.3.weight'):
        m.load_torchvision_alexnet(bad)
    bad_lin = dict(lin)
    bad_lin['lin2.model.1.weight'] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match='lin2'):
        m.load_lin(bad_lin)
    assert torch.equal(m.state_dict()['features.3.weight'], sd['features.3.weight'])     # a rejected load changes nothing
    with pytest.raises(KeyError):
        m.load_torchvision_alexnet({k: v for k, v in sd.items() if k != 'features.10.bias'})


def test_cpu_tensors_are_refused():
    from sradsgan_amd.lpips import LPIPS
    m = LPIPS()
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(x, x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.pairs(x, [(0, 0)])


def test_library_exports_the_lpips_entry_points():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    assert lib.srhip_abi_version() >= 14 and lib.srhip_lpips_blocks() > 0
    for name in ('srhip_lpips_stem', 'srhip_maxpool3x3s2_fwd', 'srhip_lpips_head', 'srhip_lpips_finish'):
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    assert lib.srhip_maxpool3x3s2_fwd(None, None, 1, 2, 2, 64, None) == -1                      # argument errors come back as codes
    x = torch.zeros(1)
    p = x.data_ptr()                                                                          # host memory: never dereferenced on error
    assert lib.srhip_maxpool3x3s2_fwd(p, p, 1, 2, 5, 64, None) == -1 and b'H, W >= 3' in lib.srhip_last_error()
    assert lib.srhip_maxpool3x3s2_fwd(p, p, 1, 5, 5, 6, None) == -1
    assert lib.srhip_lpips_stem(p, p, p, p, 1, 6, 31, 1, None) == -1
    assert lib.srhip_lpips_head(p, p, p, p, 2, 1, 3, 3, 30, None) == -1
