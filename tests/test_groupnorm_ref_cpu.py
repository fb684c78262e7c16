"""The closed forms of tests/groupnorm_ref.py (forward, first- and second-order backward of the per-sample normalisations of gn.hip)
against fp64 autograd of the reference's own formulation, at the tolerance tests/test_reduction_ref_cpu.py holds the BatchNorm
closed forms to; and the host-side refusals of the gn entry points, which need no device."""
import pytest
import torch

from tests import groupnorm_ref as G
from tests import reduction_ref as R

EPS = 1e-5
SLOPE = 0.2          # a python float: an fp32 0.2 alone costs 1e-8

# (n, p, c, groups, unbiased): cpg 1, 2, 6, 16 under both variance kinds (instance norm is cpg 1, biased)
CASES = [(2, 13, 12, 12, 0), (2, 13, 12, 12, 1), (3, 7, 64, 32, 0), (3, 7, 64, 32, 1), (2, 9, 192, 32, 0), (2, 9, 192, 32, 1),
         (2, 5, 512, 32, 0), (2, 5, 512, 32, 1), (3, 1, 64, 32, 1)]


@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('slope', [SLOPE, None], ids=['lrelu', 'linear'])
@pytest.mark.parametrize('n,p,c,groups,unbiased', CASES, ids=['%dx%dx%d-g%d-u%d' % k for k in CASES])
def test_closed_forms_match_fp64_autograd(n, p, c, groups, unbiased, slope, affine):
    t = G.gn_inputs('normal', n, p, c)
    gamma, beta = (t['gamma'], t['beta']) if affine else (None, None)
    a = G.gn_autograd(t['x'], gamma, beta, t['dy'], t['u'], groups, unbiased, EPS, slope, torch.float64, addend=t['addend'])
    f = G.gn_fwd_ref(t['x'], gamma, beta, groups, unbiased, EPS, slope)
    for k in ('y', 'mean', 'invstd'):
        assert R.err(f[k], a[k]) < 1e-12, k
    assert torch.equal(f['y'] > 0, a['mask'])
    dx, dgamma, dbeta = G.gn_bwd_ref(t['dy'], t['x'], gamma, a['mask'], groups, unbiased, EPS, slope, addend=t['addend'])
    g_dy, g_x, g_gamma = G.gn_bwd2_ref(t['u'], t['dy'], t['x'], gamma, a['mask'], groups, unbiased, EPS, slope)
    for k, v in (('dx', dx), ('g_dy', g_dy), ('g_x', g_x)) + ((('dgamma', dgamma), ('dbeta', dbeta), ('g_gamma', g_gamma)) if affine else ()):
        assert R.err(v, a[k]) < 1e-11, k


def test_instance_kind_is_torch_instance_norm():
    """groups = c, biased, no affine is nn.InstanceNorm2d(C) as the reference builds it (no affine, no running statistics)."""
    t = G.gn_inputs('normal', 2, 30, 8)
    x4 = t['x'].double().permute(0, 2, 1).reshape(2, 8, 5, 6)
    want = torch.nn.InstanceNorm2d(8)(x4).reshape(2, 8, 30).permute(0, 2, 1)
    assert R.err(G.gn_fwd_ref(t['x'], None, None, 8, 0, EPS, None)['y'], want) < 1e-12


def test_case_table_covers_what_the_gpu_test_needs():
    shapes = {c[1:] for c in G.GN_CASES}
    assert shapes == set(G.GN_SHAPES) | set(G.GN_ALL_FAMILIES) and len(G.GN_CASES) == len(set(G.GN_CASES))
    for s in G.GN_ALL_FAMILIES:
        assert {c[0] for c in G.GN_CASES if c[1:] == s} == set(R.BN_FAMILIES)
    assert any(c // g == 6 for _, _, c, g, _ in G.GN_SHAPES)          # a group that straddles a float4


@pytest.fixture(scope='module')
def lib():
    import os
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


def test_gn_entry_points_refuse_on_the_host(lib):
    """Argument checks run before any device call: m = 1, C not a multiple of 4, C not a multiple of the groups, C > 1024, a short
    workspace, half an affine pair."""
    p, big = 4096, 1 << 30
    for n, pp, c, groups, word in ((2, 1, 64, 64, b'two elements'), (2, 8, 6, 2, b'multiple of 4'), (2, 8, 64, 24, b'groups'),
                                   (2, 8, 1028, 4, b'1024')):
        for rc in (lib.srhip_gn_fwd(p, p, p, p, p, p, p, big, n, pp, c, groups, 0, EPS, 0.2, 1, None),
                   lib.srhip_gn_bwd(p, p, p, p, p, p, None, p, p, p, None, None, p, big, n, pp, c, groups, 0, 0.2, 1, None),
                   lib.srhip_gn_bwd_bwd(p, p, p, p, p, p, p, p, p, p, None, p, big, n, pp, c, groups, 0, 0.2, 1, None)):
            assert rc == -1 and word in lib.srhip_last_error(), (n, pp, c, groups, lib.srhip_last_error())
    need = lib.srhip_gn_workspace(2, 65, 64)
    assert need > 0
    assert lib.srhip_gn_fwd(p, p, p, p, p, p, p, need - 1, 2, 65, 64, 32, 1, EPS, 0.2, 1, None) == -1 and b'workspace' in lib.srhip_last_error()
    assert lib.srhip_gn_fwd(p, p, None, p, p, p, p, big, 2, 65, 64, 32, 1, EPS, 0.2, 1, None) == -1 and b'together' in lib.srhip_last_error()
