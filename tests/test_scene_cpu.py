"""Tiled scene super-resolution, the parts that need no GPU: the geometry of sradsgan_amd/scene.py against its fp64
restatement (tests/scene_ref.py) and against first principles, the refusals of the public entry point, and the
declarations of the two new C entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import scene_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sradsgan_hip.h')

LENGTHS, TILES, OVERLAPS, SCALES = (16, 17, 37, 64), (16, 40), (0, 1, 4, 15), (1, 3)
CASES = [(L, t, ov, s) for L in LENGTHS for t in TILES for ov in OVERLAPS for s in SCALES]


@pytest.mark.parametrize('L,t,ov,scale', CASES)
def test_axis_plan_properties(L, t, ov, scale):
    from sradsgan_amd.scene import AxisPlan
    ax = AxisPlan(L, t, ov, scale)
    tt = min(t, L)
    assert ax.tile == tt and ax.hr_tile == tt * scale and ax.hr_length == L * scale
    if t >= L:
        assert ax.n == 1
    assert len(ax.positions) == ax.n and ax.positions[0] == 0 and ax.positions[-1] == L - tt
    assert all(0 <= p and p + tt <= L for p in ax.positions)                         # every position is in range
    assert all(b > a for a, b in zip(ax.positions, ax.positions[1:]))
    covered = np.zeros(L, bool)
    for p in ax.positions:
        covered[p:p + tt] = True
    assert covered.all()                                                             # the union of the tiles is [0, L)
    assert ax.hr_positions == [p * scale for p in ax.positions]
    assert all(o >= 0 for o in ax.overlaps) and ax.overlaps[0] == 0
    # the restatement agrees bit for bit
    ref = R.axis(L, t, ov, scale)
    assert ax.n == ref['n'] and ax.positions == ref['positions'] and ax.overlaps == ref['o']
    assert ax.weights.dtype == np.float32 and np.array_equal(ax.weights, ref['w'])
    # weights: in (0, 1], exactly 1 outside the overlaps, positive total everywhere
    assert (ax.weights > 0).all() and (ax.weights <= 1).all()
    T, count, total = ax.hr_tile, np.zeros(L * scale, int), np.zeros(L * scale)
    for i, a in enumerate(ax.hr_positions):
        count[a:a + T] += 1
        total[a:a + T] += ax.weights[i]
        lo = ax.overlaps[i]
        hi = T - (ax.overlaps[i + 1] if i + 1 < ax.n else 0)
        assert (ax.weights[i, lo:hi] == 1).all()
    assert (count >= 1).all() and (total > 0).all()
    for i, a in enumerate(ax.hr_positions):
        alone = count[a:a + T] == 1
        assert (ax.weights[i][alone] == 1).all()
    # cover table = brute force, and contiguous
    for y in range(L * scale):
        mine = [i for i, a in enumerate(ax.hr_positions) if a <= y < a + T]
        assert mine == list(range(ax.cover[y, 0], ax.cover[y, 1])) and mine


@pytest.mark.parametrize('L,t,ov,scale', CASES)
def test_finalisation_ranges_and_ring_depth(L, t, ov, scale):
    from sradsgan_amd.scene import ScenePlan
    plan = ScenePlan(L, 23, scale, t, ov)
    assert (plan.hr_h, plan.hr_w) == (L * scale, 23 * scale) and (plan.th, plan.tw) == (min(t, L), min(t, 23))
    assert len(plan.row_final) == plan.ys.n
    edge = 0
    for r0, r1 in plan.row_final:                                                    # a partition of the HR rows, in order
        assert r0 == edge and r1 > r0
        edge = r1
    assert edge == plan.hr_h
    needed = 1
    for j, (r0, r1) in enumerate(plan.row_final):
        for y in range(r0, r1):
            k0, k1 = plan.ys.cover[y]
            assert k1 - 1 <= j                                                       # every covering tile row has been run
            assert j - k0 < plan.ring_depth                                          # and is still in a ring of that depth
            needed = max(needed, j - k0 + 1)
    assert needed == plan.ring_depth                                                 # sufficient, and not more than that
    if plan.ys.n == 1:
        assert plan.ring_depth == 1
    assert plan.origins(plan.ys.n - 1) == [(plan.ys.positions[-1], x) for x in plan.xs.positions]
    assert R.origins(L, 23, t, ov) == [o for j in range(plan.ys.n) for o in plan.origins(j)]


def test_identity_geometry_without_overlap():
    from sradsgan_amd.scene import ScenePlan
    plan = ScenePlan(32, 48, 2, 16, 0)
    assert plan.ys.positions == [0, 16] and plan.xs.positions == [0, 16, 32] and plan.ring_depth == 1
    assert (plan.ys.weights == 1).all() and (plan.xs.weights == 1).all()
    assert plan.row_final == [(0, 32), (32, 64)]


def test_reference_blend_is_exact_where_it_must_be():
    """The restatement itself: overlap 0 pastes, one tile returns the tile, and fp32 stays within a few roundings of fp64."""
    tiles = R.random_tiles(6, 32, 32, 1)
    out = R.blend(32, 48, 2, 16, 0, tiles, torch.float32)
    for k, (y, x) in enumerate(R.origins(32, 48, 16, 0)):
        assert torch.equal(out[2 * y:2 * y + 32, 2 * x:2 * x + 32], tiles[k].permute(1, 2, 0))
    one = R.random_tiles(1, 20, 14, 2)
    assert torch.equal(R.blend(10, 7, 2, 16, 4, one, torch.float32), one[0].permute(1, 2, 0))
    tiles = R.random_tiles(len(R.origins(37, 29, 16, 15)), 32, 32, 3)
    a, b = R.blend(37, 29, 2, 16, 15, tiles, torch.float32), R.blend(37, 29, 2, 16, 15, tiles, torch.float64)
    assert float((a.double() - b).abs().max()) < 1e-5
    q, decided = R.quantise(b)
    assert q.dtype == torch.uint8 and int(q.min()) == 0 and int(q.max()) == 255 and bool(decided.any())


def test_refusals():
    from sradsgan_amd.scene import super_resolve_scene
    gen = torch.nn.Conv2d(3, 3, 1)
    ok = torch.zeros(20, 20, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='overlap'):
        super_resolve_scene(gen, ok, 2, 8, 8)
    with pytest.raises(ValueError, match='overlap'):
        super_resolve_scene(gen, ok, 2, 8, 9)
    with pytest.raises(ValueError, match='uint8'):
        super_resolve_scene(gen, ok.float(), 2, 8, 2)
    with pytest.raises(ValueError, match='HWC'):
        super_resolve_scene(gen, torch.zeros(20, 20, 4, dtype=torch.uint8), 2, 8, 2)
    with pytest.raises(ValueError, match='HWC'):
        super_resolve_scene(gen, torch.zeros(3, 20, 20, dtype=torch.uint8), 2, 8, 2)
    with pytest.raises(ValueError, match='HWC'):
        super_resolve_scene(gen, torch.zeros(20, 20, dtype=torch.uint8), 2, 8, 2)
    was_training = gen.training
    with pytest.raises(RuntimeError, match='no CPU fallback'):                       # a CPU generator: ops._require_gpu
        super_resolve_scene(gen, ok, 2, 8, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        super_resolve_scene(gen, ok.numpy(), 2, 8, 2)
    assert gen.training == was_training


# --------------------------------------------------------------------------------------------- #
# ABI: the new entry points are declared identically in the header and in the ctypes table
# --------------------------------------------------------------------------------------------- #

_CTYPES = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _header_signature(name):
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\b(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, name
    args = []
    for a in m.group(2).split(','):
        a = a.strip()
        if '*' in a:
            args.append(ctypes.c_void_p)
        else:
            args.append(_CTYPES[a.replace('const', '').split()[0]])
    return _CTYPES[m.group(1).split()[-1]], args


@pytest.mark.parametrize('name', ['srhip_scene_tiles_u8', 'srhip_scene_blend_u8'])
def test_new_entry_points_are_declared_alike(name):
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    res, args = _header_signature(name)
    assert _hip.SIGNATURES[name] == (res, args)
    assert getattr(lib, name) is not None
    assert lib.srhip_abi_version() == 14                                             # additive: the version does not move


def test_entry_points_refuse_bad_arguments_on_the_host():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    assert lib.srhip_scene_tiles_u8(None, 4, 4, None, 1, 2, 2, None, None) == -1 and b'null tensor' in lib.srhip_last_error()
    one = ctypes.c_void_p(16)                                                        # never dereferenced: refused before any launch
    assert lib.srhip_scene_tiles_u8(one, 4, 4, one, 1, 5, 2, one, None) == -1 and b'does not fit' in lib.srhip_last_error()
    assert lib.srhip_scene_blend_u8(*([None, 1, 1, 1, 1] + [None] * 6 + [1] * 8 + [None] * 3)) == -1
    args = [one, 1, 1, 1, 1] + [one] * 6 + [1, 1, 4, 4, 4, 4]
    assert lib.srhip_scene_blend_u8(*(args + [0, 5, one, None, None])) == -1 and b'rows' in lib.srhip_last_error()
    assert lib.srhip_scene_blend_u8(*(args + [0, 4, None, None, None])) == -1 and b'no output' in lib.srhip_last_error()
    assert lib.srhip_scene_blend_u8(*(args + [0, 4, ctypes.c_void_p(18), None, None])) == -1 and b'aligned' in lib.srhip_last_error()
    assert lib.srhip_scene_blend_u8(*(args + [2, 2, one, None, None])) == 0         # an empty band: nothing to launch
