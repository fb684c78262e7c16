"""Host side of the augmentation / self-ensemble feature: the numpy restatement (tests/augment_ref.py) against Pillow and against the
recorded reference items (tests/golden/augment.npz), the op tables, Augment.draw, the refusals and the trainer's switches."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sradsgan_hip.h')


def _pil(a, rv, fliplr, fliptb):
    img = Image.fromarray(a)
    if rv:
        img = img.rotate(90 * rv, expand=True)
    if fliplr:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if fliptb:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    return np.asarray(img)


def test_op_tables_agree_with_pillow_on_an_asymmetric_image():
    from sradsgan_amd import data as D
    a = np.random.RandomState(3).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    assert len(D.DIHEDRAL_OP) == 16 and D.DIHEDRAL_OP == R.OP_OF
    assert sorted(set(R.OP_OF.values())) == list(range(8))
    for (rv, fliplr, fliptb), op in R.OP_OF.items():
        assert np.array_equal(R.apply_op(a, op), _pil(a, rv, fliplr, fliptb)), (rv, fliplr, fliptb)


def test_inverse_of_every_op_is_the_identity_on_a_non_square_array():
    from sradsgan_amd import data as D
    a = np.arange(5 * 7 * 2).reshape(5, 7, 2)
    assert tuple(D.DIHEDRAL_INVERSE) == R.INVERSE
    for op in range(8):
        assert np.array_equal(R.apply_op(R.apply_op(a, op), R.INVERSE[op]), a), op
        assert np.array_equal(R.apply_op(R.apply_op(a, R.INVERSE[op]), op), a), op
        assert R.apply_op(a, op).shape[:2] == ((7, 5) if op & 1 else (5, 7))
    b = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)                 # the NCHW form the merge uses
    for op in range(8):
        assert np.array_equal(R.apply_op(R.apply_op(b, op, (2, 3)), R.INVERSE[op], (2, 3)), b)


def test_restatement_reproduces_every_golden_case(golden):
    g = golden('augment')
    src, cases, cs = g['src'], g['cases'], g['hr'].shape[1]
    assert src.shape == (3, 17, 15, 3) and cs == 12 and len(cases) == 17
    assert sorted(set(map(tuple, cases[:16, 3:].tolist()))) == sorted(R.OP_OF)          # every (rv, fliplr, fliptb) once
    offs = set(map(tuple, cases[:, 1:3].tolist()))
    assert {(0, 0), (5, 3), (0, 3), (5, 0)} <= offs and any(0 < y < 5 and 0 < x < 3 for y, x in offs)
    for k, (s, y0, x0, rv, fliplr, fliptb) in enumerate(cases.tolist()):
        noisy = k == len(cases) - 1
        params = np.array([[y0, x0, R.OP_OF[(rv, fliplr, fliptb)], 0]])
        got = R.augment(src[s:s + 1], params, cs, float(g['noise_sigma']) if noisy else 0.0, g['noise_z'][None] if noisy else None)[0]
        assert np.array_equal(got, g['hr'][k]), k
        for scale in (2, 3):                                                         # Pillow here resamples the restated tile alike
            lr = Image.fromarray(got).resize((cs // scale, cs // scale), Image.BICUBIC)
            assert np.array_equal(np.asarray(lr), g['lr%d' % scale][k]), (k, scale)
            assert np.array_equal(np.asarray(lr.resize((cs, cs), Image.BICUBIC)), g['bc%d' % scale][k]), (k, scale)
    last = cases[-1].tolist()
    plain = R.augment(src[last[0]:last[0] + 1], np.array([[last[1], last[2], R.OP_OF[tuple(last[3:])], 0]]), cs)[0]
    assert not np.array_equal(plain, g['hr'][-1])                                     # the noise case does carry noise


def test_noise_is_float64_clip_then_truncation():
    crop = np.array([[[0, 10, 250, 255]]], np.uint8)
    z = np.array([[[-1.0, 0.99, 1.0, 0.5]]], np.float32)
    assert R.add_noise(crop, 10.0, z).tolist() == [[[0, 19, 255, 255]]]                # 9.9 above 10 truncates to 19
    z = np.array([[[0.0, np.float32(0.9999999), 0.0, 0.0]]], np.float32)
    assert R.add_noise(crop, 1.0, z)[0, 0, 1] == 10                                    # 10.99999994 in float64: still 10


def test_draw_is_seeded_bounded_and_follows_the_reference_rules():
    from sradsgan_amd.data import Augment, calculate_valid_crop_size
    kw = dict(random_crop=True, rotate=True, fliplr=True, fliptb=True)
    a, b, other = Augment(13, 2, seed=7, **kw), Augment(13, 2, seed=7, **kw), Augment(13, 2, seed=7, rank=1, **kw)
    assert a.crop_size == calculate_valid_crop_size(13, 2) == 12
    ta, tb, tc = a.draw(64, 20, 17), b.draw(64, 20, 17), other.draw(64, 20, 17)
    assert ta.dtype == torch.int32 and tuple(ta.shape) == (64, 4) and not ta.is_cuda
    assert torch.equal(ta, tb) and not torch.equal(ta, tc)                              # same seed, same table; ranks differ
    assert torch.equal(Augment(13, 2, seed=8, **kw).draw(64, 20, 17), tc)               # seed + rank is the generator's seed
    assert not torch.equal(a.draw(64, 20, 17), ta)                                      # the stream advances
    t = Augment(12, 3, seed=1, **kw).draw(10000, 20, 17)
    assert int(t[:, 0].min()) == 0 and int(t[:, 0].max()) == 8 and int(t[:, 1].min()) == 0 and int(t[:, 1].max()) == 5
    assert int(t[:, 3].abs().max()) == 0
    # rv is never 0: with rotation on, an op is one of the 12 that (rv, fliplr, fliptb), rv in {1, 2, 3}, reach -- with the flips
    # off, exactly the three rotations
    r = Augment(12, 3, seed=1, random_crop=True, rotate=True).draw(10000, 20, 17)
    assert sorted(set(r[:, 2].tolist())) == [3, 5, 6]
    f = Augment(12, 3, seed=1, fliplr=True).draw(10000, 20, 17)
    assert sorted(set(f[:, 2].tolist())) == [0, 4] and 0.45 < float((f[:, 2] == 4).float().mean()) < 0.55     # p = 1/2, 10 sigma wide
    assert sorted(set(t[:, 2].tolist())) == list(range(8))
    c = Augment(12, 3, seed=1, fliptb=True).draw(5, 17, 15)                             # centre crop, odd margin: 5 -> 2 (3 -> 2: half to even)
    assert set(c[:, 0].tolist()) == {int(round(5 / 2.0))} == {2} and set(c[:, 1].tolist()) == {int(round(3 / 2.0))}
    assert torch.equal(Augment(12, 3, seed=1).draw(3, 12, 12)[:, :3], torch.zeros(3, 3, dtype=torch.int32))


def test_refusals_say_why():
    from sradsgan_amd.data import Augment
    with pytest.raises(NotImplementedError, match='squash'):
        Augment(12, 3, random_scale=True)
    with pytest.raises(NotImplementedError, match='Poisson'):
        Augment(12, 3, noise=['Poisson', 0.1])
    with pytest.raises(NotImplementedError, match='is_gray'):
        Augment(12, 3, is_gray=True)
    with pytest.raises(NotImplementedError, match='smaller than the 12 crop'):
        Augment(12, 3).draw(2, 11, 20)
    with pytest.raises(ValueError, match='Gaussain'):
        Augment(12, 3, noise=['Uniform', 1.0])
    assert Augment(12, 3, noise=['Gaussain', 2.5]).sigma == 2.5
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Augment(12, 3)(torch.zeros(1, 12, 12, 3, dtype=torch.uint8))


def test_trainer_switches_default_off_and_build_no_augment():
    from sradsgan_amd import data as D
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model import drcan
    for args in (T.default_args(), drcan.default_args()):
        for name in ('augment_random_crop', 'augment_rotate', 'augment_fliplr', 'augment_fliptb', 'self_ensemble'):
            assert getattr(args, name) is False, name
        assert args.augment_noise is None and args.augment_seed is None
        assert T.training_augment(args) is None
    import argparse
    assert T.training_augment(argparse.Namespace(crop_size=216, scale_factor=8)) is None            # a reference Namespace: no fields
    aug = T.training_augment(T.default_args(augment_rotate=True, augment_seed=5, crop_size=50, scale_factor=4), rank=2)
    assert isinstance(aug, D.Augment) and aug.crop_size == 48 and aug.rotate and not aug.fliplr and aug.seed == 7
    assert T.training_augment(T.default_args(augment_noise=['Gaussain', 3.0])).sigma == 3.0
    with pytest.raises(NotImplementedError):
        T.training_augment(T.default_args(augment_noise=['Poisson', 3.0]))


def test_ensemble_refuses_bad_arguments_before_touching_the_device():
    from sradsgan_amd import ensemble as E
    x = torch.zeros(1, 3, 4, 6)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.dihedral(x, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        E.self_ensemble(lambda t: t, x)
    with pytest.raises(ValueError, match='0..7'):
        E.self_ensemble(lambda t: t, x, ops=[0, 8])
    with pytest.raises(ValueError, match='distinct'):
        E.self_ensemble(lambda t: t, x, ops=[1, 1])
    with pytest.raises(TypeError):
        E.dihedral(x.double(), 1)
    net = torch.nn.Conv2d(3, 3, 1)
    wrapped = E.SelfEnsemble(net)
    assert list(wrapped.parameters()) == list(net.parameters()) and wrapped.ops == list(range(8))
    wrapped.eval()
    assert not net.training


# --------------------------------------------------------------------------------------------- #
# ABI: the new entry points are declared alike in the header and the ctypes table, and refuse bad arguments on the host
# --------------------------------------------------------------------------------------------- #

_CTYPES = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
           'unsigned long long': ctypes.c_ulonglong}


def _header_signature(name):
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, name
    args = []
    for a in m.group(1).split(','):
        a = ' '.join(a.replace('const', '').split())
        args.append(ctypes.c_void_p if '*' in a else _CTYPES[a.rsplit(' ', 1)[0]])
    return ctypes.c_int, args


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


@pytest.mark.parametrize('name', ['srhip_augment_u8', 'srhip_dihedral_f32', 'srhip_ensemble_merge_f32'])
def test_new_entry_points_are_declared_alike(lib, name):
    from sradsgan_amd import _hip
    assert _hip.SIGNATURES[name] == _header_signature(name)
    assert getattr(lib, name) is not None
    assert lib.srhip_abi_version() == 14                                             # additive: the version does not move


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    one = ctypes.c_void_p(16)                                                        # never dereferenced: refused before any launch
    assert lib.srhip_augment_u8(None, None, None, None, 1, 8, 8, 3, 8, 0.0, 0, 0, 0, None) == -1 and b'null tensor' in lib.srhip_last_error()
    assert lib.srhip_augment_u8(one, one, None, one, 1, 8, 7, 3, 8, 0.0, 0, 0, 0, None) == -1 and b'does not fit' in lib.srhip_last_error()
    assert lib.srhip_augment_u8(one, one, None, ctypes.c_void_p(18), 1, 8, 8, 3, 8, 0.0, 0, 0, 0, None) == -1
    assert b'aligned' in lib.srhip_last_error()
    assert lib.srhip_augment_u8(one, one, None, one, 1, 8, 8, 3, 8, 1.0, 0, 0, 0, None) == -1 and b'needs z' in lib.srhip_last_error()
    assert lib.srhip_augment_u8(one, one, one, one, 1, 8, 8, 3, 8, 1.0, 1, 0, 0, None) == -1 and b'not both' in lib.srhip_last_error()
    st = (ctypes.c_long * 4)(60, 20, 5, 1)
    assert lib.srhip_dihedral_f32(one, st, ctypes.c_void_p(32), st, 1, 3, 4, 5, 8, None) == -1 and b'0..7' in lib.srhip_last_error()
    assert lib.srhip_dihedral_f32(one, st, one, st, 1, 3, 4, 5, 1, None) == -1 and b'in place' in lib.srhip_last_error()
    ptrs, ops = (ctypes.c_void_p * 9)(*([16] * 9)), (ctypes.c_int * 9)()
    sts = (ctypes.c_long * 36)(*([60, 20, 5, 1] * 9))
    assert lib.srhip_ensemble_merge_f32(ptrs, sts, ops, 9, ctypes.c_void_p(32), st, 1, 3, 4, 5, None) == -1
    assert b'1..8' in lib.srhip_last_error()
    assert lib.srhip_ensemble_merge_f32(ptrs, sts, ops, 0, ctypes.c_void_p(32), st, 1, 3, 4, 5, None) == -1
    ops[1] = 9
    assert lib.srhip_ensemble_merge_f32(ptrs, sts, ops, 2, ctypes.c_void_p(32), st, 1, 3, 4, 5, None) == -1
    assert b'outside 0..7' in lib.srhip_last_error()
