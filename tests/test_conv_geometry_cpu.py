"""CPU half of the conv geometry sweep: the table of tests/conv_geometry_cases.py obeys its own rules, and the fp64 emulation the GPU
tests trust (tests/conv_emulation.py) agrees with plain fp64 torch convolutions on every KIND of degenerate geometry the sweep adds --
a wrong reference at an edge would pass a wrong kernel or fail a right one.  Also the host-side refusals the table's notes rely on."""
import collections
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_emulation as E
from tests import conv_geometry_cases as C

KNOB_KEYS = (0, 1, 5, 10, 11, 17)          # the keys test_conv_routes_gpu.KNOB_DEFAULTS resets (that module needs a GPU to import its device)
OPS = ('fwd', 'fwd_ld', 'dgrad', 'dgrad_ld', 'wgrad', 'wgrad_multi', 'dil_fwd', 'dil_dgrad', 'dil_wgrad')


def test_ids_are_unique_and_rows_are_well_formed():
    dup = [k for k, v in collections.Counter(C.IDS).items() if v > 1]
    assert not dup, dup
    for r in C.ROWS:
        assert r['op'] in OPS and r['mode'] in ('fp32', 'bf16x3', 'half') and r['expect'] in E.ARITHS, r['id']
        assert r['fam'] in C.FAMILIES and r['cls'] in C.CLASSES[r['fam']], r['id']
        assert 'fam' in r['route'], r['id']
        n, cin, h, w, cout, k, s, p = r['shape']
        d = r.get('d', 1)
        assert h + 2 * p >= d * (k - 1) + 1 and w + 2 * p >= d * (k - 1) + 1, '%s: no such convolution' % r['id']


def test_every_class_has_a_row_in_every_mode_it_exists_in():
    seen = collections.defaultdict(set)
    for r in C.ROWS:
        seen[(r['fam'], r['cls'])].add(r['mode'])
    for fam in C.FAMILIES:
        need = {'bf16x3'} if fam in C.MODES16 else {'bf16x3', 'fp32'}
        for cls in C.CLASSES[fam]:
            assert need <= seen[(fam, cls)], '%s / %s: modes %s, needs %s' % (fam, cls, sorted(seen[(fam, cls)]), sorted(need))
        assert any(r['mode'] == 'half' for r in C.ROWS if r['fam'] == fam), '%s: no half row' % fam


def test_sizes_stay_under_the_caps():
    for r in C.ROWS:
        n, cin, h, w, cout, k, s, p = r['shape']
        assert n <= C.CAPS['n'] or r.get('big_n'), '%s: n = %d without a reason' % (r['id'], n)
        assert max(h, w) <= C.CAPS['side'], r['id']
        assert max(cin, cout) <= C.CAPS['chan'] or r.get('big_c'), r['id']
        assert max(r.get('ldx', 0), r.get('ldy', 0)) <= C.CAPS['chan'], r['id']


def test_every_knob_a_row_names_is_a_live_key():
    """A retired key is an argument error of srhip_debug_set: a row that names one would fail before it ran anything."""
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    for r in C.ROWS:
        for knobs in [r['knobs']] + list(r.get('same') or ()):
            for key, v in knobs.items():
                assert key in KNOB_KEYS, '%s: key %d is not reset by KNOB_DEFAULTS' % (r['id'], key)
    for key in KNOB_KEYS:
        assert lib.srhip_debug_set(key, {10: 1, 11: 1, 17: 1}.get(key, 0)) == 0, key      # (sets the default: no state left behind)


def test_patch_classes_of_the_table_are_the_documented_ones():
    used = {r['patch'] for r in C.ROWS if r.get('patch')}
    assert used == set(C.PATCH_CLASSES)


# ---- the emulation on the new degenerate geometries ------------------------------------------------------------------------------- #
# (n, cin, h, w, cout, k, stride, pad, dilation): 1 x 1 image, filter larger than the image, stride 2 onto 1 x W and H x 1, 2 x 2 and 3 x 3
# images with many samples, a 4 x 4 stride-2 filter on 2 x 2, dilation above h and w, dilation that does not divide the image
DEGENERATE = [(2, 3, 1, 1, 4, 3, 1, 1, 1), (3, 2, 2, 1, 3, 3, 1, 1, 1), (2, 2, 2, 1, 3, 5, 1, 2, 1), (3, 4, 1, 5, 2, 3, 2, 1, 1), (3, 4, 5, 1, 2, 3, 2, 1, 1),
              (5, 3, 2, 2, 4, 3, 2, 1, 1), (4, 3, 3, 3, 2, 3, 2, 1, 1), (2, 3, 2, 2, 4, 4, 2, 1, 1), (2, 3, 2, 7, 4, 4, 2, 1, 1), (2, 4, 1, 1, 4, 3, 1, 2, 2),
              (2, 4, 1, 4, 4, 3, 1, 3, 3), (2, 4, 2, 2, 4, 3, 1, 3, 3), (2, 4, 5, 7, 4, 3, 1, 2, 2), (2, 4, 5, 7, 4, 3, 1, 3, 3), (9, 2, 3, 3, 3, 3, 1, 1, 1),
              (2, 3, 7, 5, 2, 7, 1, 3, 1)]


@pytest.mark.parametrize('case', DEGENERATE, ids=lambda c: 'n%d-%dx%dx%d-c%d-k%ds%dp%dd%d' % c)
def test_emulation_agrees_with_plain_fp64_convolutions(case):
    n, cin, h, w, cout, k, s, p, d = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cin, h, w, generator=g).double()
    wt = torch.randn(cout, cin, k, k, generator=g).double()
    y = F.conv2d(x, wt, None, s, p, d)
    dy = torch.randn(y.shape, generator=g).double()
    # forward
    ref, absref = E.conv_fwd(x.float(), wt.float(), s, p, 'fp32', d)
    want = F.conv2d(x.float().double(), wt.float().double(), None, s, p, d)
    assert ref.shape == want.shape and torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(absref, F.conv2d(x.float().double().abs(), wt.float().double().abs(), None, s, p, d), rtol=1e-12, atol=1e-12)
    # data gradient: conv_transpose2d, with the output padding that restores the input size
    dyf, wf = dy.float().double(), wt.float().double()
    oph, opw = h - ((y.shape[2] - 1) * s - 2 * p + d * (k - 1) + 1), w - ((y.shape[3] - 1) * s - 2 * p + d * (k - 1) + 1)
    want = F.conv_transpose2d(dyf, wf, None, s, p, (oph, opw), 1, d)
    ref, _ = E.conv_dgrad(dy.float(), wt.float(), (n, cin, h, w), s, p, 'fp32', d)
    assert ref.shape == want.shape and torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    # weight gradient: autograd of the fp64 convolution
    wv = wf.clone().requires_grad_(True)
    F.conv2d(x.float().double(), wv, None, s, p, d).backward(dyf)
    ref, _ = E.conv_wgrad(x.float(), dy.float(), (cout, cin, k, k), s, p, 'fp32', d)
    assert torch.allclose(ref, wv.grad, rtol=1e-12, atol=1e-12)
    # the rounded arithmetics stay within their operand rounding of it (a dropped tap would be O(1))
    for arith, rel in (('bf16x3', 2.0 ** -14), ('bf16', 2.0 ** -6), ('fp16', 2.0 ** -9)):
        r2, a2 = E.conv_fwd(x.float(), wt.float(), s, p, arith, d)
        assert bool(((r2 - F.conv2d(x.float().double(), wf, None, s, p, d)).abs() <= rel * a2 + 1e-30).all()), arith


# ---- host-side refusals the table's notes rely on (argument checks only: no kernel is launched) ------------------------------------- #
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


def _fake(k):
    return ctypes.c_void_p(0x1000 * (k + 1))              # 16-byte aligned, never dereferenced: every call below is refused on the host


def test_a_filter_larger_than_the_padded_image_is_refused(lib):
    """(h + 2 pad - k) / stride + 1 in C truncates a negative numerator towards zero: with stride 2 a 4 x 4 pad-1 filter on a 1 x 1 image
    would count one output pixel that the caller's (empty) tensors do not have."""
    for (h, w, k, s, p) in ((1, 1, 4, 2, 1), (1, 5, 4, 2, 1), (5, 1, 4, 2, 1), (2, 2, 7, 2, 2), (2, 2, 6, 3, 1)):
        rc = lib.srhip_conv2d_fwd(_fake(0), _fake(1), None, None, None, None, _fake(2), 1, h, w, 16, 16, k, k, s, p, 16, 16, 16, 0.0, 0, None)
        assert rc == -1 and b'larger than the padded image' in lib.srhip_last_error(), (h, w, k, s, p)
        if p <= k - 1:
            rc = lib.srhip_conv2d_dgrad(_fake(0), _fake(1), _fake(2), None, None, 0.0, 1, h, w, 16, 16, k, k, s, p, 16, 16, 16, 0, None)
            assert rc == -1 and b'larger than the padded image' in lib.srhip_last_error(), (h, w, k, s, p)
        rc = lib.srhip_conv2d_wgrad(_fake(0), _fake(1), _fake(2), None, None, None, 0, _fake(3), 1 << 20, 1, h, w, 16, 16, k, k, s, p, 16, 16, None)
        assert rc == -1 and b'larger than the padded image' in lib.srhip_last_error(), (h, w, k, s, p)


def test_a_source_row_stride_that_is_no_multiple_of_4_is_refused(lib):
    """The dot kernel's own `lds % 4` test can therefore never decline a call from outside (the note of the dot / row-stride row)."""
    rc = lib.srhip_conv2d_fwd(_fake(0), _fake(1), None, None, None, None, _fake(2), 2, 3, 5, 48, 1, 3, 3, 1, 1, 50, 1, 1, 0.0, 0, None)
    assert rc == -1 and b'ldx % 4' in lib.srhip_last_error()


def test_the_last_route_record_is_cleared_by_a_refused_call_and_needs_no_buffer(lib):
    """A public conv entry point clears the record on entry, before its argument checks: a refused call leaves an empty record, and the
    query tolerates a missing or tiny buffer."""
    assert lib.srhip_conv2d_fwd(None, None, None, None, None, None, None, 1, 4, 4, 3, 3, 3, 3, 1, 1, 3, 3, 3, 0.0, 0, None) == -1
    buf = ctypes.create_string_buffer(b'x' * 8, 8)
    assert lib.srhip_conv2d_last_route(buf, 8) == 0 and buf.value == b''
    assert lib.srhip_conv2d_last_route(None, 0) == 0
