"""csrc/amssrn.hip's non-local attention on image quadrants, srhip_nl_quad_fwd / _bwd through the C ABI (ctypes), where the model-level
test never goes: 1 x 1 quadrants (h = w = 2: y = g and dg = dy exactly), odd sizes with 1-wide quadrants, image boundaries inside a
256-thread block and a ragged last block with n > 1, and logits in the hundreds -- the kernels run an online soft-max on unscaled
energies.  Families: unit-scale operands, sharp (operand scale 2.5, saturated rows), keys ascending along the walk (the running
maximum moves at every key), descending (never after the first), all keys equal.

Protocol of tests/test_cbam_gpu.py: every tensor lies in a pointwise_ref.Guarded allocation (sentinel bands, outputs NaN, the saved ml
and the dd scratch exactly n h w 2 and n h w floats), bands and inputs intact after every call, two runs with equal bits.  The measure
is err = max|got - ref64| / max|ref64| per output (tests/reduction_ref.py) and the bar 8 x the same err of stock fp32 torch on the CPU
(soft-max, matmuls), floor 32 * 2^-24; the kernels' own formulation evaluated in fp32 on the CPU is printed next to it.  'equal' makes
dtheta zero in exact arithmetic; it is measured against the largest sum of its absolute terms (leaf_kernels_ref.nl_scales)."""
import pytest
import torch

from tests import leaf_kernels_ref as L
from tests.test_reductions_gpu import _lib, _ok, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32
CASES = [(f,) + s for s in L.NL_SHAPES for f in L.NL_FAMILIES]
GRADS = ('dtheta', 'dphi', 'dg')
_cache = {}


def _refs(family, n, h, w):
    key = (family, n, h, w)
    if key not in _cache:
        inp = L.nl_inputs(family, n, h, w)
        _cache[key] = (inp, L.nl_eval(inp, F64), L.nl_eval(inp, F32), L.nl_eval_online32(inp), L.nl_scales(family, inp))
    return _cache[key]


def _run(inp, img=None):
    """forward, then backward from the forward's own saved y and ml; img: that image alone."""
    t = {k: (v if img is None else v[img:img + 1]) for k, v in inp.items()}
    n, h, w, _ = t['theta'].shape
    lib, b = _lib(), L.Buffers(DEV)
    p = {k: b.put(k, v) for k, v in t.items()}
    _ok(lib.srhip_nl_quad_fwd(p['theta'], p['phi'], p['g'], b.out('y', n, h, w, 8), b.out('ml', n * h * w * 2), n, h, w, _stream()), 'nl_quad_fwd')
    torch.cuda.synchronize()
    _ok(lib.srhip_nl_quad_bwd(p['theta'], p['phi'], p['g'], b.ptr('y'), b.ptr('ml'), p['dy'], b.out('dd', n * h * w), b.out('dtheta', n, h, w, 8),
                              b.out('dphi', n, h, w, 8), b.out('dg', n, h, w, 8), n, h, w, _stream()), 'nl_quad_bwd')
    torch.cuda.synchronize()
    return b


def _outputs(b, n, h, w):
    ml = b.get('ml').view(n, h, w, 2)
    got = {k: b.get(k) for k in ('y',) + GRADS}
    got.update(m=ml[..., 0].contiguous(), l=ml[..., 1].contiguous())
    return got


@pytest.mark.parametrize('family,n,h,w', CASES, ids=['%s-%dx%dx%d' % c for c in CASES])
def test_quadrant_attention_forward_and_every_gradient(family, n, h, w):
    """y, the saved m and l, dtheta, dphi, dg of every image against fp64.
    Worst err (fp32 torch, bar) per family on the MI355X, none above 0.31 of its bar, no bar needed the kernel-formulation yardstick --
    which, evaluated in fp32 on the CPU, draws the kernels' own figures to three digits:
      unit        dtheta 1.4e-6 (7.5e-7, 6.0e-6) at 1 x 2 x 515      sharp       dphi 3.4e-6 (1.4e-6, 1.1e-5) at 3 x 17 x 31
      ascending   dtheta 1.6e-5 (6.6e-6, 5.3e-5) at 1 x 2 x 515      descending  dtheta 2.5e-5 (1.1e-5, 9.0e-5) at 1 x 33 x 32
      equal       dphi 3.9e-7 (3.1e-7, 2.5e-6) at 3 x 17 x 31; dtheta 6.0e-8 of the sum of its absolute terms
    y at 1 x 33 x 32: unit 1.0e-6 (6.2e-7), sharp 2.0e-6 (1.4e-6); dg sharp 6.4e-7 (4.3e-7)."""
    inp, ref, t32, online, scales = _refs(family, n, h, w)
    tab = L.table('nl_quad %s %dx%dx%d' % (family, n, h, w))
    first, second = _run(inp), _run(inp)
    tab.guards(first, second)
    got = _outputs(first, n, h, w)
    for k in L.NL_OUT:
        tab.scaled(k, got[k], ref[k], t32[k], scales.get(k), online[k])
    if (h, w) == (2, 2):
        tab.bits('1 x 1 quadrants: y == g', got['y'], inp['g'])
        tab.bits('1 x 1 quadrants: dg == dy', got['dg'], inp['dy'])
        tab.bits('1 x 1 quadrants: l == 1', got['l'], torch.ones(n, h, w))
    for k in ('y', 'ml', 'dd') + GRADS:
        tab.rerun(k, first.get(k), second.get(k))
    tab.done()


@pytest.mark.parametrize('family', ['unit', 'sharp'])
def test_each_image_of_a_batch_equals_the_image_run_alone(family):
    """3 x 17 x 31: 527 pixels per image, so both image boundaries fall inside a block and the last block is ragged."""
    n, h, w = L.NL_INDEPENDENCE
    inp = _refs(family, n, h, w)[0]
    tab = L.table('nl_quad %s batch independence' % family)
    whole = _run(inp)
    tab.guards(whole)
    tab.true('every output written', all(bool(torch.isfinite(whole.get(k)).all()) for k in ('y', 'ml', 'dd') + GRADS))
    for img in range(n):
        alone = _run(inp, img)
        tab.guards(alone)
        for k in ('y', 'ml', 'dd') + GRADS:
            tab.rerun('image %d alone: %s' % (img, k), whole.get(k).view(n, -1)[img], alone.get(k).reshape(-1))
    tab.done()


def test_refusals_leave_every_buffer_untouched():
    L.run_refusals(_lib(), DEV, L.nl_quad_refusals)
