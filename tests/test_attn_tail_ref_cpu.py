"""tests/attn_tail_ref.py checked on the CPU: the closed-form fp64 reference of the attention tail against fp64 autograd of the
straightforward stock-torch formulation, its first-index routing on the tie families, and -- for every case tests/test_attn_tail_gpu.py
runs -- the margin preconditions that keep an fp32 kernel's arg-max and ReLU decisions away from a flip."""
import pytest
import torch

from tests import attn_tail_ref as A

C = A.C
TIGHT = 1e-11          # two fp64 evaluations of the same formula in different orders


def _rel(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


TIE_FREE = [c for c in A.ALL_CASES if c[0] in A.FAMILIES[:3] and c[1] * c[2] * c[3] <= 2 * 13 * 70]


@pytest.mark.parametrize('case', TIE_FREE, ids=A.case_id)
def test_closed_forms_agree_with_fp64_autograd_of_the_stock_formulation(case):
    """Forward and backward of the reference against F.adaptive_avg_pool2d / F.adaptive_max_pool2d / max(dim 1) / F.conv2d under
    fp64 autograd, on inputs without ties (there torch's choice of index is the only one)."""
    t = A.case_inputs(*case)
    f = A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    b = A.tail_bwd_parts(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'])
    s = A.tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], t['dz'], torch.float64)
    for k in ('avg', 'mx', 's', 'pooled', 'm', 'z'):
        assert _rel(f[k], s[k]) < TIGHT, k
    for k in ('du', 'dfc1', 'dfc2', 'dw7'):
        assert _rel(b[k], s[k]) < TIGHT, k
    n, _, h, w = t['u'].shape
    uf = t['u'].double().reshape(n, C, h * w)
    assert torch.equal(f['arg'], uf.argmax(2)) and torch.equal(f['argc'], (f['s'][:, :, None] * uf).argmax(1))
    assert torch.equal(f['mx'], uf.gather(2, f['arg'][:, :, None]).squeeze(2))
    # the same gradients when the indices are handed in, and through the gathering form of the stock formulation
    du, dfc1, dfc2, dw7 = A.tail_bwd_ref(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], f['arg'].int(), f['argc'].int())
    assert torch.equal(du, b['du']) and torch.equal(dfc1, b['dfc1']) and torch.equal(dfc2, b['dfc2']) and torch.equal(dw7, b['dw7'])
    sg = A.tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], t['dz'], torch.float64, f['arg'], f['argc'])
    for k in ('du', 'dfc1', 'dfc2', 'dw7'):
        assert _rel(b[k], sg[k]) < TIGHT, k


@pytest.mark.parametrize('shape', A.TIE_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_pixel_ties_send_the_gradient_to_the_first_pixel(shape):
    n, h, w = shape
    hw = h * w
    t = A.case_inputs('pixel_ties', n, h, w)
    p1, p2 = A.tie_pixels(hw)
    uf = t['u'].reshape(n, C, hw)
    assert torch.equal(uf[:, A.TIE_C, p1], uf[:, A.TIE_C, p2]) and bool((uf[:, A.TIE_C, p1] == uf[:, A.TIE_C].amax(1)).all())
    assert bool((uf[:, A.CONST_C] == A.CONST_VALUE).all())
    f = A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    assert bool((f['arg'][:, A.TIE_C] == p1).all()) and bool((f['arg'][:, A.CONST_C] == 0).all())
    b = A.tail_bwd_parts(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'])
    extra = (b['du'] - b['du_spatial']).reshape(n, C, hw) - b['davg'][:, :, None] / hw        # what the max pool's backward added
    assert float(b['dmax'][:, [A.TIE_C, A.CONST_C]].abs().min()) > 0
    for c, win in ((A.TIE_C, p1), (A.CONST_C, 0)):
        lose = torch.ones(hw, dtype=torch.bool)
        lose[win] = False
        assert float(extra[:, c, lose].abs().max()) < TIGHT * float(b['dmax'].abs().max()), 'a losing pixel received dmax'
        assert _rel(extra[:, c, win], b['dmax'][:, c]) < 1e-9
    # the gathering autograd form at those indices is the same gradient
    sg = A.tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], t['dz'], torch.float64, f['arg'], f['argc'])
    for k in ('du', 'dfc1', 'dfc2', 'dw7'):
        assert _rel(b[k], sg[k]) < TIGHT, k
    # without the exemption of the constructed ties the reporter sees them
    assert float(A.pixel_margin(t['u']).min()) == 0.0


@pytest.mark.parametrize('shape', A.TIE_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_channel_ties_send_the_gradient_to_the_first_channel(shape):
    n, h, w = shape
    hw = h * w
    t = A.case_inputs('channel_ties', n, h, w)
    f = A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    b = A.tail_bwd_parts(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'])
    y = f['s'][:, :, None] * t['u'].double().reshape(n, C, hw)
    g = t['dz'].double().reshape(n, C, hw)
    dsp = b['du_spatial'].reshape(n, C, hw)
    for c1, c2 in A.CHANNEL_TIES:
        assert torch.equal(y[:, c1], y[:, c2])
        won = f['argc'] == c1
        assert int(won.sum()) > 0, 'the tied pair is nowhere the maximum: the case checks nothing'
        assert torch.equal(y[:, c1][won], y.amax(1)[won]) and not bool((f['argc'] == c2).any())
        plain = lambda c: f['s'][:, c, None] * (f['m'] * g[:, c] + b['dpooled'][:, :, 0] / C)      # no arg-max term
        assert _rel(dsp[:, c2], plain(c2)) < TIGHT, 'the second channel of a tie received the max pool gradient'
        assert _rel(dsp[:, c1], plain(c1) + f['s'][:, c1, None] * won * b['dpooled'][:, :, 1]) < TIGHT
        assert float((f['s'][:, c1, None] * won * b['dpooled'][:, :, 1]).abs().max()) > 0
    sg = A.tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], t['dz'], torch.float64, f['arg'], f['argc'])
    for k in ('du', 'dfc1', 'dfc2', 'dw7'):
        assert _rel(b[k], sg[k]) < TIGHT, k
    assert float(A.channel_margin(t['u'], t['fc1'], t['fc2']).min()) == 0.0


def test_end_to_end_reference_agrees_with_fp64_autograd():
    """e2e_ref (the reference composed with an fp64 1x1 conv) against autograd of conv2d(z) + bias + skip in fp64, and the fp32
    yardstick lands within fp32 rounding of it."""
    import torch.nn.functional as F
    t = A.case_inputs('normal', 2, 3, 5)
    r = A.e2e_ref(t)
    leaves = [t[k].double().requires_grad_() for k in ('u', 'skip', 'fc1', 'fc2', 'w7', 'wc', 'bc')]
    u, skip, fc1, fc2, w7, wc, bc = leaves
    avg, mx = F.adaptive_avg_pool2d(u, 1), F.adaptive_max_pool2d(u, 1)
    hid = fc1.shape[0]
    mlp = lambda x: F.conv2d(F.relu(F.conv2d(x, fc1.reshape(hid, C, 1, 1))), fc2.reshape(C, hid, 1, 1))
    y = torch.sigmoid(mlp(avg) + mlp(mx)) * u
    z = torch.sigmoid(F.conv2d(torch.cat([y.mean(1, keepdim=True), y.max(1, keepdim=True)[0]], 1), w7, padding=3)) * y
    out = F.conv2d(z, wc, bc) + skip
    grads = torch.autograd.grad(out, leaves, t['g'].double())
    got = dict(zip(A.E2E_NAMES, (out.detach(),) + grads))
    f = A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    y32 = A.e2e_torch32(t, f['arg'], f['argc'])
    for k in A.E2E_NAMES:
        assert _rel(r[k].reshape(got[k].shape), got[k]) < TIGHT, k
        assert _rel(y32[k].reshape(got[k].shape), got[k]) < 1e-4, k


@pytest.mark.parametrize('case', A.ALL_CASES, ids=A.case_id)
def test_every_gpu_case_keeps_its_distance_from_a_flip(case):
    """channel_margin > 1e-4 at every pixel, pixel_margin > 1e-4 for every channel, relu_margin > 1e-3 for every hidden unit, in the
    fp64 reference; the tie families are exempt on exactly their constructed ties.  This is where the seeds are chosen."""
    A.assert_margins(A.case_inputs(*case), A.case_id(case))


def test_every_shape_the_gpu_tests_use_has_a_seeded_case():
    for shapes in (A.SHAPES, A.ACC_SHAPES, A.STANDALONE_SHAPES, A.PLANE_SHAPES, A.E2E_SHAPES, A.EVAL_SHAPES, [A.HIDDEN_SHAPE]):
        for shape in shapes:
            assert ('normal',) + tuple(shape) + (4,) in A.SEEDS, shape
    assert set(A.ALL_CASES) == set(A.SEEDS)
    assert max(n * h * w for n, h, w in A.SHAPES) == 2 * 54 * 54


def test_margin_reporters_see_a_near_tie():
    t = A.case_inputs('normal', 2, 3, 5)
    u = t['u'].clone()
    uf = u.view(2, C, 15)
    top, idx = uf[0, 7].max(0)
    uf[0, 7, (int(idx) + 4) % 15] = top * (1 - 2e-6) if top > 0 else top * (1 + 2e-6)
    assert float(A.pixel_margin(u).min()) < 1e-5 < A.PIXEL_MARGIN
    # a hidden unit whose weights are orthogonal to avg: |fc1 avg| = 0 relative to sum |w x|
    avg = t['u'].double().mean((2, 3))[0]
    fc1 = t['fc1'].double().clone()
    fc1[0] -= (fc1[0] @ avg) / (avg @ avg) * avg
    assert float(A.relu_margin(t['u'], fc1)[0, 0, 0]) < 1e-12
