"""The discriminator's head conv (3 -> 64, 3x3, LeakyReLU 0.2, full image size) leaves an ACTIVATION RECORD behind -- one 64-bit word per
output pixel, bit c = (y[pixel][c] > 0) -- and the three kernels that consume the gradient at its output apply the LeakyReLU mask
from the record while they stage the gradient (ops._HEAD_BITS; srhip_conv2d_{fwd,dgrad,wgrad}_head_mask).  The mask multiply is the
same fp32 product wherever it happens and no reduction order moves, so EVERY comparison here is bit for bit (on the int32 view:
it tells +0 from -0 and compares NaNs) against the composition of the existing entry points with the switch off.

Shapes: the route needs >= 65536 pixels.  (6, 108, 108) is the plain case; (2, 150, 221) has H and W that are no multiples of 16 or
32 and W > 128, so a wave of the head conv kernel wraps its row loop; (1, 260, 255) is a single image with an odd W."""
import contextlib

import pytest
import torch

from oracle import sradsgan_ref as O
from tests.parity_util import build_pair

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SLOPE = 0.2
SHAPES = [(6, 108, 108), (2, 150, 221), (1, 260, 255)]
_CASES = {}


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@contextlib.contextmanager
def _switch(on):
    from sradsgan_amd import ops
    old, ops._HEAD_BITS = ops._HEAD_BITS, on
    try:
        yield
    finally:
        ops._HEAD_BITS = old


def _case(shape):
    """Operands of one shape and the references of the existing ops, computed once and left unchanged.  Channel 5 has zero weights
    and a zero bias (exact zeros in y, NaN around the NaN pixel), channel 9 a zero bias only; one input pixel is NaN."""
    if shape not in _CASES:
        from sradsgan_amd import ops
        n, h, w = shape
        g = torch.Generator().manual_seed(1000 * n + h + w)
        x = torch.randn(n, 3, h, w, generator=g)
        x[n - 1, 1, h // 2, w - 2] = float('nan')
        wt = torch.randn(64, 3, 3, 3, generator=g) * 0.3
        b = torch.randn(64, generator=g) * 0.1
        wt[5] = 0.0
        b[5] = 0.0
        b[9] = 0.0
        c = dict(x=_cl(x), w=wt.to(DEV), b=b.to(DEV), dy=_cl(torch.randn(n, 64, h, w, generator=g)),
                 ddx=_cl(torch.randn(n, 3, h, w, generator=g)))
        c['y'] = ops.conv2d_fwd_raw(c['x'], c['w'], c['b'], 1, 1, SLOPE)
        c['g'] = ops.lrelu_bwd_raw(c['dy'], c['y'], SLOPE)
        c['y_new'], c['bits'] = ops.conv2d_fwd_head_mask_raw(c['x'], c['w'], c['b'], SLOPE)
        torch.cuda.synchronize()
        _CASES[shape] = c
    return _CASES[shape]


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_writes_the_record_of_its_output(shape):
    """y is the plain head conv's, bit for bit, and the record equals the one derived on the host from y > 0 (NaN, +0, -0 -> 0)."""
    from sradsgan_amd import _hip, ops
    n, h, w = shape
    c = _case(shape)
    assert ops.head_mask_ok((n, 3, h, w), (64, 3, 3, 3), 1, 1)
    assert _hip.lib().srhip_conv2d_head_mask_bytes(n, h, w, 64) == n * h * w * 8 == c['bits'].numel() * 8
    assert _same(c['y_new'], c['y'])
    y = c['y'].permute(0, 2, 3, 1).reshape(-1, 64).cpu()
    assert bool(torch.isnan(y).any()) and bool((y[:, 5] == 0).any()) and bool((y > 0).any()) and bool((y < 0).any())
    pos = (y > 0).to(torch.int64)
    sh = torch.arange(32, dtype=torch.int64)
    halves = torch.stack([(pos[:, :32] << sh).sum(1), (pos[:, 32:] << sh).sum(1)], 1)     # little endian: channels 0-31, then 32-63
    halves = torch.where(halves >= (1 << 31), halves - (1 << 32), halves).to(torch.int32)
    assert torch.equal(c['bits'].cpu().view(torch.int32).view(-1, 2), halves)


@pytest.mark.parametrize('shape', SHAPES)
def test_masked_data_gradient(shape):
    from sradsgan_amd import ops
    n, h, w = shape
    c = _case(shape)
    dx = ops.conv2d_dgrad_head_mask_raw(c['dy'], c['w'], (n, 3, h, w), c['bits'], SLOPE)
    assert _same(dx, ops.conv2d_dgrad_raw(c['g'], c['w'], (n, 3, h, w), 1, 1))


@pytest.mark.parametrize('shape', SHAPES)
def test_masked_weight_and_bias_gradient(shape):
    """With the bias gradient (the D step) and without it (the penalty's second-order weight gradient, whose `x` is ddx)."""
    from sradsgan_amd import ops
    c = _case(shape)
    dw, db = ops.conv2d_wgrad_raw(c['x'], c['dy'], (64, 3, 3, 3), 1, 1, True, head_bits=(c['bits'], SLOPE))
    dw0, db0 = ops.conv2d_wgrad_raw(c['x'], c['g'], (64, 3, 3, 3), 1, 1, True)
    assert _same(dw, dw0) and _same(db, db0)
    dw, db = ops.conv2d_wgrad_raw(c['ddx'], c['dy'], (64, 3, 3, 3), 1, 1, False, head_bits=(c['bits'], SLOPE))
    dw0, _ = ops.conv2d_wgrad_raw(c['ddx'], c['g'], (64, 3, 3, 3), 1, 1, False)
    assert db is None and _same(dw, dw0)


@pytest.mark.parametrize('shape', SHAPES)
def test_masked_head_conv_epilogue(shape):
    from sradsgan_amd import ops
    c = _case(shape)
    d_dy = ops.conv2d_fwd_head_mask_raw(c['ddx'], c['w'], None, SLOPE, bits=c['bits'])
    assert _same(d_dy, ops.lrelu_bwd_raw(ops.conv2d_fwd_raw(c['ddx'], c['w'], None, 1, 1), c['y'], SLOPE))
    # the second-order pass marks its input as gradient data: the same bits from the kernel that flag selects
    assert _same(d_dy, ops.lrelu_bwd_raw(ops.conv2d_fwd_raw(c['ddx'], c['w'], None, 1, 1, graddata=True), c['y'], SLOPE))


def _conv_backward(on, x0, w0, b0, dy):
    """y, dx, dw, db of ops.conv2d + LeakyReLU through autograd, and how often the forward wrote a record."""
    from sradsgan_amd import ops
    calls = []
    real = ops.conv2d_fwd_head_mask_raw

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    ops.conv2d_fwd_head_mask_raw = counted
    try:
        with _switch(on):
            x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
            y = ops.conv2d(x, w, b, 1, 1, act_slope=SLOPE)
            y.backward(dy)
            torch.cuda.synchronize()
    finally:
        ops.conv2d_fwd_head_mask_raw = real
    return [y.detach(), x.grad, w.grad, b.grad], len(calls)


def test_plain_backward_through_autograd_takes_the_record_and_keeps_every_bit():
    c = _case(SHAPES[0])
    on, used = _conv_backward(True, c['x'], c['w'], c['b'], c['dy'])
    off, unused = _conv_backward(False, c['x'], c['w'], c['b'], c['dy'])
    assert used == 1 and unused == 0
    assert all(_same(a, b) for a, b in zip(on, off))


@pytest.mark.parametrize('case', [(2, 64, 16, 16), (6, 32, 108, 108)])
def test_unserved_shapes_keep_the_old_path(case):
    """Too few pixels, or a channel count the record is not built for: switch on and switch off run the same kernels."""
    from sradsgan_amd import ops
    n, cout, h, w = case
    assert not ops.head_mask_ok((n, 3, h, w), (cout, 3, 3, 3), 1, 1)
    g = torch.Generator().manual_seed(cout + h)
    x, dy = _cl(torch.randn(n, 3, h, w, generator=g)), _cl(torch.randn(n, cout, h, w, generator=g))
    wt, b = (torch.randn(cout, 3, 3, 3, generator=g) * 0.3).to(DEV), (torch.randn(cout, generator=g) * 0.1).to(DEV)
    on, used = _conv_backward(True, x, wt, b, dy)
    off, _ = _conv_backward(False, x, wt, b, dy)
    assert used == 0
    assert all(_same(a, b) for a, b in zip(on, off))


def test_gradient_penalty_second_order_is_bit_identical():
    """sradsgan.py:595-641 on a discriminator at (6, 3, 108, 108): first-order pass under create_graph, then the penalty's backward
    (double backward through the head conv: the masked epilogue and the masked weight gradient)."""
    from sradsgan_amd import model as M
    from sradsgan_amd import ops
    od = O.Discriminator()
    O.det_init_(od, prefix='D.')
    interp0 = O.det_fill('headmask.interp', (6, 3, 108, 108), 0.5, 0.5).to(DEV)

    def run(on):
        with _switch(on):
            D = M.Discriminator().to(DEV)
            D.load_state_dict(od.state_dict(), strict=True)
            interp = interp0.clone().requires_grad_(True)
            d_out = D(interp)
            with ops.no_param_grads():
                (grads,) = torch.autograd.grad(d_out, interp, torch.ones_like(d_out), create_graph=True)
            gp = ops.gp_penalty(grads)
            with ops.bn_fold_second_order():        # as TrainStep._backward_terms runs it
                gp.backward()
            torch.cuda.synchronize()
            # (a parameter the penalty does not depend on -- the output conv's bias -- has no gradient, with or without the record)
            return gp.detach().clone(), grads.detach().clone(), [None if p.grad is None else p.grad.clone() for p in D.parameters()]

    gp1, gr1, pg1 = run(True)
    gp0, gr0, pg0 = run(False)
    assert bool(torch.isfinite(gp1)) and _same(gp1.view(1), gp0.view(1)) and _same(gr1, gr0)
    assert pg1[0] is not None and float(pg1[0].abs().max()) > 0          # the head conv's weight
    assert [a is None for a in pg1] == [b is None for b in pg0]
    assert all(_same(a, b) for a, b in zip(pg1, pg0) if a is not None)


@contextlib.contextmanager
def _count_record_calls(counts):
    """counts[kind] += 1 for every forward that writes a record ('record'), masked epilogue ('epilogue'), masked data gradient
    ('dgrad') and masked weight gradient ('wgrad') that ops launches."""
    from sradsgan_amd import ops
    real = {k: getattr(ops, k) for k in ('conv2d_fwd_head_mask_raw', 'conv2d_dgrad_head_mask_raw', 'conv2d_wgrad_raw')}

    def fwd(*a, bits=None, **k):
        counts['record' if bits is None else 'epilogue'] += 1
        return real['conv2d_fwd_head_mask_raw'](*a, bits=bits, **k)

    def dgrad(*a, **k):
        counts['dgrad'] += 1
        return real['conv2d_dgrad_head_mask_raw'](*a, **k)

    def wgrad(*a, **k):
        if k.get('head_bits') is not None:
            counts['wgrad'] += 1
        return real['conv2d_wgrad_raw'](*a, **k)
    ops.conv2d_fwd_head_mask_raw, ops.conv2d_dgrad_head_mask_raw, ops.conv2d_wgrad_raw = fwd, dgrad, wgrad
    try:
        yield
    finally:
        for k, v in real.items():
            setattr(ops, k, v)


def _train_steps(on, iters=1, **step_args):
    from sradsgan_amd.train_step import TrainStep
    B, side, scale = 6, 27, 4                       # HR 108 x 108: 69984 pixels, the smallest square the head route takes at B = 6
    lr = O.det_fill('headmask.lr', (B, 3, side, side), 0.5, 0.5).to(DEV)
    hr = O.det_fill('headmask.hr', (B, 3, side * scale, side * scale), 0.5, 0.5).to(DEV)
    al = O.det_fill('headmask.alpha', (B, 1, 1, 1), 0.5, 0.5).to(DEV)
    with _switch(on):
        (hg, hd, hf), _ = build_pair(2, 2, scale, DEV)
        step = TrainStep(hg, hd, hf, **step_args)
        scal = []
        for _ in range(iters):
            out = step(lr, hr, al)
            scal.append(torch.stack([out[k].double() for k in ('loss_G', 'loss_D', 'pixel', 'content', 'loss_gan', 'gp')]).clone())
        torch.cuda.synchronize()
        grads = [p.grad.detach().clone() for p in list(hg.parameters()) + list(hd.parameters())]
        weights = [p.detach().clone() for p in list(hg.parameters()) + list(hd.parameters())]
    return torch.stack(scal).cpu(), grads, weights


@pytest.mark.parametrize('math', ['default', 'fp32'])
def test_full_training_step_is_bit_identical(math):
    """One full iteration (sradsgan.py:818-892: the walk of D(gen), D(real), the penalty's two orders) with the record against the
    data flow without it: the six scalars and every generator / discriminator gradient."""
    from sradsgan_amd import ops
    import collections
    c1, c0 = collections.Counter(), collections.Counter()
    with (ops.conv_math('fp32') if math == 'fp32' else contextlib.nullcontext()):
        with _count_record_calls(c1):
            s1, g1, _ = _train_steps(True)
        with _count_record_calls(c0):
            s0, g0, _ = _train_steps(False)
    # the step really ran on the record: D's forwards leave one each; the walk of D(gen) and the penalty's first order take the masked
    # data gradient, the penalty's second order the masked epilogue, D(real) / the fake term / the penalty the masked weight gradient
    print('record calls per step:', dict(c1))
    assert c1['record'] >= 2 and c1['epilogue'] >= 1 and c1['dgrad'] >= 2 and c1['wgrad'] >= 2, dict(c1)
    assert not c0, dict(c0)
    assert torch.isfinite(s1).all() and torch.equal(s1, s0)
    assert all(_same(a, b) for a, b in zip(g1, g0))


def test_capture_with_per_call_record_buffers_replays_like_eager():
    """The record is allocated per forward.  The three-stream step captured into one hipGraph (1 eager warm-up + 3 replays) is bit
    identical to the eager three-stream step at a shape that takes the record: scalars of every iteration, final weights."""
    from sradsgan_amd import ops
    assert ops._HEAD_BITS
    gs, _, gw = _train_steps(True, iters=4, use_graph=True, overlap_wgrad=True, overlap_d_step=True)
    es, _, ew = _train_steps(True, iters=4, use_graph=False, overlap_wgrad=True, overlap_d_step=True)
    assert torch.isfinite(gs).all() and torch.equal(gs, es)
    assert all(_same(a, b) for a, b in zip(gw, ew))
