"""The dilated 3x3 convolution (csrc/conv_dilated.hip) and PReLU (csrc/prelu.hip) of ABI 14 against fp64 torch, in split-bf16 and
exact-fp32 conv arithmetic (and one forward in 'half'), with bit-identical reruns: dilations 1-3, even and odd sizes, 256 -> 256 and
64 -> 64, the output written into a channel slice of a [n, h, w, 768] buffer, the data gradient accumulated into a strided buffer,
every kernel family of the plain 3x3 path the sub-image batch can reach forced through srhip_debug_set, and once at training size."""
import pytest
import torch
import torch.nn.functional as F

from oracle import sradsgan_ref as O

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CL = torch.channels_last
WIDE = 768                                        # ASPP's concatenation: three 256-channel outputs


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def _wide(name, n, c, h, w, scale=1.0):
    return O.det_fill(name, (n, c, h, w), scale).to(DEV).contiguous(memory_format=CL)


class kernel_choice:
    """Forward / data-gradient kernel (srhip_debug_set key 0) and weight-gradient kernel (key 1) of the plain 3x3 path:
    'heuristic' the dispatcher's choice; 'dma' the LDS-DMA kernels; 'patch' the persistent patch kernel wherever it applies;
    'reg' the register-staged exact-fp32 kernels with the register-staged weight gradient."""

    KEYS = {'heuristic': (0, 0), 'dma': (-1, 7), 'patch': (-2, 0), 'reg': (20, 10)}

    def __init__(self, name):
        self.keys = self.KEYS[name]

    def __enter__(self):
        from sradsgan_amd import _hip
        _hip.lib().srhip_debug_set(0, self.keys[0])
        _hip.lib().srhip_debug_set(1, self.keys[1])

    def __exit__(self, *exc):
        from sradsgan_amd import _hip
        _hip.lib().srhip_debug_set(0, 0)
        _hip.lib().srhip_debug_set(1, 0)


CASES = ([(m, d, 2, 256, 256, (13, 14), 'heuristic') for m in ('bf16x3', 'fp32') for d in (1, 2, 3)]
         + [(m, d, 2, 64, 64, (12, 12), 'heuristic') for m in ('bf16x3', 'fp32') for d in (1, 2, 3)]
         + [('bf16x3', d, 2, 256, 256, (27, 27), k) for d in (2, 3) for k in ('dma', 'patch', 'reg')]
         + [('fp32', 3, 2, 64, 64, (13, 14), 'reg')]
         # sides shorter than the dilation: sub-images of 1 x 1 and 1 x 2 pixels
         + [(m, 3, 2, 64, 64, (2, 3), 'heuristic') for m in ('bf16x3', 'fp32')] + [('bf16x3', 2, 1, 256, 256, (1, 3), 'heuristic')])


@pytest.mark.parametrize('mode,d,n,cin,cout,hw,kernel', CASES)
def test_dilated_conv_strided_against_fp64_and_bit_identical(mode, d, n, cin, cout, hw, kernel):
    from sradsgan_amd import ops
    h, w = hw
    x = _wide('dil.x.%d' % cin, n, cin, h, w)
    wt = torch.nn.Parameter(O.det_fill('dil.w.%d.%d' % (cin, d), (cout, cin, 3, 3), 0.05).to(DEV))
    b = O.det_fill('dil.b.%d' % cout, (cout,), 0.1).to(DEV)
    dy = _wide('dil.dy.%d' % cout, n, cout, h, w)
    x64, w64, dy64 = x.cpu().double(), wt.detach().cpu().double(), dy.cpu().double()
    y64 = F.conv2d(x64, w64, b.cpu().double(), 1, d, d)
    dx64 = torch.nn.grad.conv2d_input(x64.shape, w64, dy64, 1, d, d)
    dw64 = torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, 1, d, d)
    tol = 5e-6 if mode == 'fp32' else 2e-5
    slot = d - 1                                   # ASPP: output d lands in channels 256 (d - 1) : 256 d of the wide buffer
    runs = []
    with ops.conv_math(mode), kernel_choice(kernel):
        for _ in range(2):
            buf = _wide('dil.buf', n, WIDE, h, w)
            before = buf.clone()
            ops.conv2d_dil_fwd_raw(x, cin, wt, b, buf[:, slot * 256:], WIDE, n, h, w, d)
            dbuf = _wide('dil.dbuf', n, WIDE, h, w)
            d0 = dbuf.clone()
            ops.conv2d_dil_dgrad_raw(dy, cout, wt, dbuf[:, 256:], WIDE, n, h, w, d, accumulate=True)
            dw, db = ops.conv2d_dil_wgrad_raw(x, cin, dy, cout, tuple(wt.shape), n, h, w, d)
            dw2, db2 = dw.clone(), db.clone()
            ops.conv2d_dil_wgrad_raw(x, cin, dy, cout, tuple(wt.shape), n, h, w, d, out=(dw2, db2))   # accumulate: 2x
            torch.cuda.synchronize()
            runs.append([t.cpu() for t in (buf, dbuf, dw, db, dw2, db2)])
    buf, dbuf, dw, db, dw2, db2 = runs[0]
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c), 'rerun differs'
    keep = torch.ones(WIDE, dtype=torch.bool)
    keep[slot * 256:slot * 256 + cout] = False
    assert torch.equal(buf[:, keep], before.cpu()[:, keep]), 'forward wrote outside its slice'
    e_y = rel_err(buf[:, slot * 256:slot * 256 + cout], y64)
    dkeep = torch.ones(WIDE, dtype=torch.bool)
    dkeep[256:256 + cin] = False
    assert torch.equal(dbuf[:, dkeep], d0.cpu()[:, dkeep]), 'data gradient wrote outside its slice'
    e_dx = rel_err(dbuf[:, 256:256 + cin].double() - d0.cpu().double()[:, 256:256 + cin], dx64)
    e_dw, e_db = rel_err(dw, dw64), rel_err(db, dy64.sum(dim=(0, 2, 3)))
    print('dilated %s d=%d %dx%d->%d %s (%s): y %.2e dx %.2e dw %.2e db %.2e' % (mode, d, n, cin, cout, hw, kernel, e_y, e_dx, e_dw, e_db))
    assert e_y < tol and e_dx < 10 * tol and e_dw < 10 * tol and e_db < 1e-5
    assert rel_err(dw2, 2 * dw64) < 10 * tol and rel_err(db2, 2 * dy64.sum(dim=(0, 2, 3))) < 1e-5


@pytest.mark.parametrize('d', [2, 3])
def test_dilated_conv_at_training_size(d):
    """ASPP's shape at x4, B = 16, 54 x 54 LR: the sub-image batch is 64 / 144 images of 27 / 18 pixels."""
    from sradsgan_amd import ops
    n, c, h, w = 16, 256, 54, 54
    conv = torch.nn.Conv2d(c, c, 3, padding=d, dilation=d)
    with torch.no_grad():
        conv.weight.copy_(O.det_fill('dilT.w', tuple(conv.weight.shape), 0.03))
        conv.bias.copy_(O.det_fill('dilT.b', (c,), 0.1))
    x = _wide('dilT.x', n, c, h, w)
    g = _wide('dilT.g', n, c, h, w, 1e-3)
    wt = torch.nn.Parameter(conv.weight.detach().to(DEV))
    bt = torch.nn.Parameter(conv.bias.detach().to(DEV))
    xl = x.clone().requires_grad_()
    y = ops.conv2d_dil(xl, wt, bt, d)
    y.backward(g)
    torch.cuda.synchronize()
    ref = conv.double()
    x64 = x.cpu().double().requires_grad_()
    y64 = ref(x64)
    y64.backward(g.cpu().double())
    e = (rel_err(y, y64), rel_err(xl.grad, x64.grad), rel_err(wt.grad, ref.weight.grad), rel_err(bt.grad, ref.bias.grad))
    print('dilated training size d=%d: y %.2e dx %.2e dw %.2e db %.2e' % ((d,) + e))
    assert e[0] < 2e-5 and e[1] < 2e-4 and e[2] < 2e-4 and e[3] < 1e-5


def test_dilated_conv_half_mode_forward():
    """At training size: the sub-image batch (64 images of 27 x 27) is large enough for the 16-bit kernels (small grids run the
    exact-fp32 ones in every mode), so the forward really rounds its operands to fp16."""
    from sradsgan_amd import ops
    n, c, h, w, d = 16, 256, 54, 54, 2
    x = _wide('dilH.x', n, c, h, w)
    wt = torch.nn.Parameter(O.det_fill('dilH.w', (c, c, 3, 3), 0.05).to(DEV))
    b = O.det_fill('dilH.b', (c,), 0.1).to(DEV)
    with ops.conv_math('half'):
        y = ops.conv2d_dil(x, wt, b, d)
    e = rel_err(y, F.conv2d(x.cpu().double(), wt.detach().cpu().double(), b.cpu().double(), 1, d, d))
    print('dilated half mode forward: %.2e' % e)
    assert 2e-5 < e < 1.5e-3


@pytest.mark.parametrize('slope', [0.25, 0.0, -0.3])
def test_prelu_strided_against_fp64_with_shared_slope(slope):
    """Forward into a channel slice of the wide buffer; the backward of three applications sharing one slope (ASPP's act) reduced
    in one call; values exactly at 0 included."""
    from sradsgan_amd import ops, _hip
    n, c, h, w = 2, 256, 13, 14
    rows = n * h * w
    a32 = torch.tensor([slope], dtype=torch.float32)
    a = a32.to(DEV)
    zc = []
    for k in range(3):
        z = O.det_fill('pr.z%d' % k, (n, c, h, w), 1.0)
        z.view(-1)[::7] = 0.0
        zc.append(z)
    gc = [O.det_fill('pr.g%d' % k, (n, c, h, w), 1.0) for k in range(3)]
    zs = [z.to(DEV).contiguous(memory_format=CL) for z in zc]
    gs = [g.to(DEV).contiguous(memory_format=CL) for g in gc]
    parts = _hip.lib().srhip_prelu_parts()
    runs = []
    for _ in range(2):
        buf = _wide('pr.buf', n, WIDE, h, w)
        dzs, partials = [], torch.empty(3 * parts, device=DEV)
        for k in range(3):
            ops.prelu_fwd_raw(zs[k], c, buf[:, 256 * k:], WIDE, a, rows, c)
            dz = torch.empty_like(zs[k], memory_format=CL)
            ops.prelu_bwd_raw(gs[k], c, zs[k], c, dz, c, a, partials[k * parts:], rows, c)
            dzs.append(dz)
        da = torch.empty(1, device=DEV)
        ops.prelu_slope_reduce_raw(partials, da)
        torch.cuda.synchronize()
        runs.append([buf.cpu(), da.cpu()] + [t.cpu() for t in dzs])
    for p, q in zip(runs[0], runs[1]):
        assert torch.equal(p, q), 'rerun differs'
    a64 = a32.double().requires_grad_()
    da64, scale = 0.0, 0.0
    for k in range(3):
        # one fp32 multiply per element: the fp32 values are exact
        assert torch.equal(runs[0][0][:, 256 * k:256 * (k + 1)], torch.where(zc[k] > 0, zc[k], a32 * zc[k])), 'forward'
        assert torch.equal(runs[0][2 + k], torch.where(zc[k] > 0, gc[k], a32 * gc[k])), 'input gradient'
        z64 = zc[k].double().requires_grad_()
        gz, ga = torch.autograd.grad(F.prelu(z64, a64), (z64, a64), gc[k].double())
        assert torch.equal(runs[0][2 + k].double(), gz) or rel_err(runs[0][2 + k], gz) < 1e-7
        da64 = da64 + ga
        scale += float((zc[k].double().clamp(max=0) * gc[k].double()).abs().sum())
    assert abs(float(runs[0][1]) - float(da64)) <= 1e-6 * scale


def test_aspp_like_modules_match_fp64_autograd():
    """HipDilatedConv2d d = 1, 2, 3 sharing one HipPReLU, as amssrn.py:200-217 composes them, through autograd against nn modules."""
    from sradsgan_amd import ops
    from sradsgan_amd.model.layers import HipDilatedConv2d, HipPReLU
    n, c, h, w = 2, 64, 13, 14
    refs = [torch.nn.Conv2d(c, c, 3, padding=d, dilation=d) for d in (1, 2, 3)]
    act = torch.nn.PReLU()
    with torch.no_grad():
        for d, r in zip((1, 2, 3), refs):
            r.weight.copy_(O.det_fill('asp.w%d' % d, tuple(r.weight.shape), 0.05))
            r.bias.copy_(O.det_fill('asp.b%d' % d, (c,), 0.1))
        act.weight.fill_(-0.1)
    hips = [HipDilatedConv2d(c, c, 3, padding=d, dilation=d) for d in (1, 2, 3)]
    hact = HipPReLU()
    for hm, r in zip(hips, refs):
        hm.load_state_dict(r.state_dict())
        hm.to(DEV)
    hact.load_state_dict(act.state_dict())
    hact.to(DEV)
    x = O.det_fill('asp.x', (n, c, h, w), 1.0)
    g = O.det_fill('asp.g', (n, 3 * c, h, w), 1.0)
    for mode, tol in (('bf16x3', 2e-5), ('fp32', 5e-6)):
        for m in hips + [hact]:
            m.zero_grad(set_to_none=True)
        xl = x.to(DEV).contiguous(memory_format=CL).requires_grad_()
        with ops.conv_math(mode):
            y = torch.cat([hact(hm(xl)) for hm in hips], 1)
            y.backward(g.to(DEV))
        torch.cuda.synchronize()
        x64 = x.double().requires_grad_()
        r64 = [r.double() for r in refs]
        a64 = act.double()
        for m in r64 + [a64]:
            m.zero_grad(set_to_none=True)
        z64 = [r(x64) for r in r64]
        y64 = torch.cat([a64(z) for z in z64], 1)
        y64.backward(g.double())
        # scale of the slope gradient sum (z g over z <= 0): its error is relative to that, not to the (cancelling) sum
        scale = float(sum((z.detach().clamp(max=0) * gk).abs().sum() for z, gk in zip(z64, g.double().split(c, 1))))
        assert rel_err(y, y64) < tol
        assert rel_err(xl.grad, x64.grad) < 10 * tol
        for hm, r in zip(hips, r64):
            assert rel_err(hm.weight.grad, r.weight.grad) < 10 * tol and rel_err(hm.bias.grad, r.bias.grad) < 1e-5
        assert abs(float(hact.weight.grad) - float(a64.weight.grad)) <= 10 * tol * scale
