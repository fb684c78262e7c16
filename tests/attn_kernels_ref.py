"""References, case tables and refusal lists of csrc/global_attn.hip (CGAM, flash-style SGAM) and csrc/hat.hip (LayerNorm, GELU, window
attention, channel attention and HAB's combine), shared by the CPU check of these references (test_attn_kernels_ref_cpu.py) and the
GPU tests that call every entry point through the C ABI (test_global_attn_kernels_gpu.py, test_hat_kernels_gpu.py).

Every formula is plain torch with autograd, evaluated in float64 (the reference) and in float32 on the CPU (the yardstick: what a
correct fp32 implementation loses on the same inputs).  Layouts are the kernels': NHWC, i.e. [n][hw][c] tensors, qkv [n][h][w][288].

The measure is err = max|got - ref64| / max|ref64| per tensor (tests/reduction_ref.py).  A tensor whose reference is identically zero
(dq / dk of SGAM at hw = 1: one key, the soft-max is the constant 1) has no scale of its own; the case supplies the magnitude of the
terms whose difference it is (`scales`), and the CPU test asserts that nothing else uses that escape.
  bar of an fp32 kernel:          max(8 x err of the fp32 CPU evaluation, 32 * 2^-24)
  bar of the split-bf16 SGAM:     that + 2 x err of the split emulation (sgam_split_emulation) against float64
  cap:                            the bound the older tests hold for the same quantity (CAPS), except on the families built to make
                                  the fp32 reference itself lose digits (sharp / ascending / descending / amplitude x 6)."""
import torch
import torch.nn.functional as F

from tests import hat_ref as H
from tests import reduction_ref as R
from tests.conv_emulation import split_bf16
from tests.pointwise_ref import NAN

CAPS = {'sgam': (2e-5, 2e-4), 'cgam': (2e-5, 1e-4), 'hat_ln': (2e-6, 2e-6), 'hat_gelu': (2e-6, 2e-6), 'hat_attn': (1e-5, 1e-5),
        'hat_combine': (1e-5, 1e-5)}                      # (forward and saved tensors, gradients)


def err(got, ref, scale=None):
    """reduction_ref.err; scale: the denominator when the reference is identically zero."""
    ref = torch.as_tensor(ref).detach().cpu().double()
    if scale is not None and float(ref.abs().max()) == 0.0:
        got = torch.as_tensor(got).detach().cpu().double()
        return float('inf') if not bool(torch.isfinite(got).all()) else float(got.abs().max()) / scale
    return R.err(got, ref)


def bar(e32, cap=None, esplit=0.0):
    b = R.bound(e32) + 2.0 * esplit
    return b if cap is None else min(b, cap)


FORWARD = ('y', 'o', 'lse', 'att', 'out', 's', 'mz', 'mean', 'rstd')


def bars(ref, t32, family, capped=True, split=None, scales=None):
    """name -> (bar, err of the fp32 evaluation, err of the split emulation) for every tensor of the float64 result `ref`."""
    out = {}
    for name, r in ref.items():
        sc = (scales or {}).get(name)
        e32 = err(t32[name], r, sc)
        es = err(split[name], r, sc) if split is not None else 0.0
        if split is not None and name in split.get('sizes', {}):
            es = max(es, split['sizes'][name] / float(r.abs().max()))
        cap = CAPS[family][0 if name in FORWARD else 1] if capped else None
        out[name] = (bar(e32, cap, es), e32, es)
    return out


def _gen(*salt):
    seed = 77
    for s in salt:
        seed = (seed * 1000003 + int(s)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _u(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_()


def _grads(out, leaves, cot):
    return torch.autograd.grad(out, leaves, cot)


# --------------------------------------------------------------------------------------------- #
# CGAM and SGAM
# --------------------------------------------------------------------------------------------- #


def cgam_eval(inp, dtype):
    """_cgam_ref of tests/test_attention_gpu.py on x [n][hw][64]: y, att [n][64][64] (saved), dx, dgamma [1]."""
    x, gamma = _leaf(inp['x'], dtype), _leaf(inp['gamma'], dtype)
    e = x.transpose(1, 2) @ x
    e = e.max(dim=-1, keepdim=True)[0] - e
    att = torch.softmax(e, dim=-1)
    y = gamma * (x @ att.transpose(1, 2)) + x
    dx, dg = _grads(y, [x, gamma], inp['dy'].to(dtype))
    return {'y': y.detach(), 'att': att.detach(), 'dx': dx, 'dgamma': dg}


def sgam_scores(inp, dtype=torch.float64):
    return inp['q'].to(dtype) @ inp['k'].to(dtype).transpose(1, 2)


def sgam_eval(inp, dtype):
    """_sgam_ref on q, k [n][hw][8], v, x [n][hw][64]: y, o = softmax(q k^T) v, lse [n][hw], dq, dk, dv, dgamma [1]."""
    q, k, v, gamma = (_leaf(inp[name], dtype) for name in ('q', 'k', 'v', 'gamma'))
    s = q @ k.transpose(1, 2)
    o = torch.softmax(s, dim=-1) @ v
    y = gamma * o + inp['x'].to(dtype)
    dq, dk, dv, dg = _grads(y, [q, k, v, gamma], inp['dy'].to(dtype))
    return {'y': y.detach(), 'o': o.detach(), 'lse': torch.logsumexp(s.detach(), -1), 'dq': dq, 'dk': dk, 'dv': dv, 'dgamma': dg}


def _mm3(a, b):
    """a @ b with both operands split: hi.hi + hi.lo + lo.hi, summed in float64."""
    ah, al = split_bf16(a.float())
    bh, bl = split_bf16(b.float())
    return ah @ bh + ah @ bl + al @ bh


def sgam_split_emulation(inp):
    """Dense float64 attention whose five big products -- P.V, dout.V^T, P^T.dout, dS.K, dS^T.Q -- have split-bf16 operands, as the
    default kernels' have; energies, soft-max and the row dots stay float64.  The size of the split error, not its bits.

    dgamma = <dy, o> is ONE number, a sum of 16,512 and more terms of both signs that largely cancel (at the sharp family 663 of
    absolute terms leave 2.95), so its error <dy, do> under this emulation is one signed draw, not a size: a tile-by-tile emulation
    of the kernel's own order draws 1.36e-5 where this one draws 2.1e-6 from element errors of the same size (and smaller ones in
    o).  'sizes' therefore gives the root-sum-square of the terms dy * do -- the standard deviation of that sum under independent
    signs -- and bars() takes the larger of the draw and it."""
    q, k, v, x, gamma, dy = (inp[name].double() for name in ('q', 'k', 'v', 'x', 'gamma', 'dy'))
    s = q @ k.transpose(1, 2)
    p = torch.softmax(s, -1)
    o = _mm3(p, v)
    dout = gamma * dy
    dp = _mm3(dout, v.transpose(1, 2))
    dv = _mm3(p.transpose(1, 2), dout)
    ds = p * (dp - (dout * o).sum(-1, keepdim=True))
    exact_o = p @ v
    return {'y': gamma * o + x, 'o': o, 'lse': torch.logsumexp(s, -1), 'dq': _mm3(ds, k), 'dk': _mm3(ds.transpose(1, 2), q), 'dv': dv,
            'dgamma': (dy * o).sum().view(1), 'sizes': {'dgamma': float((dy * (o - exact_o)).norm())}}


SGAM_HW = (1, 31, 32, 33, 127, 128, 129, 257)             # one partial key tile, 32 k and 128 k exactly (no masked tail), +-1
SGAM_FAMILIES = ('sharp', 'ascending', 'descending')      # all at hw = 129: five key tiles, the last one holds key 128 alone
SGAM_FAMILY_HW = 129
SGAM_BIG = (18, 961)                                      # 17298 pixels > 16384: the prep kernel's second sweep, 1024 > 64 partials
SGAM_DGAMMA_HW = 129
SHARP_QUERY, SHARP_KEY, SHARP_EARLY_KEY = 3, 128, 40
SGAM_CASES = [('random', 2, hw) for hw in SGAM_HW] + [(f, 2, SGAM_FAMILY_HW) for f in SGAM_FAMILIES] + [('random',) + SGAM_BIG]


def sgam_inputs(family, n, hw):
    """random: the inputs of test_attention_gpu (q / k scale 1.5).  sharp: q / k scale 0.5, query 3 all 4.0 against key 128 all 4.0
    (score 128, the last tile) and key 40 all 2.5 (score 80, tile 1); everything else scores below 17.  ascending / descending: every
    q channel in [0.9, 1.1] and key j = 0.02 j (descending: 0.02 (hw - 1 - j)) + noise below 0.005, so the score of key j against
    EVERY query moves by at least 0.05 per key in one direction: the running maximum rises in every tile, or never after the first."""
    g = _gen(n, hw, 1 + (('random',) + SGAM_FAMILIES).index(family))
    inp = {'x': _u(g, n, hw, 64), 'v': _u(g, n, hw, 64), 'dy': _u(g, n, hw, 64), 'gamma': torch.tensor([0.6])}
    if family == 'random':
        inp['q'], inp['k'] = 1.5 * _u(g, n, hw, 8), 1.5 * _u(g, n, hw, 8)
    elif family == 'sharp':
        q, k = 0.5 * _u(g, n, hw, 8), 0.5 * _u(g, n, hw, 8)
        q[:, SHARP_QUERY], k[:, SHARP_KEY], k[:, SHARP_EARLY_KEY] = 4.0, 4.0, 2.5
        inp['q'], inp['k'] = q, k
    else:
        j = torch.arange(hw, dtype=torch.float32)
        ramp = j if family == 'ascending' else (hw - 1) - j
        inp['q'] = 1.0 + 0.1 * _u(g, n, hw, 8)
        inp['k'] = (0.02 * ramp).view(1, hw, 1) + 0.005 * _u(g, n, hw, 8)
    return inp


def sgam_scales(inp):
    """Magnitude of the terms whose difference dq / dk are: max|dP| max|k| (max|q|), dP = gamma dy v^T."""
    dp = float(((inp['gamma'].double() * inp['dy'].double()) @ inp['v'].double().transpose(1, 2)).abs().max())
    return {'dq': dp * float(inp['k'].abs().max()), 'dk': dp * float(inp['q'].abs().max())}


def tile_maxima(scores, tile=32):
    """scores [..][queries][keys] -> [..][queries][tiles]: the maximum of each key tile."""
    keys = scores.shape[-1]
    return torch.stack([scores[..., t:t + tile].amax(-1) for t in range(0, keys, tile)], -1)


CGAM_CASES = [(2, hw, 0.3) for hw in (1, 15, 16, 17, 127, 128, 129, 257)] + [(2, 729, 1.0)]      # 729 at scale 1: energies in the hundreds
CGAM_DGAMMA_HW = 129


def cgam_inputs(n, hw, scale):
    g = _gen(n, hw, 9)
    return {'x': scale * _u(g, n, hw, 64), 'dy': _u(g, n, hw, 64), 'gamma': torch.tensor([0.7])}


# --------------------------------------------------------------------------------------------- #
# HAT: window attention
# --------------------------------------------------------------------------------------------- #


def hat_table_rows(kind, ws):
    return (2 * ws - 1) ** 2 if kind == 0 else (ws + (ws + ws // 2) - 1) ** 2


def hat_attn_terms(qkv, table, kind, ws, shift):
    """attn_ref64 of tests/test_hat_gpu.py on qkv [n][h][w][288] up to the logits: (a [windows][6][nq][nk], v, geometry)."""
    n, h, w, _ = qkv.shape
    c, heads = 96, 6
    if kind == 0:
        t = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift else qkv
        tw = H.window_partition(t, ws).view(-1, ws * ws, 3 * c)
        b_, nq, _ = tw.shape
        p = tw.reshape(b_, nq, 3, heads, 16).permute(2, 0, 3, 1, 4)
        q, k, v = p[0] * 0.25, p[1], p[2]
        rpi, nk = H.rpi_sa(ws), nq
    else:
        ows = ws + ws // 2
        q = H.window_partition(qkv[..., :c].contiguous(), ws).view(-1, ws * ws, c)
        kv = F.unfold(qkv[..., c:].permute(0, 3, 1, 2), (ows, ows), stride=ws, padding=(ows - ws) // 2)
        nw = kv.shape[-1]
        kv = kv.view(n, 2, c, ows * ows, nw).permute(1, 0, 4, 3, 2).reshape(2, n * nw, ows * ows, c)
        b_, nq, _ = q.shape
        nk = ows * ows
        q = q.reshape(b_, nq, heads, 16).permute(0, 2, 1, 3) * 0.25
        k = kv[0].reshape(b_, nk, heads, 16).permute(0, 2, 1, 3)
        v = kv[1].reshape(b_, nk, heads, 16).permute(0, 2, 1, 3)
        rpi = H.rpi_oca(ws)
    a = q @ k.transpose(-2, -1) + table[rpi.view(-1)].view(nq, nk, -1).permute(2, 0, 1).unsqueeze(0)
    if kind == 0 and shift:
        m = H.shift_mask(h, w, ws, shift).to(a.dtype)
        nw = m.shape[0]
        a = (a.view(b_ // nw, nw, heads, nq, nk) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, nq, nk)
    return a, v


def _unwindow(t, kind, ws, shift, h, w):
    """[windows][nq][ch] -> [n][h][w][ch] at the original pixel positions."""
    o = H.window_reverse(t.reshape(-1, ws, ws, t.shape[-1]), ws, h, w)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if kind == 0 and shift else o


def hat_attn_eval(inp, dtype):
    """out [n][h][w][96], lse [n][h][w][6], dqkv, dtable for the cotangent inp['dout']."""
    kind, ws, shift = inp['kind'], inp['ws'], inp['shift']
    qkv, table = _leaf(inp['qkv'], dtype), _leaf(inp['table'], dtype)
    n, h, w, _ = qkv.shape
    a, v = hat_attn_terms(qkv, table, kind, ws, shift)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(a.shape[0], a.shape[2], 96)
    out = _unwindow(o, kind, ws, shift, h, w)
    lse = _unwindow(torch.logsumexp(a.detach(), -1).transpose(1, 2), kind, ws, shift, h, w)
    dqkv, dtable = _grads(out, [qkv, table], inp['dout'].to(dtype))
    return {'out': out.detach(), 'lse': lse, 'dqkv': dqkv, 'dtable': dtable}


# (label, kind, ws, shift, n, h, w, family)
HAT_ATTN_CASES = [('%s ws %d shift %d, 75 windows' % ('OCA' if kind else 'SA', ws, shift), kind, ws, shift, 3, 5 * ws, 5 * ws, 'random')
                  for ws in (8, 9) for kind, shift in ((0, 0), (0, ws // 2), (1, 0))]
HAT_ATTN_CASES += [('SA ws 8 shift 4, %d windows' % (n * (h // 8) * (w // 8)), 0, 8, 4, n, h, w, 'random')
                   for n, h, w in ((1, 64, 64), (5, 8, 104), (2, 64, 64))]
HAT_ATTN_CASES += [('SA ws 8 shift 0, 75 windows, %s' % f, 0, 8, 0, 3, 40, 40, f) for f in ('x6', 'ascending', 'descending')]
HAT_ATTN_UNCAPPED = ('x6', 'ascending', 'descending')


def hat_attn_windows(case):
    _, kind, ws, shift, n, h, w, family = case
    return n * (h // ws) * (w // ws)


def hat_attn_inputs(case):
    """random: qkv amplitude 1.5, table 0.5 (test_hat_gpu's).  x6: qkv amplitude 9, logits of tens.  ascending / descending (SA, no
    shift): q channels in [0.9, 1.1], k = 0.1 j (0.1 (63 - j)) for key slot j of its window + noise below 0.005, table 0.05: the logit
    0.25 q.k + bias of key j moves by at least 0.2 per key, so the forward's running-maximum branch fires at every key, or at none."""
    _, kind, ws, shift, n, h, w, family = case
    g = _gen(kind, ws, shift, n, h, w, len(family))
    amp = 9.0 if family == 'x6' else 1.5
    qkv = amp * _u(g, n, h, w, 288)
    table = 0.5 * _u(g, hat_table_rows(kind, ws), 6)
    if family in ('ascending', 'descending'):
        assert kind == 0 and shift == 0
        slot = (torch.arange(h) % ws).view(h, 1) * ws + (torch.arange(w) % ws).view(1, w)
        ramp = slot.float() if family == 'ascending' else (ws * ws - 1) - slot.float()
        qkv[..., :96] = 1.0 + 0.1 * _u(g, n, h, w, 96)
        qkv[..., 96:192] = (0.1 * ramp).view(1, h, w, 1) + 0.005 * _u(g, n, h, w, 96)
        table = 0.1 * table
    return {'qkv': qkv, 'table': table, 'dout': _u(g, n, h, w, 96), 'kind': kind, 'ws': ws, 'shift': shift}


# --------------------------------------------------------------------------------------------- #
# HAT: LayerNorm, GELU
# --------------------------------------------------------------------------------------------- #

LN_TOKENS = (1, 5, 323, 2048, 2049, 4099)        # tail waves; the 512-block cap at 2048; blocks that walk two and three tokens
LN_FAMILIES = ('random', 'constant_token', 'mean_1000')
LN_CASES = [(f, t) for t in LN_TOKENS for f in LN_FAMILIES]


def ln_inputs(family, tokens):
    """random: uniform(-1, 1) + 0.3.  constant_token: one token all 0.75 (variance 0: rstd = eps^-1/2).  mean_1000: 1000 + k / 8 with
    integers k in [-4, 4] that cancel in pairs within a token (shuffled), so that every token's sum, its mean (exactly 1000) and every
    x - mean are exact in fp32 in any summation order: what is left is the variance, which a two-pass kernel gets to fp32 accuracy and
    one that forms E[x^2] - E[x]^2 (x^2 ~ 1e6, ulp 0.06, for a variance of 0.1) does not.  Without that, rounding the mean alone costs
    ~1e-4 of y in ANY fp32 implementation, stock torch included, and the family could say nothing about the kernel."""
    g = _gen(tokens, 3 + LN_FAMILIES.index(family))
    x = _u(g, tokens, 96) + 0.3
    if family == 'constant_token':
        x[tokens // 2] = 0.75
    elif family == 'mean_1000':
        k = torch.randint(-4, 5, (tokens, 48), generator=g).float()
        k[:, 0] = 4.0
        k = torch.cat([k, -k], 1)
        order = torch.rand(tokens, 96, generator=g).argsort(1)
        x = 1000.0 + k.gather(1, order) / 8
    return {'x': x, 'gamma': 1.0 + 0.2 * _u(g, 96), 'beta': 0.1 * _u(g, 96), 'dy': _u(g, tokens, 96), 'dadd': _u(g, tokens, 96)}


def ln_eval(inp, dtype, with_dadd, stock=None):
    """y, mean, rstd, dx (+ dadd), dgamma, dbeta.  float64 (stock None): F.layer_norm.  float32: the definition written out,
    (x - mean) rstd gamma + beta, because stock F.layer_norm evaluates x (rstd gamma) + (beta - mean rstd gamma) on the CPU, which
    cancels at mean 1000 and would set a bar of 1e-3 there; the CPU test holds the two forms together in float64."""
    x, gamma, beta = (_leaf(inp[k], dtype) for k in ('x', 'gamma', 'beta'))
    if stock is None:
        stock = dtype == torch.float64
    if stock:
        y = F.layer_norm(x, (96,), gamma, beta, 1e-5)
    else:
        mu = x.mean(-1, keepdim=True)
        y = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * gamma + beta
    dx, dg, db = _grads(y, [x, gamma, beta], inp['dy'].to(dtype))
    xd = x.detach()
    mean = xd.mean(-1)
    rstd = 1.0 / torch.sqrt(((xd - mean.unsqueeze(-1)) ** 2).mean(-1) + 1e-5)
    return {'y': y.detach(), 'mean': mean, 'rstd': rstd, 'dx': dx + inp['dadd'].to(dtype) if with_dadd else dx, 'dgamma': dg, 'dbeta': db}


GELU_COUNTS = (4, 1028, 4194308)                 # 4194308: one float4 into the second sweep of the 4096 x 256 grid
GELU_SPECIALS = (0.0, -0.0, NAN)


def gelu_inputs(count):
    """x uniform in [-12, 12] with 0.0, -0.0 and a NaN in the last float4 (the second sweep's at 4194308), dy uniform(-1, 1)."""
    g = _gen(count, 5)
    x = 12.0 * _u(g, count)
    x[0], x[count - 1] = -12.0, 12.0
    for i, v in enumerate(GELU_SPECIALS):
        x[count - 4 + i] = v
    return {'x': x, 'dy': _u(g, count)}


def gelu_eval(inp, dtype):
    x = _leaf(inp['x'], dtype)
    y = F.gelu(x)
    (dx,) = _grads(y, [x], inp['dy'].to(dtype))
    return {'y': y.detach(), 'dx': dx}


# --------------------------------------------------------------------------------------------- #
# HAT: channel attention and combine
# --------------------------------------------------------------------------------------------- #

CA_DIMS = ((4, 1), (96, 3), (128, 16))
CA_HW = (1, 7, 8, 9, 64, 729)                    # chan_sum's 8 pixel lanes: fewer, one short, exact, one over, many trips
CA_N = (1, 3)
CA_BIG = (3, 11000, 128, 16)                     # 1,056,000 quads > 4096 x 256
CA_ZERO_UNIT = (3, 9, 96, 3)                     # n, hw, c, hid of the case whose hidden unit 0 is exactly 0
CS = 0.01


def ca_inputs(n, hw, c, hid, zero_unit=False):
    """x, a, u, g [n][hw][c]; w1 [hid][c], b1, w2 [c][hid], b2; kb [n] = 1 / 0.9 with entry n // 2 zero (a dropped path).  u and g are
    uniform(-1, 1) + 0.25 (pointwise_ref.cbam_random's offset): the channel sums of u and of g u, which everything behind the pooling
    hangs on, are then no pure cancellation -- at hidden = 1 the whole of dw1 / db1 is ONE such number times constants, and a relative
    error of a single cancelling sum measures the draw, not the kernel.  w2 carries + 0.1 for the same reason (dz = w2^T dl)."""
    gen = _gen(n, hw, c, hid, 21)
    inp = {k: _u(gen, n, hw, c) for k in ('x', 'a', 'u', 'g')}
    inp['u'] += 0.25
    inp['g'] += 0.25
    inp.update(w1=0.3 * _u(gen, hid, c), b1=0.2 + 0.1 * _u(gen, hid), w2=0.1 + 0.3 * _u(gen, c, hid), b2=0.1 * _u(gen, c))
    kb = torch.full((n,), 1 / 0.9)
    kb[n // 2] = 0.0
    inp['kb'] = kb
    if zero_unit:
        inp['w1'][0], inp['b1'][0] = 0.0, 0.0
    return inp


def ca_eval(inp, dtype, bias=True, kb=True, with_u=True):
    """test_hab_combine_with_96_channel_attention_matches_fp64's formula: s [n][c], mz [n][c + hid], out, and for the cotangent g:
    da, du, dw1, db1, dw2, db2.  with_u False: the MLP form out = x + kb a."""
    x, a, u, w1, b1, w2, b2 = (_leaf(inp[k], dtype) for k in ('x', 'a', 'u', 'w1', 'b1', 'w2', 'b2'))
    n = x.shape[0]
    kk = inp['kb'].to(dtype) if kb else torch.ones(n, dtype=dtype)
    if not with_u:
        out = x + kk.view(n, 1, 1) * a
        (da,) = _grads(out, [a], inp['g'].to(dtype))
        return {'out': out.detach(), 'da': da}
    m = u.mean(1)
    z = F.relu(F.linear(m, w1, b1 if bias else None))
    s = torch.sigmoid(F.linear(z, w2, b2 if bias else None))
    out = (x + kk.view(n, 1, 1) * a) + CS * (s.unsqueeze(1) * u)
    leaves = [a, u, w1, w2] + ([b1, b2] if bias else [])
    gr = _grads(out, leaves, inp['g'].to(dtype))
    res = {'s': s.detach(), 'mz': torch.cat([m, z], 1).detach(), 'out': out.detach(), 'da': gr[0], 'du': gr[1], 'dw1': gr[2], 'dw2': gr[3]}
    if bias:
        res['db1'], res['db2'] = gr[4], gr[5]
    return res


# --------------------------------------------------------------------------------------------- #
# calls every entry point must refuse on the host (no kernel runs: the CPU test makes them with made-up addresses)
# --------------------------------------------------------------------------------------------- #

ERR_ARG, ERR_WORKSPACE = -1, -3


def _variants(names, args, required, aligned):
    """[(label, args')] with each required tensor NULL and each aligned tensor 4 bytes off."""
    out = []
    for k in required:
        b = dict(args)
        b[k] = None
        out.append(('null %s' % k, b))
    for k in aligned:
        b = dict(args)
        b[k] = args[k] + 4
        out.append(('%s 4 bytes off' % k, b))
    return out


def global_attn_refusals(lib, p):
    """[(label, expected code, thunk)]; p: 16-byte aligned addresses 'a' .. 'l' and 'ws' (with 'ws_bytes' behind it)."""
    n, hw = 2, 33
    calls = []

    def add(entry, label, fn, code=ERR_ARG):
        calls.append(('%s: %s' % (entry, label), code, fn))
    need_c = lib.srhip_cgam_workspace(n, hw)
    need_s = lib.srhip_sgam_flash_bwd_workspace(n, hw)
    assert 0 < need_c <= p['ws_bytes'] and 0 < need_s <= p['ws_bytes']

    def cgam_fwd(t, ws=p['ws'], wb=need_c, d=(n, hw, 64)):
        return lib.srhip_cgam_fwd(t['x'], t['gamma'], t['y'], t['att'], ws, wb, *d, None)

    def cgam_bwd(t, ws=p['ws'], wb=need_c, d=(n, hw, 64)):
        return lib.srhip_cgam_bwd(t['dy'], t['x'], t['att'], t['gamma'], t['dx'], t['dgamma'], 0, ws, wb, *d, None)

    def sgam_fwd(t, ws=None, wb=0, d=(n, hw, 8, 64)):
        return lib.srhip_sgam_flash_fwd(t['q'], t['k'], t['v'], t['x'], t['gamma'], t['y'], t['o'], t['lse'], *d, None)

    def sgam_bwd(t, ws=p['ws'], wb=need_s, d=(n, hw, 8, 64)):
        return lib.srhip_sgam_flash_bwd(t['dy'], t['q'], t['k'], t['v'], t['o'], t['lse'], t['gamma'], t['dq'], t['dk'], t['dv'], t['dgamma'],
                                        0, ws, wb, *d, None)
    table = [
        ('cgam_fwd', cgam_fwd, dict(x=p['a'], gamma=p['b'], y=p['c'], att=p['d']), ('x', 'gamma', 'y', 'att'), ('x', 'y', 'att'), need_c, 3),
        ('cgam_bwd', cgam_bwd, dict(dy=p['a'], x=p['b'], att=p['c'], gamma=p['d'], dx=p['e'], dgamma=p['f']),
         ('dy', 'x', 'att', 'gamma', 'dx'), ('dy', 'x', 'att', 'dx'), need_c, 3),
        ('sgam_flash_fwd', sgam_fwd, dict(q=p['a'], k=p['b'], v=p['c'], x=p['d'], gamma=p['e'], y=p['f'], o=p['g'], lse=p['h']),
         ('q', 'k', 'v', 'x', 'gamma', 'y', 'o', 'lse'), ('q', 'k', 'v', 'x', 'y', 'o'), None, 4),
        ('sgam_flash_bwd', sgam_bwd, dict(dy=p['a'], q=p['b'], k=p['c'], v=p['d'], o=p['e'], lse=p['f'], gamma=p['g'], dq=p['h'], dk=p['i'],
                                           dv=p['j'], dgamma=p['k']),
         ('dy', 'q', 'k', 'v', 'o', 'lse', 'gamma', 'dq', 'dk', 'dv'), ('dy', 'q', 'k', 'v', 'o', 'dq', 'dk', 'dv'), need_s, 4),
    ]
    for entry, fn, args, required, aligned, need, nd in table:
        for label, b in _variants(entry, args, required, aligned):
            add(entry, label, lambda fn=fn, b=b: fn(b))
        full = (n, hw, 64) if nd == 3 else (n, hw, 8, 64)
        dims = [('C = 32', full[:-1] + (32,)), ('C = 128', full[:-1] + (128,)), ('n = 0', (0,) + full[1:]), ('n < 0', (-1,) + full[1:]),
                ('hw = 0', (n, 0) + full[2:]), ('hw < 0', (n, -5) + full[2:])]
        if nd == 4:
            dims += [('q/k width 4', (n, hw, 4, 64)), ('q/k width 16', (n, hw, 16, 64))]
        for label, d in dims:
            add(entry, label, lambda fn=fn, args=args, d=d: fn(args, d=d))
        if need is not None:
            add(entry, 'null workspace', lambda fn=fn, args=args, need=need: fn(args, ws=None, wb=need), ERR_WORKSPACE)
            add(entry, 'workspace one element short', lambda fn=fn, args=args, need=need: fn(args, wb=need - 4), ERR_WORKSPACE)
        if entry.startswith('cgam'):                  # its partial tiles are read as float4
            add(entry, 'workspace 4 bytes off', lambda fn=fn, args=args: fn(args, ws=p['ws'] + 4))
    return calls


def hat_refusals(lib, p):
    """[(label, expected code, thunk)]; p as in global_attn_refusals."""
    calls = []

    def add(entry, label, fn, code=ERR_ARG):
        calls.append(('%s: %s' % (entry, label), code, fn))
    A = [p[k] for k in 'abcdefghijkl']
    tokens = 8

    def ln_fwd(t, tk=tokens):
        return lib.srhip_hat_ln_fwd(t['x'], t['gamma'], t['beta'], t['y'], t['mean'], t['rstd'], tk, None)

    def ln_bwd(t, tk=tokens):
        return lib.srhip_hat_ln_bwd(t['dy'], t['x'], t['gamma'], t['mean'], t['rstd'], t['dadd'], t['dx'], t['part'], t['dgamma'], t['dbeta'],
                                    tk, None)
    a = dict(zip(('x', 'gamma', 'beta', 'y', 'mean', 'rstd'), A))
    for label, b in _variants('', a, a.keys(), ()):
        add('hat_ln_fwd', label, lambda b=b: ln_fwd(b))
    a2 = dict(zip(('dy', 'x', 'gamma', 'mean', 'rstd', 'dadd', 'dx', 'part', 'dgamma', 'dbeta'), A))
    for label, b in _variants('', a2, ('dy', 'x', 'gamma', 'mean', 'rstd', 'dx', 'part'), ()):
        add('hat_ln_bwd', label, lambda b=b: ln_bwd(b))
    for tk in (0, -4):
        add('hat_ln_fwd', 'tokens = %d' % tk, lambda tk=tk: ln_fwd(a, tk))
        add('hat_ln_bwd', 'tokens = %d' % tk, lambda tk=tk: ln_bwd(a2, tk))

    def gelu_fwd(t, cnt=8):
        return lib.srhip_hat_gelu_fwd(t['x'], t['y'], cnt, None)

    def gelu_bwd(t, cnt=8):
        return lib.srhip_hat_gelu_bwd(t['dy'], t['x'], t['dx'], cnt, None)
    g1, g2 = dict(zip(('x', 'y'), A)), dict(zip(('dy', 'x', 'dx'), A))
    for entry, fn, args in (('hat_gelu_fwd', gelu_fwd, g1), ('hat_gelu_bwd', gelu_bwd, g2)):
        for label, b in _variants('', args, args.keys(), args.keys()):
            add(entry, label, lambda fn=fn, b=b: fn(b))
        for cnt in (6, 1, 0, -4):
            add(entry, 'count = %d' % cnt, lambda fn=fn, args=args, cnt=cnt: fn(args, cnt))

    geo = dict(kind=0, n=2, h=16, w=16, ws=8, shift=4)
    need_a = lib.srhip_hat_attn_bwd_workspace(0, 2, 16, 16, 8)
    assert 0 < need_a <= p['ws_bytes']

    def attn_fwd(t, wsp=None, wb=0, **kw):
        d = dict(geo, **kw)
        return lib.srhip_hat_attn_fwd(t['qkv'], t['table'], t['out'], t['lse'], d['kind'], d['n'], d['h'], d['w'], d['ws'], d['shift'], None)

    def attn_bwd(t, wsp=p['ws'], wb=need_a, **kw):
        d = dict(geo, **kw)
        return lib.srhip_hat_attn_bwd(t['qkv'], t['table'], t['out'], t['dout'], t['lse'], t['dqkv'], t['dtable'], wsp, wb, d['kind'], d['n'],
                                      d['h'], d['w'], d['ws'], d['shift'], None)
    f1 = dict(zip(('qkv', 'table', 'out', 'lse'), A))
    f2 = dict(zip(('qkv', 'table', 'out', 'dout', 'lse', 'dqkv', 'dtable'), A))
    bad_geo = [('kind 2', dict(kind=2)), ('window 7', dict(ws=7, h=14, w=14, shift=0)), ('window 10', dict(ws=10, h=20, w=20, shift=0)),
               ('window 0', dict(ws=0, shift=0)), ('h not a multiple of the window', dict(h=20)), ('w not a multiple of the window', dict(w=12)),
               ('window 9 on 16 x 16', dict(ws=9, shift=0)), ('shift 3', dict(shift=3)), ('shift 8', dict(shift=8)), ('shift -4', dict(shift=-4)),
               ('OCA with a shift', dict(kind=1, shift=4)), ('n = 0', dict(n=0)), ('n < 0', dict(n=-2)), ('h = 0', dict(h=0)), ('w = 0', dict(w=0))]
    for entry, fn, args in (('hat_attn_fwd', attn_fwd, f1), ('hat_attn_bwd', attn_bwd, f2)):
        for label, b in _variants('', args, args.keys(), ('qkv',)):
            add(entry, label, lambda fn=fn, b=b: fn(b))
        for label, kw in bad_geo:
            add(entry, label, lambda fn=fn, args=args, kw=kw: fn(args, **kw))
    add('hat_attn_bwd', 'workspace 4 bytes off', lambda: attn_bwd(f2, wsp=p['ws'] + 4))
    add('hat_attn_bwd', 'null workspace', lambda: attn_bwd(f2, wsp=None), ERR_WORKSPACE)
    add('hat_attn_bwd', 'workspace one element short', lambda: attn_bwd(f2, wb=need_a - 4), ERR_WORKSPACE)
    need_o = lib.srhip_hat_attn_bwd_workspace(1, 2, 16, 16, 8)
    assert need_a < need_o <= p['ws_bytes']
    add('hat_attn_bwd', 'OCA workspace one element short', lambda: attn_bwd(f2, wb=need_o - 4, kind=1, shift=0), ERR_WORKSPACE)

    n, hw, c, hid = 2, 9, 8, 2
    need_k = lib.srhip_hat_combine_bwd_workspace(n, c, hid)
    assert 0 < need_k <= p['ws_bytes']

    def ca_fwd(t, d=(n, hw, c, hid)):
        return lib.srhip_hat_ca_fwd(t['u'], t['w1'], t['b1'], t['w2'], t['b2'], t['s'], t['mz'], *d, None)

    def cmb_fwd(t, d=(n, hw, c)):
        return lib.srhip_hat_combine_fwd(t['x'], t['a'], t['kb'], t['u'], t['s'], t['out'], CS, *d, None)

    def cmb_bwd(t, ws=p['ws'], wb=need_k, d=(n, hw, c, hid)):
        return lib.srhip_hat_combine_bwd(t['g'], t['kb'], t['u'], t['s'], t['mz'], t['w1'], t['w2'], t['da'], t['du'], t['dw1'], t['db1'],
                                         t['dw2'], t['db2'], ws, wb, CS, *d, None)
    c1 = dict(zip(('u', 'w1', 'b1', 'w2', 'b2', 's', 'mz'), A))
    c2 = dict(zip(('x', 'a', 'kb', 'u', 's', 'out'), A))
    c3 = dict(zip(('g', 'kb', 'u', 's', 'mz', 'w1', 'w2', 'da', 'du', 'dw1', 'db1', 'dw2'), A), db2=p['ws'] + 4096)
    for label, b in _variants('', c1, ('u', 'w1', 'w2', 's', 'mz'), ('u',)):
        add('hat_ca_fwd', label, lambda b=b: ca_fwd(b))
    for label, d in [('C = 132', (n, hw, 132, hid)), ('C = 6', (n, hw, 6, hid)), ('C = 0', (n, hw, 0, hid)), ('hidden = 17', (n, hw, c, 17)),
                     ('hidden = 0', (n, hw, c, 0)), ('n = 0', (0, hw, c, hid)), ('hw = 0', (n, 0, c, hid)), ('hw < 0', (n, -9, c, hid))]:
        add('hat_ca_fwd', label, lambda d=d: ca_fwd(c1, d))
        add('hat_combine_bwd', label, lambda d=d: cmb_bwd(c3, d=d))
    for label, b in _variants('', c2, ('x', 'a', 'out'), ('x', 'a', 'u', 's', 'out')):
        add('hat_combine_fwd', label, lambda b=b: cmb_fwd(b))
    add('hat_combine_fwd', 'u without s', lambda: cmb_fwd(dict(c2, s=None)))
    for label, d in [('C = 6', (n, hw, 6)), ('C = 0', (n, hw, 0)), ('n = 0', (0, hw, c)), ('hw = 0', (n, 0, c))]:
        add('hat_combine_fwd', label, lambda d=d: cmb_fwd(c2, d))
    for label, b in _variants('', c3, ('g', 'u', 's', 'mz', 'w1', 'w2'), ('g', 'u', 's', 'da', 'du')):
        add('hat_combine_bwd', label, lambda b=b: cmb_bwd(b))
    add('hat_combine_bwd', 'workspace 4 bytes off', lambda: cmb_bwd(c3, ws=p['ws'] + 4))
    add('hat_combine_bwd', 'null workspace', lambda: cmb_bwd(c3, ws=None), ERR_WORKSPACE)
    add('hat_combine_bwd', 'workspace one element short', lambda: cmb_bwd(c3, wb=need_k - 4), ERR_WORKSPACE)
    for label, d in [('C = 6 without du', (n, hw, 6, hid)), ('n = 0 without du', (0, hw, c, hid))]:
        add('hat_combine_bwd', label, lambda d=d: cmb_bwd(dict(c3, du=None), d=d))
    return calls


# --------------------------------------------------------------------------------------------- #
# the GPU tests' protocol: every tensor a kernel sees is a Guarded (tests/pointwise_ref.py)
# --------------------------------------------------------------------------------------------- #


class Buffers:
    """The guarded tensors of one call sequence: inputs copied into guarded bodies (a read past the end picks up the sentinel
    12345.0), outputs and workspaces NaN-filled, the workspace exactly as large as the library asks."""

    def __init__(self, device):
        from tests.pointwise_ref import Guarded
        self._G, self.device, self.all = Guarded, device, {}

    def put(self, name, t):
        g = self._G(tuple(t.shape), self.device)
        g.t.copy_(t)
        self.all[name] = g
        return g.ptr()

    def out(self, name, *shape):
        self.all[name] = self._G(shape, self.device)
        return self.all[name].ptr()

    def workspace(self, name, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        return self.out(name, nbytes // 4)

    def ptr(self, name):
        return self.all[name].ptr()

    def get(self, name):
        return self.all[name].t.detach().cpu().clone()

    def broken_bands(self):
        return [k for k, g in self.all.items() if not g.bands_intact()]


class Table:
    """Collects the checks of one test: prints every figure before anything is asserted, asserts in done().  worst: the largest
    err / bar seen, for the docstrings."""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], 0.0

    def check(self, name, got, ref, b, scale=None, e32=None):
        e = err(got, ref, scale)
        self.worst = max(self.worst, e / b)
        print('%-52s %-8s err %.3e  bar %.3e  err/bar %.3f%s%s' % (self.case, name, e, b, e / b, '' if e32 is None else '  fp32 %.3e' % e32,
                                                                   '' if e <= b else '   <-- FAIL'))
        if not e <= b:
            self.bad.append((name, e, b))

    def check_all(self, got, ref, table, scales=None, names=None):
        for name in (names or ref.keys()):
            self.check(name, got[name], ref[name], table[name][0], (scales or {}).get(name), table[name][1])

    def same_bits(self, name, a, b):
        from tests.pointwise_ref import same_bits
        same = same_bits(a, b)
        print('%-52s %-8s bit-identical: %s' % (self.case, name, same))
        if not same:
            self.bad.append((name, 'bits differ'))

    def require(self, ok, what):
        if not ok:
            print('%-52s %s   <-- FAIL' % (self.case, what))
            self.bad.append(what)

    def buffers(self, bufs, outputs):
        """bands of every tensor intact; no NaN left in the outputs named"""
        self.require(not bufs.broken_bands(), 'sentinel band overwritten: %s' % bufs.broken_bands())
        for name in outputs:
            self.require(not bool(torch.isnan(bufs.all[name].t).any()), 'NaN left in %s' % name)

    def rerun(self, first, second, outputs):
        for name in outputs:
            self.same_bits('rerun ' + name, first.get(name), second.get(name))

    def done(self):
        print('%-52s worst err/bar %.3f' % (self.case, self.worst))
        assert not self.bad, (self.case, self.bad)
