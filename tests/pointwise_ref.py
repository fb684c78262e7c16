"""References of the point-wise and pooling kernels of csrc/cbam.hip and csrc/elementwise.hip, written from the semantics that
include/sradsgan_hip.h documents (not from the kernels): fp64 where there is arithmetic, exact indexing where there is none.  Plus
the case tables and seeded input families that the GPU tests (test_cbam_gpu.py, test_elementwise_gpu.py) and the CPU check of these
references (test_pointwise_ref_cpu.py) share, the fp32 emulations of the kernels' summation orders (the CPU proof that a correct
kernel can meet the bar), and the guarded output buffers of the GPU tests.

Layouts are the kernels': cbam tensors are [n][hw][c], gate tensors [n][2][c] / [n][hw][2], pool / shuffle tensors [n][h][w][c]."""
import torch

NAN = float('nan')


# --------------------------------------------------------------------------------------------- #
# first maximum / first NaN (the rule of csrc/common.h)
# --------------------------------------------------------------------------------------------- #


def _first_where(mask, dim):
    """Index of the first True along dim (size of the dim where there is none)."""
    size = mask.shape[dim]
    shape = [1] * mask.dim()
    shape[dim] = size
    idx = torch.arange(size).view(shape).expand_as(mask)
    return torch.where(mask, idx, torch.full_like(idx, size)).amin(dim)


def first_max(x, dim):
    """(max, arg) along dim: the first maximal element in index order; a slice that holds a NaN gives (NaN, index of the first NaN).
    The value is gathered from x, so it is exact in x's own dtype."""
    nan = torch.isnan(x)
    clean = torch.where(nan, torch.full_like(x, float('-inf')), x)
    arg = _first_where(clean == clean.amax(dim, keepdim=True), dim)
    has_nan = nan.any(dim)
    arg = torch.where(has_nan, _first_where(nan, dim), arg)
    return x.gather(dim, arg.unsqueeze(dim)).squeeze(dim), arg


# --------------------------------------------------------------------------------------------- #
# cbam.hip
# --------------------------------------------------------------------------------------------- #


def pool_hw_ref(x):
    """x [n][hw][c] -> mean [n][c] (fp64), max [n][c] (x's dtype), arg [n][c] (first maximal pixel; first NaN)."""
    mx, arg = first_max(x, 1)
    return x.double().mean(1), mx, arg


def pool_c_ref(x):
    """x [n][hw][c] -> mean [n][hw] (fp64), max [n][hw], arg [n][hw] (first maximal channel; first NaN)."""
    mx, arg = first_max(x, 2)
    return x.double().mean(2), mx, arg


def repool_hw_ref(x, arg):
    """The fixed_arg form: mean and x AT the given pixel (whether or not it is the maximum)."""
    return x.double().mean(1), x.gather(1, arg.long().unsqueeze(1)).squeeze(1)


def repool_c_ref(x, arg):
    return x.double().mean(2), x.gather(2, arg.long().unsqueeze(2)).squeeze(2)


def unpool_hw_ref(t, arg, hw):
    """t [n][2][c], arg [n][c] -> out [n][hw][c] = t0 / hw + (p == arg) t1, fp64."""
    t = t.double()
    hit = torch.arange(hw).view(1, hw, 1) == arg.long().unsqueeze(1)
    return t[:, 0].unsqueeze(1) / hw + hit.double() * t[:, 1].unsqueeze(1)


def unpool_c_ref(t, argc, c):
    """t [n][hw][2], argc [n][hw] -> out [n][hw][c] = t0 / c + (ch == argc) t1, fp64."""
    t = t.double()
    hit = torch.arange(c).view(1, 1, c) == argc.long().unsqueeze(2)
    return t[..., 0].unsqueeze(2) / c + hit.double() * t[..., 1].unsqueeze(2)


def scale_ref(x, s, mode):
    """x [n][hw][c] * s, s [n][c] (mode 0) or [n][hw] (mode 1), in x's dtype: one multiply, so fp32 in gives the exact fp32 result."""
    return x * (s.unsqueeze(1) if mode == 0 else s.unsqueeze(2))


def dot_ref(a, b, mode):
    """sum over pixels (mode 0 -> [n][c]) or over channels (mode 1 -> [n][hw]) of a * b, fp64."""
    return (a.double() * b.double()).sum(1 if mode == 0 else 2)


def _sig(v):
    """1 / (1 + exp(-v)) in fp64 without overflow warnings at either end."""
    v = v.double()
    e = torch.exp(-v.abs())
    return torch.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_ref(x, pair):
    """pair: x [n][2][c] -> sigmoid(x0 + x1) [n][c]; else elementwise.  fp64."""
    x = x.double()
    return _sig(x[:, 0] + x[:, 1]) if pair else _sig(x)


def sigmoid_bwd_ref(g, y, pair):
    """dx = g y (1 - y); pair: the same value in both rows, [n][2][c]."""
    d = g.double() * y.double() * (1.0 - y.double())
    return torch.stack([d, d], 1) if pair else d


def sigmoid_bwd_bwd_ref(gg, g, y, pair):
    """For a cotangent gg on dx (pair: gg [n][2][c], summed over the two rows): dg = gg y (1 - y), dy = gg g (1 - 2 y)."""
    u = gg.double()
    if pair:
        u = u[:, 0] + u[:, 1]
    y = y.double()
    return u * y * (1.0 - y), u * g.double() * (1.0 - 2.0 * y)


# --------------------------------------------------------------------------------------------- #
# elementwise.hip
# --------------------------------------------------------------------------------------------- #


def _windows(x):
    """x [n][h][w][c] -> [4][n][h/2][w/2][c] in window scan order (0,0), (0,1), (1,0), (1,1)."""
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], 0)


def maxpool2x2_ref(x):
    """x [n][h][w][c] -> (y [n][h/2][w/2][c], pos): the window maximum and the position 0..3 of its first occurrence in scan
    order.  A window that holds a NaN gives NaN (and the first NaN's position, which only the forward relies on)."""
    return first_max(_windows(x), 0)


def maxpool2x2_bwd_ref(dy, x, relu_input):
    """dx [n][h][w][c]: dy at the first maximum of each window, 0 elsewhere; relu_input: 0 where the window maximum is not > 0."""
    y, pos = maxpool2x2_ref(x)
    g = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu_input else dy
    dx = torch.zeros_like(x)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, i::2, j::2] = torch.where(pos == k, g, torch.zeros_like(g))
    return dx


def _shuffle_index(n, h, w, cout, r):
    """Flat input index of every output element: out[b, hh r + i, ww r + j, c] <- in[b, hh, ww, c r r + i r + j]."""
    b, oh, ow, c = torch.meshgrid(torch.arange(n), torch.arange(h * r), torch.arange(w * r), torch.arange(cout), indexing='ij')
    hh, i, ww, j = oh // r, oh % r, ow // r, ow % r
    return ((b * h + hh) * w + ww) * (cout * r * r) + c * r * r + i * r + j


def _lrelu(v, slope):
    return torch.where(v > 0, v, v * torch.tensor(slope, dtype=v.dtype))


def pixel_shuffle_ref(x, r, slope=None):
    """x [n][h][w][cout r r] -> out [n][h r][w r][cout], then LeakyReLU(slope) in x's dtype when slope is not None."""
    n, h, w, cin = x.shape
    cout = cin // (r * r)
    out = x.reshape(-1)[_shuffle_index(n, h, w, cout, r)]
    return out if slope is None else _lrelu(out, slope)


def pixel_shuffle_bwd_ref(dout, out, r, slope=None):
    """din [n][h][w][cout r r]: the inverse permutation of dout, times the LeakyReLU mask of `out` (out > 0 ? 1 : slope; a zero or
    NaN takes the slope) when slope is not None."""
    n, hr, wr, cout = dout.shape
    h, w = hr // r, wr // r
    g = dout if slope is None else torch.where(out > 0, dout, dout * torch.tensor(slope, dtype=dout.dtype))
    din = torch.empty(n * h * w * cout * r * r, dtype=dout.dtype)
    din[_shuffle_index(n, h, w, cout, r).reshape(-1)] = g.reshape(-1)
    return din.view(n, h, w, cout * r * r)


def lrelu_bwd_ref(dy, y, slope):
    """y > 0 ? dy : dy * slope in fp32 -- one multiply, so a kernel must give these bits.  A NaN or zero y takes the slope."""
    dy = dy.float()
    return torch.where(y > 0, dy, dy * torch.tensor(slope, dtype=torch.float32))


def lrelu_mask_ref(y):
    """The bit mask srhip_lrelu_bwd_bits documents: one bit per element (y > 0), in chunks of 64 float4s = 256 elements; a chunk is 4
    little-endian 64-bit words, word e holds component e of its 64 float4s, bit l of it float4 l.  Returns uint8 bytes; the bits of
    elements past the count are 0."""
    n4 = y.numel() // 4
    chunks = (n4 + 63) // 64
    p = torch.zeros(chunks * 64, 4, dtype=torch.bool)
    p[:n4] = (y.reshape(-1)[:n4 * 4] > 0).view(n4, 4)
    bits = p.view(chunks, 64, 4).permute(0, 2, 1).reshape(chunks, 4, 8, 8)          # [chunk][word][byte][bit]
    weights = (2 ** torch.arange(8)).view(1, 1, 1, 8)
    return (bits.long() * weights).sum(-1).to(torch.uint8).reshape(-1)


def cat_ref(ts):
    """ts: [rows][c_k] tensors -> [rows][sum c_k], tensor k in columns q0_k .. q0_k + c_k - 1."""
    rows = ts[0].shape[0]
    out = torch.empty(rows, sum(t.shape[1] for t in ts), dtype=ts[0].dtype)
    at = 0
    for t in ts:
        out[:, at:at + t.shape[1]] = t
        at += t.shape[1]
    return out


def split_ref(wide, chans):
    out, at = [], 0
    for c in chans:
        out.append(wide[:, at:at + c].clone())
        at += c
    return out


def same_bits(a, b):
    """Bit equality of two fp32 tensors (tells -0.0 from 0.0; equal NaN payloads compare equal)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# --------------------------------------------------------------------------------------------- #
# fp32 emulations of the kernels' summation orders (CPU): what a CORRECT kernel computes
# --------------------------------------------------------------------------------------------- #


def _seq_sum(v, dim):
    """Left-to-right fp32 sum along dim, starting from 0."""
    acc = torch.zeros_like(v.select(dim, 0))
    for k in range(v.shape[dim]):
        acc = acc + v.select(dim, k)
    return acc


def _lanes4(v):
    """v [n][hw][c] fp32: four pixel lanes p = l, l + 4, ... summed left to right, then (l0 + l1) + (l2 + l3)."""
    s = [_seq_sum(v[:, l::4], 1) if v.shape[1] > l else torch.zeros_like(v[:, 0]) for l in range(4)]
    return (s[0] + s[1]) + (s[2] + s[3])


def _butterfly(lanes):
    """lanes [...][64] fp32: v += v[lane ^ o] for o = 32, 16, .., 1; lane 0's value."""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ o]
    return lanes[..., 0]


def _lanes64(quads):
    """quads [n][hw][c/4] fp32 (one partial per float4): lane l sums quads l, l + 64, ... left to right, then the butterfly."""
    n, hw, q = quads.shape
    trips = (q + 63) // 64
    pad = torch.zeros(n, hw, trips * 64, dtype=quads.dtype)
    pad[..., :q] = quads
    return _butterfly(_seq_sum(pad.view(n, hw, trips, 64), 2))


def emulate_pool_hw_mean(x):
    return _lanes4(x.float()) / torch.tensor(float(x.shape[1]))


def emulate_dot_hw(a, b):
    return _lanes4(a.float() * b.float())


def emulate_pool_c_mean(x):
    v = x.float().view(x.shape[0], x.shape[1], -1, 4)
    return _lanes64((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) / torch.tensor(float(x.shape[2]))


def emulate_dot_c(a, b):
    p = (a.float() * b.float()).view(a.shape[0], a.shape[1], -1, 4)
    return _lanes64((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))


# --------------------------------------------------------------------------------------------- #
# cbam cases and input families
# --------------------------------------------------------------------------------------------- #

CBAM_SHAPES = [
    (1, 4, 1, 1),        # hw = 1: three of four pixel lanes empty; c = 4: one live quad, 63 idle lanes in pool_c
    (2, 68, 1, 3),       # hw = 3; second 64-channel block with 4 live channels
    (3, 64, 5, 7),       # hw = 35, not a multiple of 4
    (2, 100, 9, 9),      # ragged second channel block
    (2, 256, 27, 27),    # the discriminator's own shape
    (1, 260, 4, 5),      # pool_c / dot_c: second trip of the lane loop with one quad in it
    (2, 512, 3, 3),      # two full trips
    (3, 64, 150, 150),   # 1,080,000 float4 > 4096 x 256: the grid-stride trip of scale, unpool_hw, unpool_c
]
CBAM_BIG = (3, 64, 150, 150)
AUTOGRAD_SHAPE = (2, 68, 5, 7)

# pixel pairs (first, second) of equal maxima that sit in DIFFERENT pixel lanes (p % 4), the later pixel in the EARLIER lane: a merge
# over lanes that keeps the first lane's candidate instead of the smaller index picks the wrong one
HW_TIE_PAIRS = ((1, 4), (2, 5), (3, 6), (3, 4), (2, 4), (3, 5))
C_TIE_BASE = 14          # channel pairs (14, 14 ^ (1 << bit)), bit = 2 .. 7: one per step of the 64-lane butterfly; all partners >= 6
C_TIE_QUAD = (8, 11)     # equal maxima inside one float4
HW_PLANT, C_PLANT = 2.0, 3.0


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def _gen(shape, salt):
    n, c, h, w = shape
    return torch.Generator().manual_seed(20240 + 1000003 * salt + 7 * n + 13 * c + 101 * h + 1009 * w)


def cbam_random(shape, salt=0):
    """uniform(-1, 1) + 0.25 as [n][hw][c]: the offset keeps the means away from pure cancellation."""
    n, c, h, w = shape
    return torch.rand(n, h * w, c, generator=_gen(shape, salt)) * 2 - 1 + 0.25


def cbam_ties(shape):
    """(x, expect): values on multiples of 1/4 in [-1, 1], so maxima repeat everywhere, plus planted decisive ties.  expect lists
    what the plants force: {'hw': [(image, channel, first pixel)], 'c': [(image, pixel, first channel)]}.
      image 0:      channel c-1 constant and pixel hw-1 constant (arg 0); channels 0..5 hold HW_PLANT at HW_TIE_PAIRS[k]
      image n-1:    pixels hold C_PLANT at C_TIE_QUAD (one float4) and at the butterfly pairs of C_TIE_BASE
    Plants never touch the constant row / column of their image nor one another (channels 0..5 / >= 6, pixels 1..6 / the rest)."""
    n, c, h, w = shape
    hw = h * w
    x = torch.round((torch.rand(n, hw, c, generator=_gen(shape, 1)) * 2 - 1) * 4) / 4
    x[0, :, c - 1] = 0.5
    x[0, hw - 1, :] = 0.5
    expect = {'hw': [(0, c - 1, 0)], 'c': [(0, hw - 1, 0)]}
    for k, (p1, p2) in enumerate(HW_TIE_PAIRS):
        if k < c - 1 and p2 < hw - 1:
            x[0, p1, k] = x[0, p2, k] = HW_PLANT
            expect['hw'].append((0, k, p1))
    img = n - 1
    pixels = list(range(hw)) if img > 0 else [0] + list(range(7, hw - 1))
    pairs = [C_TIE_QUAD] + [(min(C_TIE_BASE, C_TIE_BASE ^ (1 << b)), max(C_TIE_BASE, C_TIE_BASE ^ (1 << b))) for b in range(2, 8)]
    for pix, (c1, c2) in zip(pixels, [p for p in pairs if p[1] < c - 1]):
        x[img, pix, c1] = x[img, pix, c2] = C_PLANT
        expect['c'].append((img, pix, c1))
    return x, expect


def cbam_nan_variants(shape):
    """[(x, [(image, pixel, channel) of every NaN])]: the random family with ONE NaN, placed in turn at the channels 0, 1, 4, 128
    (where c allows) and c-1 and at pixels of lane residues 0..3 (where hw allows); the last variant has a NaN that shares its
    column with a second one and its row with a third (first-NaN rule along both axes)."""
    n, c, h, w = shape
    hw = h * w
    chans = sorted({ch for ch in (0, 1, 4, 128, c - 1) if ch < c})
    out = []
    for i in range(max(len(chans), 4)):
        res = i % 4
        pix = 4 + res if 4 + res < hw else (res if res < hw else hw - 1)
        out.append([(i % n, pix, chans[i % len(chans)])])
    if hw >= 2 and c >= 2:
        pa, pb, ca, cb = hw // 3, hw - 1, c // 3, c - 1
        out.append([(n - 1, pa, ca), (n - 1, pb, ca), (n - 1, pa, cb)])
    res = []
    for places in out:
        x = cbam_random(shape)
        for (b, p, ch) in places:
            x[b, p, ch] = NAN
        res.append((x, places))
    return res


def random_arg_table(shape, over, salt=5):
    """A seeded arg table that is NOT the arg-max of anything: over = 'hw' -> [n][c] pixels, 'c' -> [n][hw] channels (int32)."""
    n, c, h, w = shape
    size = (n, c) if over == 'hw' else (n, h * w)
    return torch.randint(0, h * w if over == 'hw' else c, size, generator=_gen(shape, salt)).to(torch.int32)


SIGMOID_CASES = [(n, c) for c in (1, 68, 256) for n in (1, 3)]       # counts 1 .. 768; 68, 204 are no multiples of 256
SIGMOID_SPECIALS = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, float('inf'), float('-inf'))
SIGMOID_SATURATED = {100.0: 1.0, -100.0: 0.0, float('inf'): 1.0, float('-inf'): 0.0}


def sigmoid_inputs(n, c, pair):
    """x ([n][2][c] when pair, else [n][c]) ~ 3 N(0, 1) with SIGMOID_SPECIALS at the front of the flat tensor (pair: in row 0, with a 0
    in row 1, so that no inf - inf appears), g and gg ~ N(0, 1).  Returns x, g [n][c], gg (x's shape), specials placed [(flat index
    of y, value)]."""
    gen = torch.Generator().manual_seed(4242 + 10 * c + n + 1000 * int(pair))
    x = 3 * torch.randn((n, 2, c) if pair else (n, c), generator=gen)
    placed = []
    for k, v in enumerate(SIGMOID_SPECIALS[:n * c]):
        b, ch = divmod(k, c)
        if pair:
            x[b, 0, ch], x[b, 1, ch] = v, 0.0
        else:
            x[b, ch] = v
        placed.append((k, v))
    return x, torch.randn(n, c, generator=gen), torch.randn(x.shape, generator=gen), placed


# --------------------------------------------------------------------------------------------- #
# elementwise cases and inputs
# --------------------------------------------------------------------------------------------- #

POOL_SHAPES = [(2, 4, 2, 2), (3, 12, 6, 10), (1, 64, 14, 18), (2, 8, 2, 34)]        # (n, c, h, w); 1x64x14x18: 1008 threads, ragged last block
POOL_FAMILIES = ('random', 'relu', 'ties', 'negative', 'equal')
POOL_TIE_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def pool_inputs(family, shape):
    """x [n][h][w][c], dy [n][h/2][w/2][c], z (the pre-ReLU tensor of 'relu', else None).
      random    N(0, 1)                     relu      relu(N(0, 1)): zeros, windows of zeros
      ties      uniform(0.1, 1) with 2.0 planted at one of the six position pairs of every window, in turn
      negative  -uniform(0.1, 1)            equal     one value per window, of either sign and zero"""
    n, c, h, w = shape
    gen = _gen(shape, 11 + POOL_FAMILIES.index(family))
    z = None
    if family == 'random':
        x = torch.randn(n, h, w, c, generator=gen)
    elif family == 'relu':
        z = torch.randn(n, h, w, c, generator=gen)
        z[0, :2, :2] = -z[0, :2, :2].abs()                                            # the first window of every channel: all zeros
        x = torch.relu(z)
    elif family == 'negative':
        x = -(0.1 + 0.9 * torch.rand(n, h, w, c, generator=gen))
    elif family == 'equal':
        v = torch.round(torch.randn(n, h // 2, w // 2, c, generator=gen) * 2) / 2
        x = v.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
    else:
        x = 0.1 + 0.9 * torch.rand(n, h, w, c, generator=gen)
        win = _windows(x).clone()                                                     # [4][n][ho][wo][c]
        which = torch.arange(win[0].numel()).view(win[0].shape) % 6
        for k, (a, b) in enumerate(POOL_TIE_PAIRS):
            win[a][which == k] = 2.0
            win[b][which == k] = 2.0
        x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2] = win[0], win[1], win[2], win[3]
    return x, torch.randn(n, h // 2, w // 2, c, generator=gen), z


SHUFFLE_R = (2, 3, 4)
SHUFFLE_NHW = ((1, 1, 1), (3, 5, 7), (2, 2, 9))
SHUFFLE_COUT = (4, 12, 64)
SHUFFLE_ACTS = (None, 0.01, 0.2)


def shuffle_inputs(n, h, w, cout, r, integer):
    """in [n][h][w][cout r r] and a dout [n][h r][w r][cout] that is not the forward's input.  integer: every input element is its own
    signed flat index (+-(i + 1), exact in fp32 up to 2^24), so a wrong index cannot hide; else N(0, 1) with exact zeros sprinkled
    in (a zero output takes the slope in the backward)."""
    gen = torch.Generator().manual_seed(99 + n + 10 * h + 100 * w + 1000 * cout + 7 * r)
    count = n * h * w * cout * r * r
    if integer:
        i = torch.arange(count, dtype=torch.float32) + 1
        x = torch.where(torch.arange(count) % 3 == 0, -i, i).view(n, h, w, cout * r * r)
    else:
        x = torch.randn(n, h, w, cout * r * r, generator=gen)
        x.view(-1)[::5] = 0.0
    return x, torch.randn(n, h * r, w * r, cout, generator=gen)


LRELU_COUNTS = (1, 3, 4, 105, 1023, 4194308, 4194307)      # 4,194,308: one float4 past 4096 blocks x 256; 4,194,307: that trip plus a tail
LRELU_SLOPES = (0.2, 0.0, 1.0)
LRELU_BITS_N4 = (1, 63, 64, 65, 1048577)
LRELU_Y_SPECIALS = (0.0, -0.0, NAN, float('inf'), float('-inf'), 1e-40, -1e-40, 1.401298464324817e-45)


def lrelu_inputs(count):
    """dy ~ N(0, 1) (finite), y ~ N(0, 1) with LRELU_Y_SPECIALS at the front and, mirrored, at the very end: the last three elements
    -- the scalar tail of a count with count % 4 == 3 -- are NaN, -0.0 and 0.0, where `>` and `>=` part."""
    gen = torch.Generator().manual_seed(555 + count)
    dy, y = torch.randn(count, generator=gen), torch.randn(count, generator=gen)
    sp = torch.tensor(LRELU_Y_SPECIALS)
    k = min(count, sp.numel())
    y[count - k:] = sp[:k].flip(0)
    y[:k] = sp[:k]
    return dy, y


CAT_CASES = {
    'eight_by_four': (37, [4] * 8),                  # 8 tensors of 4 channels
    'grid_stride': (65540, [8, 4, 52]),              # 65,540 rows x 16 quads = 1,048,640 > 4096 x 256: the grid-stride trip
}


def cat_inputs(rows, chans):
    gen = torch.Generator().manual_seed(rows + sum(chans))
    return [torch.randn(rows, c, generator=gen) for c in chans]


# --------------------------------------------------------------------------------------------- #
# guarded outputs of the GPU tests
# --------------------------------------------------------------------------------------------- #

BAND = 64


class Guarded:
    """An output of `shape` inside a larger allocation: BAND sentinel elements on both sides, the body pre-filled with NaN (integer
    types: -7), so that an element the kernel never wrote and an element a tail thread wrote out of bounds both show.  misalign: the
    body starts that many ELEMENTS past a 256-byte boundary (1 -> 4 bytes off a 16-byte boundary for 4-byte types)."""

    def __init__(self, shape, device, dtype=torch.float32, misalign=0):
        self.count = 1
        for s in shape:
            self.count *= int(s)
        self.floating = dtype.is_floating_point
        self.sentinel = 12345.0 if self.floating else (0x5A if dtype == torch.uint8 else 123)
        self.fill = NAN if self.floating else (0xA5 if dtype == torch.uint8 else -7)       # bytes (the LeakyReLU mask) have no -7
        self.start = BAND + misalign
        self.buf = torch.full((self.count + 2 * BAND + misalign,), self.sentinel, device=device, dtype=dtype)
        self.t = self.buf[self.start:self.start + self.count].view(*shape) if self.count else self.buf[self.start:self.start]
        self.t.fill_(self.fill)

    def ptr(self):
        return self.buf.data_ptr() + self.start * self.buf.element_size()

    def bands_intact(self):
        lo, hi = self.buf[:self.start], self.buf[self.start + self.count:]
        return bool((lo == self.sentinel).all()) and bool((hi == self.sentinel).all())

    def untouched(self):
        """Bands intact and no element of the body written."""
        body = self.buf[self.start:self.start + self.count]
        clean = bool(torch.isnan(body).all()) if self.floating else bool((body == self.fill).all())
        return clean and self.bands_intact()


# --------------------------------------------------------------------------------------------- #
# calls every entry point must refuse (host-side argument checks: no kernel runs, so the CPU test makes them with made-up
# addresses and the GPU test with real guarded buffers)
# --------------------------------------------------------------------------------------------- #


def cbam_refusals(lib, p):
    """[(label, thunk)]; p: addresses 'x', 't', 'arg', 'out', 's' (16-byte aligned, never dereferenced).  Nominal n, hw, c = 2, 3, 8."""
    n, hw, c, off = 2, 3, 8, 4
    x, t, arg, out, s = p['x'], p['t'], p['arg'], p['out'], p['s']
    bad_dims = [('c % 4 != 0', (n, hw, 6)), ('n = 0', (0, hw, c)), ('n < 0', (-1, hw, c)), ('hw = 0', (n, 0, c)), ('hw < 0', (n, -3, c)),
                ('c = 0', (n, hw, 0)), ('c < 0', (n, hw, -4))]
    calls = []

    def add(entry, label, fn):
        calls.append(('%s: %s' % (entry, label), fn))
    for label, d in bad_dims:
        add('cbam_pool_hw', label, lambda d=d: lib.srhip_cbam_pool_hw(x, t, arg, 0, *d, None))
        add('cbam_pool_hw fixed', label, lambda d=d: lib.srhip_cbam_pool_hw(x, t, arg, 1, *d, None))
        add('cbam_unpool_hw', label, lambda d=d: lib.srhip_cbam_unpool_hw(t, arg, out, *d, None))
        add('cbam_pool_c', label, lambda d=d: lib.srhip_cbam_pool_c(x, t, arg, 0, *d, None))
        add('cbam_pool_c fixed', label, lambda d=d: lib.srhip_cbam_pool_c(x, t, arg, 1, *d, None))
        add('cbam_unpool_c', label, lambda d=d: lib.srhip_cbam_unpool_c(t, arg, out, *d, None))
        for mode in (0, 1):
            add('cbam_scale mode %d' % mode, label, lambda d=d, mode=mode: lib.srhip_cbam_scale(x, s, out, *d, mode, None))
            add('cbam_dot mode %d' % mode, label, lambda d=d, mode=mode: lib.srhip_cbam_dot(x, x, t, *d, mode, None))
    d = (n, hw, c)
    for k in range(3):
        a = [x, t, arg]
        a[k] = None
        add('cbam_pool_hw', 'null tensor %d' % k, lambda a=a: lib.srhip_cbam_pool_hw(*a, 0, *d, None))
        add('cbam_pool_c', 'null tensor %d' % k, lambda a=a: lib.srhip_cbam_pool_c(*a, 0, *d, None))
        a = [t, arg, out]
        a[k] = None
        add('cbam_unpool_hw', 'null tensor %d' % k, lambda a=a: lib.srhip_cbam_unpool_hw(*a, *d, None))
        add('cbam_unpool_c', 'null tensor %d' % k, lambda a=a: lib.srhip_cbam_unpool_c(*a, *d, None))
        a = [x, s, out]
        a[k] = None
        add('cbam_scale', 'null tensor %d' % k, lambda a=a: lib.srhip_cbam_scale(*a, *d, 0, None))
        a = [x, x, t]
        a[k] = None
        add('cbam_dot', 'null tensor %d' % k, lambda a=a: lib.srhip_cbam_dot(*a, *d, 1, None))
    # the tensors each entry documents (checks) as 16-byte aligned, 4 bytes off
    for k in range(3):
        a = [t, arg, out]
        a[k] += off
        add('cbam_unpool_hw', 'tensor %d 4 bytes off' % k, lambda a=a: lib.srhip_cbam_unpool_hw(*a, *d, None))
        a = [x, s, out]
        a[k] += off
        add('cbam_scale', 'tensor %d 4 bytes off' % k, lambda a=a: lib.srhip_cbam_scale(*a, *d, 0, None))
    add('cbam_pool_c', 'x 4 bytes off', lambda: lib.srhip_cbam_pool_c(x + off, t, arg, 0, *d, None))
    add('cbam_unpool_c', 'out 4 bytes off', lambda: lib.srhip_cbam_unpool_c(t, arg, out + off, *d, None))
    add('cbam_dot', 'a 4 bytes off', lambda: lib.srhip_cbam_dot(x + off, x, t, *d, 0, None))
    add('cbam_dot', 'b 4 bytes off', lambda: lib.srhip_cbam_dot(x, x + off, t, *d, 1, None))
    for mode in (2, -1):
        add('cbam_scale', 'mode %d' % mode, lambda mode=mode: lib.srhip_cbam_scale(x, s, out, *d, mode, None))
        add('cbam_dot', 'mode %d' % mode, lambda mode=mode: lib.srhip_cbam_dot(x, x, t, *d, mode, None))
    cnt = n * c
    add('sigmoid_fwd', 'null x', lambda: lib.srhip_sigmoid_fwd(None, out, cnt, c, 0, None))
    add('sigmoid_fwd', 'null y', lambda: lib.srhip_sigmoid_fwd(x, None, cnt, c, 0, None))
    add('sigmoid_fwd', 'count = 0', lambda: lib.srhip_sigmoid_fwd(x, out, 0, c, 0, None))
    add('sigmoid_fwd', 'count < 0', lambda: lib.srhip_sigmoid_fwd(x, out, -1, c, 0, None))
    add('sigmoid_fwd', 'pair with c = 0', lambda: lib.srhip_sigmoid_fwd(x, out, cnt, 0, 1, None))
    for k in range(3):
        a = [x, s, out]
        a[k] = None
        add('sigmoid_bwd', 'null tensor %d' % k, lambda a=a: lib.srhip_sigmoid_bwd(*a, cnt, c, 0, None))
        add('sigmoid_bwd_bwd', 'null input %d' % k, lambda a=a: lib.srhip_sigmoid_bwd_bwd(a[0], a[1], x if a[2] else None, out, t, cnt, c, 0, None))
    add('sigmoid_bwd', 'count = 0', lambda: lib.srhip_sigmoid_bwd(x, s, out, 0, c, 0, None))
    add('sigmoid_bwd', 'pair with c = 0', lambda: lib.srhip_sigmoid_bwd(x, s, out, cnt, 0, 1, None))
    add('sigmoid_bwd_bwd', 'count = 0', lambda: lib.srhip_sigmoid_bwd_bwd(x, s, x, out, t, 0, c, 0, None))
    add('sigmoid_bwd_bwd', 'pair with c = 0', lambda: lib.srhip_sigmoid_bwd_bwd(x, s, x, out, t, cnt, 0, 1, None))
    return calls


def elementwise_refusals(lib, p):
    """[(label, thunk)]; p: addresses 'x', 'y', 'rec', 'out', 'mask' (16-byte aligned, never dereferenced)."""
    import ctypes
    x, y, rec, out, mask = p['x'], p['y'], p['rec'], p['out'], p['mask']
    calls = []

    def add(entry, label, fn):
        calls.append(('%s: %s' % (entry, label), fn))
    for label, d in [('odd h', (2, 3, 4, 8)), ('odd w', (2, 4, 5, 8)), ('c % 4 != 0', (2, 4, 4, 6)), ('c < 4', (2, 4, 4, 2)), ('n = 0', (0, 4, 4, 8))]:
        add('maxpool2x2_fwd', label, lambda d=d: lib.srhip_maxpool2x2_fwd(x, out, *d, None))
        add('maxpool2x2_fwd_idx', label, lambda d=d: lib.srhip_maxpool2x2_fwd_idx(x, out, rec, *d, None))
        for relu in (0, 1):
            add('maxpool2x2_bwd relu %d' % relu, label, lambda d=d, relu=relu: lib.srhip_maxpool2x2_bwd(y, x, out, *d, relu, None))
            add('maxpool2x2_bwd_idx relu %d' % relu, label, lambda d=d, relu=relu: lib.srhip_maxpool2x2_bwd_idx(y, rec, out, *d, relu, None))
    d = (2, 4, 4, 8)
    add('maxpool2x2_fwd', 'null x', lambda: lib.srhip_maxpool2x2_fwd(None, out, *d, None))
    add('maxpool2x2_fwd', 'null y', lambda: lib.srhip_maxpool2x2_fwd(x, None, *d, None))
    add('maxpool2x2_fwd_idx', 'null rec', lambda: lib.srhip_maxpool2x2_fwd_idx(x, out, None, *d, None))
    add('maxpool2x2_bwd', 'null x', lambda: lib.srhip_maxpool2x2_bwd(y, None, out, *d, 0, None))
    add('maxpool2x2_bwd_idx', 'null rec', lambda: lib.srhip_maxpool2x2_bwd_idx(y, None, out, *d, 0, None))
    add('pixel_shuffle_fwd', 'cout % 4 != 0', lambda: lib.srhip_pixel_shuffle_fwd(x, out, 1, 2, 2, 6, 2, 0.2, 1, None))
    add('pixel_shuffle_fwd', 'null in', lambda: lib.srhip_pixel_shuffle_fwd(None, out, 1, 2, 2, 4, 2, 0.2, 1, None))
    add('pixel_shuffle_fwd', 'null out', lambda: lib.srhip_pixel_shuffle_fwd(x, None, 1, 2, 2, 4, 4, 0.2, 1, None))
    add('pixel_shuffle_fwd', 'h = 0', lambda: lib.srhip_pixel_shuffle_fwd(x, out, 1, 0, 2, 4, 2, 0.2, 1, None))
    add('pixel_shuffle_fwd', 'r = 0', lambda: lib.srhip_pixel_shuffle_fwd(x, out, 1, 2, 2, 4, 0, 0.2, 1, None))
    add('pixel_shuffle_bwd', 'cout % 4 != 0', lambda: lib.srhip_pixel_shuffle_bwd(y, x, out, 1, 2, 2, 6, 2, 0.2, 1, None))
    add('pixel_shuffle_bwd', 'null dout', lambda: lib.srhip_pixel_shuffle_bwd(None, x, out, 1, 2, 2, 4, 2, 0.2, 1, None))
    add('pixel_shuffle_bwd', 'null din', lambda: lib.srhip_pixel_shuffle_bwd(y, x, None, 1, 2, 2, 4, 4, 0.2, 1, None))
    add('pixel_shuffle_bwd', 'null out with the activation on', lambda: lib.srhip_pixel_shuffle_bwd(y, None, out, 1, 2, 2, 4, 2, 0.2, 1, None))
    add('pixel_shuffle_bwd', 'w = 0', lambda: lib.srhip_pixel_shuffle_bwd(y, x, out, 1, 2, 0, 4, 2, 0.2, 1, None))
    add('lrelu_bwd', 'null dy', lambda: lib.srhip_lrelu_bwd(None, x, out, 8, 0.2, None))
    add('lrelu_bwd', 'null y', lambda: lib.srhip_lrelu_bwd(y, None, out, 8, 0.2, None))
    add('lrelu_bwd', 'null dx', lambda: lib.srhip_lrelu_bwd(y, x, None, 8, 0.2, None))
    add('lrelu_bwd', 'count < 0', lambda: lib.srhip_lrelu_bwd(y, x, out, -1, 0.2, None))
    add('lrelu_bwd_bits', 'count % 4 != 0', lambda: lib.srhip_lrelu_bwd_bits(y, x, mask, out, 6, 0.2, None))
    add('lrelu_bwd_bits', 'count < 0', lambda: lib.srhip_lrelu_bwd_bits(y, x, mask, out, -4, 0.2, None))
    add('lrelu_bwd_bits', 'null dy', lambda: lib.srhip_lrelu_bwd_bits(None, x, mask, out, 8, 0.2, None))
    add('lrelu_bwd_bits', 'null mask', lambda: lib.srhip_lrelu_bwd_bits(y, x, None, out, 8, 0.2, None))
    add('lrelu_bwd_bits', 'null dx', lambda: lib.srhip_lrelu_bwd_bits(y, x, mask, None, 8, 0.2, None))
    for k, name in enumerate(('dy', 'y', 'mask', 'dx')):
        a = [y, x, mask, out]
        a[k] += 4
        add('lrelu_bwd_bits', '%s 4 bytes off' % name, lambda a=a: lib.srhip_lrelu_bwd_bits(*a, 8, 0.2, None))
    tab = (ctypes.c_void_p * 9)(*([x] * 9))
    otab = (ctypes.c_void_p * 9)(*([out] * 9))
    fours, six = (ctypes.c_int * 9)(*([4] * 9)), (ctypes.c_int * 9)(4, 6, 4, 4, 4, 4, 4, 4, 4)
    for n, ch, label in ((1, fours, 'n = 1'), (9, fours, 'n = 9'), (2, six, 'a channel count of 6')):
        add('cat_channels', label, lambda n=n, ch=ch: lib.srhip_cat_channels(tab, ch, n, out, 3, None))
        add('split_channels', label, lambda n=n, ch=ch: lib.srhip_split_channels(x, ch, n, otab, 3, None))
    add('cat_channels', 'null out', lambda: lib.srhip_cat_channels(tab, fours, 2, None, 3, None))
    add('split_channels', 'null in', lambda: lib.srhip_split_channels(None, fours, 2, otab, 3, None))
    return calls
