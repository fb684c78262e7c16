"""References, fp32 order emulations, case tables, seeded input families, guarded device buffers and refusal lists of the kernel-level
tests of csrc/ca.hip, csrc/prelu.hip, csrc/ndsrgan.hip and csrc/amssrn.hip (test_ca_kernels_gpu.py, test_residual_kernels_gpu.py,
test_nl_quad_kernels_gpu.py), and of the CPU check of all of it (test_leaf_kernels_ref_cpu.py).

Three kinds of reference, written from what include/sradsgan_hip.h and the kernels' comments document:
  * `*_ref32`: passes that are a fixed sequence of fp32 operations per element, evaluated in that sequence in fp32 on the CPU (the
    library is built with -ffp-contract=off, so a correct kernel gives these bits); the same functions run in fp64 for the CPU check;
  * `emulate_*`: the fixed-order sums, in fp32, in the documented order -- also compared bit for bit;
  * `*_eval(inp, dtype)`: everything else, in fp64 as the reference and in fp32 as the yardstick of reduction_ref.bound.
Layouts are the kernels': CA tensors [n][hw][64], partial arrays [n][nseg][64], row tensors [rows][ch], images [n][h][w][c]."""
import torch

from tests.pointwise_ref import Guarded, _seq_sum, lrelu_inputs
from tests.reduction_ref import bound, err

F64, F32 = torch.float64, torch.float32
NAN = float('nan')
ERR_ARG = -1

CA_C, CA_SEG, CA_LANES, CA_MAXHID, CA_MAXSEG = 64, 32, 16, 16, 64
STREAM_CAP = 4096 * 256          # float4 of one grid-stride trip of ca.hip's streaming passes (stream_blocks caps the grid at 4096)
PARTS = 512                      # srhip_prelu_parts() == srhip_gamma_parts()
PARTS_TRIP = PARTS * 256         # float4 of one trip of prelu_bwd / gamma_res_bwd


def f32(v):
    return torch.tensor(v, dtype=F32)


def exact(a, b):
    """Bit equality of two fp32 tensors that tells -0.0 from 0.0; a NaN matches a NaN whatever its payload (0 * inf makes NaNs of
    different signs on different hardware)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != F32 or b.dtype != F32:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~na])


def scaled_err(got, ref, scale=None):
    """reduction_ref.err; with `scale`, max|got - ref| / max(max|ref|, scale): for an output that is zero up to rounding, measured
    against the sum of the absolute terms it is made of."""
    if scale is None:
        return err(got, ref)
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), float(scale), 1e-30)


def cancellation(terms, dim=None):
    """|sum| / sum|terms| of an fp64 tensor of terms (over `dim`, else over everything); 1 where there is nothing to cancel."""
    t = terms.double()
    s, a = (t.sum(), t.abs().sum()) if dim is None else (t.sum(dim), t.abs().sum(dim))
    return torch.where(a > 0, s.abs() / a.clamp_min(1e-300), torch.ones_like(a))


def _gen(*key):
    seed = 77003
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------- #
# ca.hip: cases
# --------------------------------------------------------------------------------------------- #

CA_HW = (1, 31, 32, 33, 1537, 2049)           # hw < 32: empty segments; 33: ragged last segment; 1537: segment length 49; 2049: 65
CA_N = (1, 3)
CA_BIG = (2, 32771)                           # 2 * 32771 * 16 float4: one grid-stride trip past the 4096-block cap; segment length 1025
CA_SHAPES = [(n, hw) for hw in CA_HW for n in CA_N] + [CA_BIG]
CA_HIDDEN = (1, 4, 5, 16)
CA_NSEG = (1, 3, 4, 5, 32, 64)                # < 4: empty lanes of ca_seg_sum; 5: one lane with a second trip; 64: the cap
CA_MLP_FAMILIES = ('mixed', 'zero_unit', 'nan')
CA_MLP_HW = 77                                # the pixel count the synthetic partial arrays stand for
CA_BIAS_COMBOS = ((False, False), (True, False), (False, True), (True, True))
CA_INDEPENDENCE_HW = (33, 1537)
BCAST_PER_IMAGE = (4, 1020, 1024, 1028)       # float4 per image: 1, 255, 256, 257
BCAST_N = (1, 2, 5)
BATCH_SUM_BIG = (2, 4194316)                  # 1,048,579 float4 per image: a second trip of three items
ADD_BCAST_BIG = (2, 2097156)                  # 2 * 524,289 = 1,048,578 float4


def seg_len(hw):
    return -(-hw // CA_SEG)


def seg_bounds(hw):
    """[(p0, p1)] of the 32 segments of ca_chan_partial_kernel; p0 == p1: empty."""
    per = seg_len(hw)
    return [(min(s * per, hw), min(s * per + per, hw)) for s in range(CA_SEG)]


def ca_inputs(n, hw):
    """u, g with a mean offset, x; an ARBITRARY gate s in (0, 1) and dmean: every kernel is called on inputs of its own."""
    gen = _gen(1, n, hw)
    return dict(u=torch.randn(n, hw, CA_C, generator=gen) + 0.25, x=torch.randn(n, hw, CA_C, generator=gen),
                g=torch.randn(n, hw, CA_C, generator=gen) + 0.25, s=0.02 + 0.96 * torch.rand(n, CA_C, generator=gen),
                dmean=0.01 * torch.randn(n, CA_C, generator=gen))


# --------------------------------------------------------------------------------------------- #
# ca.hip: references
# --------------------------------------------------------------------------------------------- #


def ca_partial_ref(a, b=None):
    """fp64 [n][32][64]: per-segment sums over the pixels of a (a * b)."""
    v = a.double() if b is None else a.double() * b.double()
    out = torch.zeros(v.shape[0], CA_SEG, v.shape[2], dtype=F64)
    for s, (p0, p1) in enumerate(seg_bounds(v.shape[1])):
        if p1 > p0:
            out[:, s] = v[:, p0:p1].sum(1)
    return out


def emulate_ca_partial(a, b=None):
    """ca_chan_partial_kernel in fp32: lane r of 16 walks p0 + r, p0 + r + 16, ... left to right from +0.0 (the 4-deep main loop
    adds its four loads in that same order), then the 16 lanes are summed in order from +0.0.  Padding with +0.0 is exact: an
    accumulator that started at +0.0 is never -0.0.  An empty segment gives +0.0."""
    v = a.float() if b is None else a.float() * b.float()
    n, hw, c = v.shape
    per = seg_len(hw)
    trips = -(-per // CA_LANES)
    pad = torch.zeros(n, CA_SEG, trips * CA_LANES, c, dtype=F32)
    for s, (p0, p1) in enumerate(seg_bounds(hw)):
        if p1 > p0:
            pad[:, s, :p1 - p0] = v[:, p0:p1]
    lanes = _seq_sum(pad.view(n, CA_SEG, trips, CA_LANES, c), 2)
    return _seq_sum(lanes, 2)


def ca_scale_res_ref32(u, s, x):
    """out = s[n,c] * u + x: one multiply, one add, in the inputs' dtype."""
    return s.unsqueeze(1) * u + x


def ca_bwd_du_ref32(g, s, dmean):
    return s.unsqueeze(1) * g + dmean.unsqueeze(1)


def add_bcast_scaled_ref32(a, b, scale):
    """out[b, i] = a[b, i] + scale * bcast[i]; a [n][per_image], b [per_image]."""
    return a + torch.tensor(scale, dtype=a.dtype) * b.unsqueeze(0)


def batch_sum_ref(g, scale):
    return scale * g.double().sum(0)


def emulate_batch_sum_scaled(g, scale):
    """images in order starting FROM image 0 (not from zero), then one multiply."""
    acc = g[0].float()
    for b in range(1, g.shape[0]):
        acc = acc + g[b].float()
    return f32(scale) * acc


def ca_mlp_inputs(family, n, hidden, nseg):
    """A synthetic partial array and an MLP.  psum > 0 so that avg lies in (0.5, 1.5); row j of fc1 and b1[j] carry the sign (-1)^j, so
    unit j is active for even j and clipped for odd j whichever biases are passed.
      zero_unit   the last unit has a zero fc1 row and b1 = 0: its pre-activation is exactly 0
      nan         a NaN in one partial of image 1 (n >= 2)"""
    gen = _gen(2, CA_MLP_FAMILIES.index(family), n, hidden, nseg)
    sign = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(hidden)])
    inp = dict(psum=(0.5 + torch.rand(n, nseg, CA_C, generator=gen)) * (CA_MLP_HW / nseg),
               fc1=sign.unsqueeze(1) * (0.02 + 0.1 * torch.rand(hidden, CA_C, generator=gen)),
               b1=sign * (0.1 + 0.2 * torch.rand(hidden, generator=gen)), fc2=0.3 * torch.randn(CA_C, hidden, generator=gen),
               b2=0.5 * torch.randn(CA_C, generator=gen), hw=CA_MLP_HW)
    if family == 'zero_unit':
        inp['fc1'][hidden - 1] = 0.0
        inp['b1'][hidden - 1] = 0.0
    if family == 'nan' and n >= 2:
        inp['psum'][1, nseg // 2, 5] = NAN
    return inp


def ca_mlp_fwd_eval(inp, dtype, use_b1=True, use_b2=True):
    """avg = sum of the partials / hw, hid = relu(fc1 avg + b1) (a NaN passes), s = sigmoid(fc2 hid + b2); plus the pre-activation."""
    psum, fc1, b1, fc2, b2 = (inp[k].to(dtype) for k in ('psum', 'fc1', 'b1', 'fc2', 'b2'))
    avg = psum.sum(1) / inp['hw']
    pre = avg @ fc1.t()
    if use_b1:
        pre = pre + b1
    hid = torch.where(pre < 0, torch.zeros_like(pre), pre)
    lin = hid @ fc2.t()
    if use_b2:
        lin = lin + b2
    return dict(avg=avg, pre=pre, hid=hid, s=torch.sigmoid(lin))


def ca_mlp_bwd_inputs(n, hidden, hw=CA_MLP_HW):
    """Inputs of srhip_ca_mlp_bwd of their own (not a forward's): part > 0 and fc2 > 0, so that dl >= 0 and dh >= 0 and no weight
    or bias gradient is a sum of cancelling terms; hid = relu(.) with an exact zero at [0][0] and a positive value at [n-1][hidden-1]."""
    gen = _gen(3, n, hidden)
    hid = torch.relu(torch.randn(n, hidden, generator=gen) + 0.3)
    hid[0, 0] = 0.0
    hid[n - 1, hidden - 1] = 0.7
    return dict(part=(0.5 + torch.rand(n, CA_SEG, CA_C, generator=gen)) * (hw / CA_SEG), avg=0.5 + torch.rand(n, CA_C, generator=gen), hid=hid,
                s=0.05 + 0.9 * torch.rand(n, CA_C, generator=gen), fc1=0.3 * torch.randn(hidden, CA_C, generator=gen),
                fc2=0.05 + 0.3 * torch.rand(CA_C, hidden, generator=gen), hw=hw)


def ca_mlp_bwd_eval(inp, dtype):
    """ds = sum of the partials, dl = ds s (1 - s), dh = [hid > 0] fc2^T dl, dmean = fc1^T dh / hw; dfc2 = dl^T hid, dfc1 = dh^T avg,
    db2 = sum_b dl, db1 = sum_b dh."""
    part, avg, hid, s, fc1, fc2 = (inp[k].to(dtype) for k in ('part', 'avg', 'hid', 's', 'fc1', 'fc2'))
    dl = part.sum(1) * s * (1 - s)
    dh = torch.where(hid > 0, dl @ fc2, torch.zeros_like(hid))
    return dict(dmean=(dh @ fc1) / inp['hw'], dl=dl, dh=dh, dfc1=dh.t() @ avg, dfc2=dl.t() @ hid, db1=dh.sum(0), db2=dl.sum(0))


def ca_wgrad_terms(inp):
    """The fp64 terms (image axis first) of dfc1, dfc2, db1, db2."""
    r = ca_mlp_bwd_eval(inp, F64)
    return dict(dfc1=r['dh'].unsqueeze(2) * inp['avg'].double().unsqueeze(1), dfc2=r['dl'].unsqueeze(2) * inp['hid'].double().unsqueeze(1),
                db1=r['dh'], db2=r['dl'])


def emulate_ca_wgrad(dl, dh, hid, avg):
    """ca_mlp_wgrad_kernel in fp32 from the dl / dh the first kernel left in the workspace: every element is the sum over the images,
    in order from +0.0, of one product."""
    dl, dh, hid, avg = dl.float(), dh.float(), hid.float(), avg.float()
    return dict(dfc2=_seq_sum(dl.unsqueeze(2) * hid.unsqueeze(1), 0), dfc1=_seq_sum(dh.unsqueeze(2) * avg.unsqueeze(1), 0),
                db2=_seq_sum(dl, 0), db1=_seq_sum(dh, 0))


def ca_chain_ref(u, x, fc1, b1, fc2, b2, gout, dtype=F64):
    """The whole block in closed form, in `dtype`: out = s * u + x and the gradients of <gout, out> at u, fc1, b1, fc2, b2."""
    u, x, fc1, b1, fc2, b2, gout = (t.to(dtype) for t in (u, x, fc1, b1, fc2, b2, gout))
    hw = u.shape[1]
    fwd = ca_mlp_fwd_eval(dict(psum=u.sum(1, keepdim=True), fc1=fc1, b1=b1, fc2=fc2, b2=b2, hw=hw), dtype)
    s = fwd['s']
    bwd = ca_mlp_bwd_eval(dict(part=(gout * u).sum(1, keepdim=True), avg=fwd['avg'], hid=fwd['hid'], s=s, fc1=fc1, fc2=fc2, hw=hw), dtype)
    return dict(out=ca_scale_res_ref32(u, s, x), s=s, du=ca_bwd_du_ref32(gout, s, bwd['dmean']), dfc1=bwd['dfc1'], dfc2=bwd['dfc2'],
                db1=bwd['db1'], db2=bwd['db2'])


# --------------------------------------------------------------------------------------------- #
# prelu.hip, gamma_res_*, ndsrgan.hip: cases
# --------------------------------------------------------------------------------------------- #

ITEM_SHAPES = {1: (1, 4), 255: (51, 20), 256: (64, 16), 257: (257, 4), 131076: (43692, 12)}       # float4 items -> (rows, ch)
ITEM_COUNTS = tuple(ITEM_SHAPES)               # 131,076 = 512 * 256 + 4: one grid-stride trip of prelu_bwd / gamma_res_bwd plus a tail
SMALL_ITEMS = (255, 256, 257)
LAYOUTS = {'dense': (0, 0), 'slice': (8, 4)}   # (ld - ch, first column): ld == ch, and a channel slice of a wider buffer
PRELU_SLOPES = (0.25, 0.0, -0.3, 1.0)
LRELU_SLOPES = (0.2, 0.0, 1.0)
REDUCE_NPARTS = (1, 255, 256, 257, 1536)
GAMMA = 0.37
SUM_MIN_RATIO = 0.1
UP_R = (2, 3)
UP_C = (4, 8, 64)
UP_NHW = ((1, 1, 1), (3, 5, 7), (2, 13, 11))


def special_rows(rows, ch):
    """(g, z) [rows][ch] of pointwise_ref.lrelu_inputs: g ~ N(0, 1) finite; z ~ N(0, 1) with 0, -0.0, NaN, +-inf and denormals at the
    front and mirrored at the very end."""
    g, z = lrelu_inputs(rows * ch)
    return g.view(rows, ch), z.view(rows, ch)


def clean_rows(rows, ch, salt=0):
    """(g, z): g ~ N(0.5, 1), z ~ N(0, 1): the slope sum sum(z <= 0 ? z g : 0) keeps |sum| >= 0.1 sum|terms|."""
    gen = _gen(4, rows, ch, salt)
    return torch.randn(rows, ch, generator=gen) + 0.5, torch.randn(rows, ch, generator=gen)


def gamma_inputs(count):
    """a, b, g flat: b, g ~ N(0.5, 1)."""
    gen = _gen(5, count)
    return torch.randn(count, generator=gen), torch.randn(count, generator=gen) + 0.5, torch.randn(count, generator=gen) + 0.5


def prelu_fwd_ref32(z, a):
    """y = z > 0 ? z : a z (zero, -0.0 and NaN take the slope), in z's dtype."""
    return torch.where(z > 0, z, torch.tensor(a, dtype=z.dtype) * z)


def prelu_bwd_ref32(g, z, a):
    return torch.where(z > 0, g, torch.tensor(a, dtype=g.dtype) * g)


def prelu_slope_terms(g, z):
    z, g = z.double(), g.double()
    return torch.where(z > 0, torch.zeros_like(z), z * g)


def prelu_slope_eval(g, z, dtype):
    z, g = z.to(dtype), g.to(dtype)
    return torch.where(z > 0, torch.zeros_like(z), z * g).sum().reshape(1)


def gamma_fwd_ref32(a, b, gamma):
    return a + torch.tensor(gamma, dtype=a.dtype) * b


def gamma_db_ref32(g, gamma):
    return torch.tensor(gamma, dtype=g.dtype) * g


def gamma_sum_eval(g, b, dtype):
    return (g.to(dtype) * b.to(dtype)).sum().reshape(1)


def scaled_res_fwd_ref32(r, c, s, alpha, beta):
    """y = r + c * alpha (c None: y = r), z = s + beta * y (s None: no z): the operation order of the kernel's comment."""
    y = r if c is None else r + c * torch.tensor(alpha, dtype=r.dtype)
    return y, (None if s is None else s + torch.tensor(beta, dtype=r.dtype) * y)


def scaled_res_bwd_ref32(dz, e, ka, kb, kc):
    """dc = ka * dz, dr[0:ch] = kb * dz (+ kc * e)."""
    k = [torch.tensor(v, dtype=dz.dtype) for v in (ka, kb, kc)]
    dr = k[1] * dz
    return k[0] * dz, (dr if e is None else dr + k[2] * e)


def lrelu_bwd_strided_ref32(dy, y, slope):
    return torch.where(y > 0, dy, dy * torch.tensor(slope, dtype=dy.dtype))


def upsample_nearest_ref(x, r):
    """x [n][h][w][c] -> [n][h r][w r][c], y[b, oy, ox] = x[b, oy // r, ox // r]."""
    return x.repeat_interleave(r, 1).repeat_interleave(r, 2)


def upsample_nearest_bwd_ref(dy, r):
    n, hr, wr, c = dy.shape
    return dy.double().view(n, hr // r, r, wr // r, r, c).sum((2, 4))


def emulate_upsample_nearest_bwd(dy, r):
    """fp32, from +0.0: rows of the r x r block in order, the columns of each row in order."""
    n, hr, wr, c = dy.shape
    v = dy.float().view(n, hr // r, r, wr // r, r, c)
    acc = torch.zeros(n, hr // r, wr // r, c, dtype=F32)
    for a in range(r):
        for e in range(r):
            acc = acc + v[:, :, a, :, e]
    return acc


def rows_inputs(rows, ch, count, salt):
    """`count` independent [rows][ch] tensors ~ N(0, 1)."""
    gen = _gen(6, rows, ch, salt)
    return [torch.randn(rows, ch, generator=gen) for _ in range(count)]


# --------------------------------------------------------------------------------------------- #
# nl_quad
# --------------------------------------------------------------------------------------------- #

NL_SHAPES = ((1, 2, 2), (2, 3, 2), (1, 2, 515), (3, 17, 31), (1, 33, 32))
NL_FAMILIES = ('unit', 'sharp', 'ascending', 'descending', 'equal')
NL_OUT = ('y', 'm', 'l', 'dtheta', 'dphi', 'dg')
NL_SHARP_SCALE = 2.5
NL_INDEPENDENCE = (3, 17, 31)


def nl_quadrants(h, w):
    h1, w1 = h // 2, w // 2
    return [(0, h1, 0, w1), (0, h1, w1, w), (h1, h, 0, w1), (h1, h, w1, w)]


def nl_inputs(family, n, h, w):
    """theta, phi, g, dy [n][h][w][8].
      unit        N(0, 1) operands: logits within about +-15
      sharp       theta and phi at scale 2.5: logits to +-100, saturated rows
      ascending   theta_i = a_i e, phi_j = b_j e with a_i > 0 and b_j rising along the key walk: the running maximum moves at every key
      descending  b_j falling: it never moves after the first key
      equal       one phi for every key: uniform rows, dtheta = 0 up to rounding"""
    gen = _gen(7, NL_FAMILIES.index(family), n, h, w)
    th, ph, g, dy = (torch.randn(n, h, w, 8, generator=gen) for _ in range(4))
    if family == 'sharp':
        th, ph = th * NL_SHARP_SCALE, ph * NL_SHARP_SCALE
    elif family in ('ascending', 'descending'):
        e = torch.tensor([1.5, -2.0, 1.0, 2.5, -1.0, 0.5, 2.0, -3.0])                 # |e|^2 = 30.75
        a = 0.5 + torch.rand(n, h, w, 1, generator=gen)
        b = torch.linspace(0.0, 1.0, h * w).view(1, h, w, 1).expand(n, h, w, 1)
        th, ph = a * e, (b if family == 'ascending' else 1.0 - b) * e
    elif family == 'equal':
        ph = torch.randn(8, generator=gen).expand(n, h, w, 8)
    return dict(theta=th.contiguous(), phi=ph.contiguous(), g=g, dy=dy)


def _quad(t, q):
    r0, r1, c0, c1 = q
    return t[:, r0:r1, c0:c1].reshape(t.shape[0], -1, t.shape[-1])


def _unquad(out, q, v):
    r0, r1, c0, c1 = q
    out[:, r0:r1, c0:c1] = v.view(v.shape[0], r1 - r0, c1 - c0, *v.shape[2:])


def nl_logits(inp):
    """fp64 logits of every quadrant: [[n][queries][keys]] x 4."""
    h, w = inp['theta'].shape[1:3]
    return [_quad(inp['theta'].double(), q) @ _quad(inp['phi'].double(), q).transpose(1, 2) for q in nl_quadrants(h, w)]


def nl_eval(inp, dtype=F64):
    """Per quadrant y = softmax(theta phi^T) g with stock torch ops in `dtype`, the row maximum m and row sum l of exp(s - m), and the
    closed-form gradients at theta, phi, g of <dy, y>."""
    th, ph, g, dy = (inp[k].to(dtype) for k in ('theta', 'phi', 'g', 'dy'))
    n, h, w, _ = th.shape
    out = {k: torch.zeros(n, h, w, 8, dtype=dtype) for k in ('y', 'dtheta', 'dphi', 'dg')}
    out.update(m=torch.zeros(n, h, w, dtype=dtype), l=torch.zeros(n, h, w, dtype=dtype))
    for q in nl_quadrants(h, w):
        t, k, v, o = _quad(th, q), _quad(ph, q), _quad(g, q), _quad(dy, q)
        s = t @ k.transpose(1, 2)
        m = s.amax(-1)
        p = torch.softmax(s, -1)
        y = p @ v
        ds = p * (o @ v.transpose(1, 2) - (o * y).sum(-1, keepdim=True))
        for name, val in (('y', y), ('dtheta', ds @ k), ('dphi', ds.transpose(1, 2) @ t), ('dg', p.transpose(1, 2) @ o), ('m', m),
                          ('l', torch.exp(s - m.unsqueeze(-1)).sum(-1))):
            _unquad(out[name], q, val)
    return out


def _dot8(a, b):
    """a[..., 0] b[..., 0] + a[..., 1] b[..., 1] + ... left to right (the kernels' dot8)."""
    s = a[..., 0] * b[..., 0]
    for c in range(1, 8):
        s = s + a[..., c] * b[..., c]
    return s


def nl_eval_online32(inp):
    """The kernels' own formulation in fp32 on the CPU: the online soft-max over the keys in walk order (rescale when a logit exceeds
    the running maximum), P = exp(s - m) / l recomputed in the backward, every sum left to right."""
    th, ph, g, dy = (inp[k].float() for k in ('theta', 'phi', 'g', 'dy'))
    n, h, w, _ = th.shape
    out = {k: torch.zeros(n, h, w, 8) for k in ('y', 'dtheta', 'dphi', 'dg')}
    out.update(m=torch.zeros(n, h, w), l=torch.zeros(n, h, w))
    for q in nl_quadrants(h, w):
        t, k, v, o = _quad(th, q), _quad(ph, q), _quad(g, q), _quad(dy, q)
        s = _dot8(t.unsqueeze(2), k.unsqueeze(1))                                     # [n][queries][keys]
        cnt = s.shape[1]
        m, l, acc = torch.full((n, cnt), float('-inf')), torch.zeros(n, cnt), torch.zeros(n, cnt, 8)
        for j in range(cnt):
            sj = s[:, :, j]
            up = sj > m
            sc = torch.where(up, torch.exp(m - sj), torch.ones_like(sj))
            l, acc, m = l * sc, acc * sc.unsqueeze(-1), torch.where(up, sj, m)
            e = torch.exp(sj - m)
            l, acc = l + e, acc + e.unsqueeze(-1) * v[:, j].unsqueeze(1)
        y = acc / l.unsqueeze(-1)
        p = torch.exp(s - m.unsqueeze(-1)) / l.unsqueeze(-1)
        ds = p * (_dot8(o.unsqueeze(2), v.unsqueeze(1)) - _dot8(o, y).unsqueeze(-1))
        dth, dph, dg = torch.zeros(n, cnt, 8), torch.zeros(n, cnt, 8), torch.zeros(n, cnt, 8)
        for j in range(cnt):
            dth = dth + ds[:, :, j].unsqueeze(-1) * k[:, j].unsqueeze(1)
            dph = dph + ds[:, j, :].unsqueeze(-1) * t[:, j].unsqueeze(1)
            dg = dg + p[:, j, :].unsqueeze(-1) * o[:, j].unsqueeze(1)
        for name, val in (('y', y), ('dtheta', dth), ('dphi', dph), ('dg', dg), ('m', m), ('l', l)):
            _unquad(out[name], q, val)
    return out


def nl_scales(family, inp):
    """{output: scale} for scaled_err.  'equal': dtheta_i = phi sum_j P_ij (dy_i . g_j - D_i) = phi (D_i - D_i) is zero in exact
    arithmetic; with 1 x 1 quadrants (h = w = 2) dy_i . g_i - D_i is, so dtheta and dphi are.  Such an output is measured against
    the largest sum of its absolute terms, sum P_ij (|dy_i . g_j| + |D_i|) |phi_j| (dphi: over i, with |theta_i|); every other
    output against its own maximum."""
    th, ph, g, dy = (inp[k].double() for k in ('theta', 'phi', 'g', 'dy'))
    single = tuple(th.shape[1:3]) == (2, 2)
    if family != 'equal' and not single:
        return {}
    worst = {'dtheta': 0.0, 'dphi': 0.0}
    for q in nl_quadrants(*th.shape[1:3]):
        t, k, v, o = _quad(th, q), _quad(ph, q), _quad(g, q), _quad(dy, q)
        p = torch.softmax(t @ k.transpose(1, 2), -1)
        terms = p * ((o @ v.transpose(1, 2)).abs() + (o * (p @ v)).sum(-1, keepdim=True).abs())
        worst['dtheta'] = max(worst['dtheta'], float((terms @ k.abs()).max()))
        worst['dphi'] = max(worst['dphi'], float((terms.transpose(1, 2) @ t.abs()).max()))
    return worst if single else {'dtheta': worst['dtheta']}


# --------------------------------------------------------------------------------------------- #
# the GPU tests' buffers and table
# --------------------------------------------------------------------------------------------- #


class Buffers:
    """Every tensor a kernel sees, each in a pointwise_ref.Guarded allocation of its own: inputs copied in, outputs NaN.  A `wide`
    tensor is a [rows][ch] channel slice starting at column `off` of a [rows][ld] allocation whose other columns stay NaN."""

    def __init__(self, device):
        self.dev, self.all, self.src, self.wide = device, {}, {}, {}

    def put(self, name, t):
        t = t.detach().to(F32).contiguous()
        g = Guarded(tuple(t.shape), self.dev)
        g.t.copy_(t)
        self.all[name], self.src[name] = g, t.clone()
        return g.ptr()

    def out(self, name, *shape, fill=None):
        g = Guarded(shape, self.dev)
        if fill is not None:
            g.t.fill_(fill)
        self.all[name] = g
        return g.ptr()

    def put_wide(self, name, t, ld, off):
        rows, ch = t.shape
        g = Guarded((rows, ld), self.dev)
        g.t[:, off:off + ch] = t.to(self.dev)
        self.all[name], self.wide[name] = g, (off, ch)
        self.src[name] = g.t.detach().cpu().clone()
        return g.ptr() + 4 * off

    def out_wide(self, name, rows, ch, ld, off):
        self.all[name], self.wide[name] = Guarded((rows, ld), self.dev), (off, ch)
        return self.all[name].ptr() + 4 * off

    def ptr(self, name):
        off = self.wide[name][0] if name in self.wide else 0
        return self.all[name].ptr() + 4 * off

    def get(self, name):
        """The tensor on the CPU (a wide one: its slice)."""
        t = self.all[name].t.detach().cpu().clone()
        if name in self.wide:
            off, ch = self.wide[name]
            t = t[:, off:off + ch].contiguous()
        return t

    def rest_untouched(self, name, lo=None, hi=None):
        """A wide tensor: every column outside [lo, hi) (default: outside its slice) is still NaN."""
        off, ch = self.wide[name]
        lo, hi = off if lo is None else lo, off + ch if hi is None else hi
        t = self.all[name].t
        return bool(torch.isnan(t[:, :lo]).all()) and bool(torch.isnan(t[:, hi:]).all())

    def broken(self):
        """Names whose sentinel bands were written, and inputs that no longer hold what was put in (NaN == NaN)."""
        bad = [k for k, g in self.all.items() if not g.bands_intact()]
        for k, t in self.src.items():
            now = self.all[k].t.detach().cpu()
            if not torch.equal(torch.nan_to_num(now, nan=-77.0), torch.nan_to_num(t.view(now.shape), nan=-77.0)):
                bad.append(k + ' (input changed)')
        return bad


def table(case):
    """tests/test_reductions_gpu._Table plus the bit-exact, guard and scaled checks of these files."""
    from tests.test_reductions_gpu import _Table

    class Table(_Table):
        def bits(self, name, got, want):
            same = exact(got, want)
            print('%-46s %-22s bit-exact: %s' % (self.case, name, same))
            if not same:
                g, w = got.detach().cpu().double(), want.detach().cpu().double()
                diff = float(torch.nan_to_num(g - w, nan=float('inf')).abs().max()) if g.shape == w.shape else NAN
                self.bad.append((name, 'bits differ', diff))

        def rerun(self, name, a, b):
            self.same_bits(name + ' rerun', torch.nan_to_num(a, nan=-77.0), torch.nan_to_num(b, nan=-77.0))

        def guards(self, *buffers):
            for b in buffers:
                bad = b.broken()
                print('%-46s %-22s bands and inputs intact: %s' % (self.case, 'guards', not bad))
                if bad:
                    self.bad.append(('guards', bad))

        def true(self, name, cond):
            print('%-46s %-22s %s' % (self.case, name, bool(cond)))
            if not cond:
                self.bad.append((name, 'does not hold'))

        def scaled(self, name, got, ref, yard, scale=None, extra=None):
            """err of got and of the fp32 yardstick(s) under scaled_err; the bar from `yard` alone, `extra` is printed only."""
            e, te = scaled_err(got, ref, scale), scaled_err(yard, ref, scale)
            b = bound(te)
            more = '' if extra is None else '  kernel-form fp32 %.3e' % scaled_err(extra, ref, scale)
            print('%-46s %-22s err %.3e  torch-fp32 %.3e  bound %.3e%s%s' % (self.case, name, e, te, b, more, '' if e <= b else '   <-- FAIL'))
            if not e <= b:
                self.bad.append((name, e, te, b))

    return Table(case)


# --------------------------------------------------------------------------------------------- #
# calls every entry point must refuse: [(label, thunk)], every one SRHIP_ERR_ARG from the host-side checks.  p: 16-byte aligned
# addresses 'a' .. 'h' of at least 4096 floats each, 'ws' with 'ws_bytes'.  The dimensions are small enough that a call which is NOT
# refused stays inside those buffers.
# --------------------------------------------------------------------------------------------- #


def ca_refusals(lib, p):
    a, b, c, d, e, f, g, h, ws = (p[k] for k in ('a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'ws'))
    n, hw, hid = 2, 3, 4
    need = lib.srhip_ca_mlp_bwd_workspace(n, hid)
    calls = []

    def add(entry, label, fn):
        calls.append(('%s: %s' % (entry, label), fn))

    def fwd(nseg=CA_SEG, ch=CA_C, hidden=hid):
        return lib.srhip_ca_mlp_fwd(a, nseg, b, c, d, e, f, n, hw, ch, hidden, None)

    def fwd_bias(nseg=CA_SEG, ch=CA_C, hidden=hid):
        return lib.srhip_ca_mlp_fwd_bias(a, nseg, b, g, c, h, d, e, f, n, hw, ch, hidden, None)

    def bwd(ch=CA_C, hidden=hid, w=ws, wb=need):
        return lib.srhip_ca_mlp_bwd(a, b, c, d, e, f, g, h, p['i'], w, wb, n, hw, ch, hidden, None)

    def bwd_bias(ch=CA_C, hidden=hid, w=ws, wb=need):
        return lib.srhip_ca_mlp_bwd_bias(a, b, c, d, e, f, g, h, p['j'], p['i'], p['k'], w, wb, n, hw, ch, hidden, None)

    add('ca_pool_sum', 'c != 64', lambda: lib.srhip_ca_pool_sum(a, b, n, hw, 60, None))
    add('ca_bwd_partial', 'c != 64', lambda: lib.srhip_ca_bwd_partial(a, b, c, n, hw, 60, None))
    add('ca_scale_res', 'c != 64', lambda: lib.srhip_ca_scale_res(a, b, c, d, n, hw, 60, None))
    add('ca_bwd_du', 'c != 64', lambda: lib.srhip_ca_bwd_du(a, b, c, d, n, hw, 60, None))
    for name, fn in (('ca_mlp_fwd', fwd), ('ca_mlp_fwd_bias', fwd_bias)):
        add(name, 'c != 64', lambda fn=fn: fn(ch=60))
        for v in (0, CA_MAXHID + 1):
            add(name, 'hidden = %d' % v, lambda fn=fn, v=v: fn(hidden=v))
        for v in (0, CA_MAXSEG + 1):
            add(name, 'nseg = %d' % v, lambda fn=fn, v=v: fn(nseg=v))
    for name, fn in (('ca_mlp_bwd', bwd), ('ca_mlp_bwd_bias', bwd_bias)):
        add(name, 'c != 64', lambda fn=fn: fn(ch=60))
        for v in (0, CA_MAXHID + 1):
            add(name, 'hidden = %d' % v, lambda fn=fn, v=v: fn(hidden=v, wb=1 << 14))
        add(name, 'null workspace', lambda fn=fn: fn(w=None))
        add(name, 'workspace 4 bytes short', lambda fn=fn: fn(wb=need - 4))
    add('ca_pool_sum', 'u 4 bytes off', lambda: lib.srhip_ca_pool_sum(a + 4, b, n, hw, CA_C, None))
    for k, nm in enumerate(('g', 'u')):
        t = [a, b]
        t[k] += 4
        add('ca_bwd_partial', '%s 4 bytes off' % nm, lambda t=t: lib.srhip_ca_bwd_partial(t[0], t[1], c, n, hw, CA_C, None))
    for k in range(4):
        t = [a, b, c, d]
        t[k] += 4
        add('ca_scale_res', 'tensor %d 4 bytes off' % k, lambda t=t: lib.srhip_ca_scale_res(*t, n, hw, CA_C, None))
        add('ca_bwd_du', 'tensor %d 4 bytes off' % k, lambda t=t: lib.srhip_ca_bwd_du(*t, n, hw, CA_C, None))
    for k in range(3):
        t = [a, b, c]
        t[k] += 4
        add('add_bcast_scaled', 'tensor %d 4 bytes off' % k, lambda t=t: lib.srhip_add_bcast_scaled(t[0], t[1], 0.5, t[2], n, 8, None))
    add('batch_sum_scaled', 'g 4 bytes off', lambda: lib.srhip_batch_sum_scaled(a + 4, 0.5, b, n, 8, None))
    add('batch_sum_scaled', 'out 4 bytes off', lambda: lib.srhip_batch_sum_scaled(a, 0.5, b + 4, n, 8, None))
    for v in (6, 0):
        add('add_bcast_scaled', 'per_image = %d' % v, lambda v=v: lib.srhip_add_bcast_scaled(a, b, 0.5, c, n, v, None))
        add('batch_sum_scaled', 'per_image = %d' % v, lambda v=v: lib.srhip_batch_sum_scaled(a, 0.5, b, n, v, None))
    return calls


def residual_refusals(lib, p):
    a, b, c, d, e = (p[k] for k in ('a', 'b', 'c', 'd', 'e'))
    rows, ch = 3, 8
    calls = []

    def add(entry, label, fn):
        calls.append(('%s: %s' % (entry, label), fn))

    def pf(z=a, ldz=ch, y=b, ldy=ch, chans=ch):
        return lib.srhip_prelu_fwd(z, ldz, y, ldy, e, rows, chans, None)

    def pb(g=a, ldg=ch, z=b, ldz=ch, dz=c, lddz=ch, chans=ch):
        return lib.srhip_prelu_bwd(g, ldg, z, ldz, dz, lddz, e, d, rows, chans, None)

    def sf(r=a, ldr=ch, cc=b, ldc=ch, s=c, lds=ch, y=d, ldy=ch, z=e, ldz=ch, chans=ch):
        return lib.srhip_scaled_res_fwd(r, ldr, cc, ldc, s, lds, 0.2, 0.2, y, ldy, z, ldz, rows, chans, None)

    def sb(dz=a, ldz=ch, ee=b, lde=ch, dc=c, ldc=ch, dr=d, ldr=16, width=12, chans=ch):
        return lib.srhip_scaled_res_bwd(dz, ldz, ee, lde, 0.2, 1.0, 0.2, dc, ldc, dr, ldr, width, rows, chans, None)

    def lb(dy=a, ldg=ch, y=b, ldy=ch, dx=c, ldx=ch, chans=ch):
        return lib.srhip_lrelu_bwd_strided(dy, ldg, y, ldy, dx, ldx, 0.2, rows, chans, None)

    # ch % 4 != 0, ld < ch, ld % 4 != 0, 4 bytes off
    add('prelu_fwd', 'ch % 4 != 0', lambda: pf(chans=6))
    add('prelu_bwd', 'ch % 4 != 0', lambda: pb(chans=6))
    add('scaled_res_fwd', 'ch % 4 != 0', lambda: sf(chans=6))
    add('scaled_res_bwd', 'ch % 4 != 0', lambda: sb(chans=6))
    add('lrelu_bwd_strided', 'ch % 4 != 0', lambda: lb(chans=6))
    for label, ld in (('ld < ch', 4), ('ld % 4 != 0', 10)):
        for k in ('ldz', 'ldy'):
            add('prelu_fwd', '%s (%s)' % (label, k), lambda k=k, ld=ld: pf(**{k: ld}))
        for k in ('ldg', 'ldz', 'lddz'):
            add('prelu_bwd', '%s (%s)' % (label, k), lambda k=k, ld=ld: pb(**{k: ld}))
        for k in ('ldr', 'ldc', 'lds', 'ldy', 'ldz'):
            add('scaled_res_fwd', '%s (%s)' % (label, k), lambda k=k, ld=ld: sf(**{k: ld}))
        for k in ('ldz', 'lde', 'ldc'):
            add('scaled_res_bwd', '%s (%s)' % (label, k), lambda k=k, ld=ld: sb(**{k: ld}))
        for k in ('ldg', 'ldy', 'ldx'):
            add('lrelu_bwd_strided', '%s (%s)' % (label, k), lambda k=k, ld=ld: lb(**{k: ld}))
    add('scaled_res_bwd', 'ldr % 4 != 0', lambda: sb(ldr=18))
    for k, base in (('z', a), ('y', b)):
        add('prelu_fwd', '%s 4 bytes off' % k, lambda k=k, base=base: pf(**{k: base + 4}))
    for k, base in (('g', a), ('z', b), ('dz', c)):
        add('prelu_bwd', '%s 4 bytes off' % k, lambda k=k, base=base: pb(**{k: base + 4}))
    for k, base in (('r', a), ('cc', b), ('s', c), ('y', d), ('z', e)):
        add('scaled_res_fwd', '%s 4 bytes off' % k, lambda k=k, base=base: sf(**{k: base + 4}))
    for k, base in (('dz', a), ('ee', b), ('dc', c), ('dr', d)):
        add('scaled_res_bwd', '%s 4 bytes off' % k, lambda k=k, base=base: sb(**{k: base + 4}))
    for k, base in (('dy', a), ('y', b), ('dx', c)):
        add('lrelu_bwd_strided', '%s 4 bytes off' % k, lambda k=k, base=base: lb(**{k: base + 4}))
    # upsample
    for r in (1, 4):
        add('upsample_nearest_fwd', 'r = %d' % r, lambda r=r: lib.srhip_upsample_nearest_fwd(a, b, 1, 2, 2, 4, r, None))
        add('upsample_nearest_bwd', 'r = %d' % r, lambda r=r: lib.srhip_upsample_nearest_bwd(a, b, 1, 2, 2, 4, r, None))
    add('upsample_nearest_fwd', 'c % 4 != 0', lambda: lib.srhip_upsample_nearest_fwd(a, b, 1, 2, 2, 6, 2, None))
    add('upsample_nearest_bwd', 'c % 4 != 0', lambda: lib.srhip_upsample_nearest_bwd(a, b, 1, 2, 2, 6, 2, None))
    add('upsample_nearest_fwd', 'x 4 bytes off', lambda: lib.srhip_upsample_nearest_fwd(a + 4, b, 1, 2, 2, 4, 2, None))
    add('upsample_nearest_fwd', 'y 4 bytes off', lambda: lib.srhip_upsample_nearest_fwd(a, b + 4, 1, 2, 2, 4, 2, None))
    add('upsample_nearest_bwd', 'dy 4 bytes off', lambda: lib.srhip_upsample_nearest_bwd(a + 4, b, 1, 2, 2, 4, 2, None))
    add('upsample_nearest_bwd', 'dx 4 bytes off', lambda: lib.srhip_upsample_nearest_bwd(a, b + 4, 1, 2, 2, 4, 2, None))
    # scaled_res NULL patterns and widths
    add('scaled_res_fwd', 'z but no s', lambda: sf(s=None))
    add('scaled_res_fwd', 'neither y nor z', lambda: sf(y=None, z=None))
    add('scaled_res_bwd', 'width < ch', lambda: sb(width=4))
    add('scaled_res_bwd', 'width > ldr', lambda: sb(width=20))
    add('scaled_res_bwd', 'dr NULL and width != ch', lambda: sb(dr=None, width=12))
    # gamma_res, slope_reduce
    add('gamma_res_fwd', 'count % 4 != 0', lambda: lib.srhip_gamma_res_fwd(a, b, e, c, 6, None))
    add('gamma_res_bwd', 'count % 4 != 0', lambda: lib.srhip_gamma_res_bwd(a, b, e, c, d, 6, None))
    for k in range(3):
        t = [a, b, c]
        t[k] += 4
        add('gamma_res_fwd', 'tensor %d 4 bytes off' % k, lambda t=t: lib.srhip_gamma_res_fwd(t[0], t[1], e, t[2], 8, None))
        add('gamma_res_bwd', 'tensor %d 4 bytes off' % k, lambda t=t: lib.srhip_gamma_res_bwd(t[0], t[1], e, t[2], d, 8, None))
    add('prelu_slope_reduce', 'nparts = 0', lambda: lib.srhip_prelu_slope_reduce(a, 0, b, 0, None))
    # row strides of aliased and of separate tensors
    add('lrelu_bwd_strided', 'separate tensors, different row strides', lambda: lb(ldg=8, ldx=12))
    add('prelu_fwd', 'in place, different row strides', lambda: pf(y=a, ldz=8, ldy=12))
    add('prelu_bwd', 'in place over z, different row strides', lambda: pb(dz=b, ldz=8, lddz=12))
    add('prelu_bwd', 'in place over g, different row strides', lambda: pb(dz=a, ldg=8, lddz=12))
    add('lrelu_bwd_strided', 'in place, different row strides', lambda: lb(dx=a, ldg=8, ldx=12))
    return calls


def nl_quad_refusals(lib, p):
    a, b, c, d, e, f, g, h, i, j = (p[k] for k in 'abcdefghij')
    calls = []

    def add(entry, label, fn):
        calls.append(('%s: %s' % (entry, label), fn))

    def fwd(t, hh=3, ww=3):                    # t: theta, phi, g, y
        return lib.srhip_nl_quad_fwd(t[0], t[1], t[2], t[3], e, 2, hh, ww, None)

    def bwd(t, hh=3, ww=3):                    # t: theta, phi, g, y, dy, dtheta, dphi, dg
        return lib.srhip_nl_quad_bwd(t[0], t[1], t[2], t[3], e, t[4], g, t[5], t[6], t[7], 2, hh, ww, None)

    for name, fn, base in (('nl_quad_fwd', fwd, (a, b, c, d)), ('nl_quad_bwd', bwd, (a, b, c, d, f, h, i, j))):
        add(name, 'h = 1', lambda fn=fn, base=base: fn(base, hh=1))
        add(name, 'w = 1', lambda fn=fn, base=base: fn(base, ww=1))
        for k in range(len(base)):
            t = list(base)
            t[k] += 4
            add(name, 'tensor %d 4 bytes off' % k, lambda fn=fn, t=t: fn(t))
    return calls


def run_refusals(lib, device, make_calls):
    """The GPU side of a refusal list: every call returns SRHIP_ERR_ARG and leaves a message, on real guarded buffers, and nothing --
    output, input stand-in, workspace or band -- is written."""
    bufs = {k: Guarded((4096,), device) for k in 'abcdefghijkl'}
    bufs['ws'] = Guarded((1 << 14,), device)
    p = {k: g.ptr() for k, g in bufs.items()}
    p['ws_bytes'] = 4 << 14
    bad = []
    for label, call in make_calls(lib, p):
        rc = call()
        msg = lib.srhip_last_error()
        print('%-70s rc %d  %s' % (label, rc, msg))
        if rc != ERR_ARG or not msg:
            bad.append((label, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(g.untouched() for g in bufs.values()), [k for k, g in bufs.items() if not g.untouched()]
