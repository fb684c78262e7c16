"""fp64 reference (plain torch, no kernels) of the fused attention tail of every RAB / ResGroup -- csrc/attn_tail.hip:
    s = sigmoid(fc2 relu(fc1 avg) + fc2 relu(fc1 mx))        avg, mx: mean / max of u over the pixels of a channel          (CLAM)
    y = s u,  pooled = (mean_c y, max_c y),  m = sigmoid(conv7x7(pooled, pad 3)),  z = m y                                  (SLAM)
and of its backward in closed form, the stock-torch formulation that serves as the error yardstick of the GPU tests, the margin
reporters that prove an input is not within rounding of an arg-max or ReLU flip, and the input generators.

Nothing here depends on how torch breaks a tie: every arg-max is written out as `the first index that attains the maximum`, and the
backward takes the indices as arguments -- the caller passes what it observed, like bn_bwd_ref's mask.

u, dz, z, du: [n, 64, h, w];  fc1 [hidden, 64];  fc2 [64, hidden];  w7 [1, 2, 7, 7] (any shape with those element counts);
avg, mx, s, arg: [n, 64];  pooled [n, hw, 2];  argc, m: [n, hw];  a pixel's index is y * w + x."""
import torch
import torch.nn.functional as F

C = 64
POOL_SEGMENTS = 32          # segments per image of the stand-alone pooling pass (srhip_clam_pool_segments(); the GPU test asserts it)

CHANNEL_MARGIN = 1e-4       # what every GPU case must show in the fp64 reference (test_attn_tail_ref_cpu.py asserts it for all of them)
PIXEL_MARGIN = 1e-4
RELU_MARGIN = 1e-3


def first_argmax(x, dim):
    """Index of the FIRST element along dim that attains the maximum (int64)."""
    top = x.amax(dim, keepdim=True)
    shape = [1] * x.dim()
    shape[dim] = x.shape[dim]
    idx = torch.arange(x.shape[dim]).view(shape)
    return torch.where(x == top, idx, x.shape[dim]).amin(dim)


def _mats(fc1, fc2, w7):
    fc1 = fc1.detach().double().reshape(-1, C)
    return fc1, fc2.detach().double().reshape(C, fc1.shape[0]), w7.detach().double().reshape(2, 7, 7)


def _scale(avg, mx, fc1, fc2):
    return torch.sigmoid(torch.relu(avg @ fc1.t()) @ fc2.t() + torch.relu(mx @ fc1.t()) @ fc2.t())


def _conv7(p, w7):
    """p [n, 2, h, w], w7 [2, 7, 7] -> [n, h, w]: cross-correlation with zero padding 3, tap by tap."""
    n, _, h, w = p.shape
    pp = F.pad(p, (3, 3, 3, 3))
    out = torch.zeros(n, h, w, dtype=p.dtype)
    for kh in range(7):
        for kw in range(7):
            out += (w7[:, kh, kw].view(1, 2, 1, 1) * pp[:, :, kh:kh + h, kw:kw + w]).sum(1)
    return out


def tail_fwd_ref(u, fc1, fc2, w7):
    """Returns a dict of fp64 tensors avg, mx, s, pooled, m, z and int64 arg (first max pixel of a channel), argc (first max channel
    of s u at a pixel)."""
    fc1, fc2, w7 = _mats(fc1, fc2, w7)
    n, c, h, w = u.shape
    assert c == C
    uf = u.detach().double().reshape(n, c, h * w)
    avg, mx, arg = uf.mean(2), uf.amax(2), first_argmax(uf, 2)
    s = _scale(avg, mx, fc1, fc2)
    y = s[:, :, None] * uf
    pooled = torch.stack([y.mean(1), y.amax(1)], 2)                        # [n, hw, 2]
    argc = first_argmax(y, 1)
    m = torch.sigmoid(_conv7(pooled.permute(0, 2, 1).reshape(n, 2, h, w), w7)).reshape(n, h * w)
    z = (m[:, None, :] * y).reshape(n, c, h, w)
    return dict(avg=avg, mx=mx, arg=arg, s=s, pooled=pooled, argc=argc, m=m, z=z)


def tail_bwd_parts(dz, u, fc1, fc2, w7, arg=None, argc=None):
    """The backward in closed form, fp64, the two max pools differentiated at the given indices (default: the reference's own first
    arg-maxes).  Returns a dict: du, dfc1 [hidden, 64], dfc2 [64, hidden], dw7 [2, 7, 7] and the intermediates the stand-alone entry
    points hand over -- du_spatial (s dy), ds, davg, dmax, dpooled [n, hw, 2] (the gradient at the pooled map)."""
    f = tail_fwd_ref(u, fc1, fc2, w7)
    fc1, fc2, w7 = _mats(fc1, fc2, w7)
    n, c, h, w = u.shape
    hw = h * w
    arg = f['arg'] if arg is None else arg.detach().cpu().long().reshape(n, c)
    argc = f['argc'] if argc is None else argc.detach().cpu().long().reshape(n, hw)
    uf, g = u.detach().double().reshape(n, c, hw), dz.detach().double().reshape(n, c, hw)
    s, m, avg, mx = f['s'], f['m'], f['avg'], f['mx']
    y = s[:, :, None] * uf
    # z = m y: the gate m = sigmoid(a), a = conv7(pooled)
    da = (g * y).sum(1) * m * (1 - m)                                      # [n, hw]
    dap = F.pad(da.reshape(n, h, w), (3, 3, 3, 3))
    pp = F.pad(f['pooled'].permute(0, 2, 1).reshape(n, 2, h, w), (3, 3, 3, 3))
    dpooled = torch.zeros(n, 2, h, w, dtype=torch.float64)
    dw7 = torch.zeros(2, 7, 7, dtype=torch.float64)
    for kh in range(7):
        for kw in range(7):
            dpooled += w7[:, kh, kw].view(1, 2, 1, 1) * dap[:, None, 6 - kh:6 - kh + h, 6 - kw:6 - kw + w]
            dw7[:, kh, kw] = (dap[:, None, 3:3 + h, 3:3 + w] * pp[:, :, kh:kh + h, kw:kw + w]).sum((0, 2, 3))
    dpooled = dpooled.reshape(n, 2, hw)
    onehot_c = torch.zeros(n, c, hw, dtype=torch.float64).scatter_(1, argc[:, None, :], 1.0)
    dy = m[:, None, :] * g + dpooled[:, 0:1] / c + onehot_c * dpooled[:, 1:2]
    du_spatial = s[:, :, None] * dy
    ds = (dy * uf).sum(2)                                                   # [n, 64]
    # s = sigmoid(l), l = fc2 (relu(fc1 avg) + relu(fc1 mx))
    dl = ds * s * (1 - s)
    xa, xm = avg @ fc1.t(), mx @ fc1.t()                                    # [n, hidden]
    dh = dl @ fc2
    dpa, dpm = dh * (xa > 0), dh * (xm > 0)
    dfc2 = dl.t() @ (torch.relu(xa) + torch.relu(xm))
    dfc1 = dpa.t() @ avg + dpm.t() @ mx
    davg, dmax = dpa @ fc1, dpm @ fc1
    onehot_p = torch.zeros(n, c, hw, dtype=torch.float64).scatter_(2, arg[:, :, None], 1.0)
    du = du_spatial + davg[:, :, None] / hw + onehot_p * dmax[:, :, None]
    return dict(du=du.reshape(n, c, h, w), dfc1=dfc1, dfc2=dfc2, dw7=dw7, du_spatial=du_spatial.reshape(n, c, h, w), ds=ds, davg=davg,
                dmax=dmax, dpooled=dpooled.permute(0, 2, 1))


def tail_bwd_ref(dz, u, fc1, fc2, w7, arg=None, argc=None):
    """du, dfc1, dfc2, dw7 (fp64) for the gradient dz at z; arg / argc: the arg-max indices as the caller observed them."""
    p = tail_bwd_parts(dz, u, fc1, fc2, w7, arg, argc)
    return p['du'], p['dfc1'], p['dfc2'], p['dw7']


def tail_torch(u, fc1, fc2, w7, dz=None, dtype=torch.float32, arg=None, argc=None):
    """The straightforward stock-torch formulation in `dtype` under autograd: F.adaptive_avg_pool2d / F.adaptive_max_pool2d, mean
    and max over dim 1, F.conv2d.  With arg / argc the two maxima are gathered at those indices instead (same values when they are
    the arg-maxes, and the gradient goes where the caller says).  fp32: the yardstick of the GPU tests; fp64 without indices: the
    check of the closed forms.  Returns a dict avg, mx, s, pooled, m, z (+ du, dfc1, dfc2, dw7 when dz is given)."""
    n, c, h, w = u.shape
    hw = h * w
    hid = fc1.numel() // C
    uu = u.detach().to(dtype).contiguous().requires_grad_()
    a1 = fc1.detach().to(dtype).reshape(hid, C, 1, 1).requires_grad_()
    a2 = fc2.detach().to(dtype).reshape(C, hid, 1, 1).requires_grad_()
    k7 = w7.detach().to(dtype).reshape(1, 2, 7, 7).requires_grad_()
    avg = F.adaptive_avg_pool2d(uu, 1)
    if arg is None:
        mx = F.adaptive_max_pool2d(uu, 1)
    else:
        mx = uu.reshape(n, c, hw).gather(2, arg.detach().cpu().long().reshape(n, c, 1)).reshape(n, c, 1, 1)
    mlp = lambda t: F.conv2d(F.relu(F.conv2d(t, a1)), a2)
    s = torch.sigmoid(mlp(avg) + mlp(mx))
    y = s * uu
    if argc is None:
        ymax = y.max(1, keepdim=True)[0]
    else:
        ymax = y.gather(1, argc.detach().cpu().long().reshape(n, 1, h, w))
    pooled = torch.cat([y.mean(1, keepdim=True), ymax], 1)
    m = torch.sigmoid(F.conv2d(pooled, k7, padding=3))
    z = m * y
    out = dict(avg=avg.reshape(n, c), mx=mx.reshape(n, c), s=s.reshape(n, c), pooled=pooled.reshape(n, 2, hw).permute(0, 2, 1),
               m=m.reshape(n, hw), z=z)
    if dz is not None:
        du, d1, d2, d7 = torch.autograd.grad(z, [uu, a1, a2, k7], dz.detach().to(dtype))
        out.update(du=du, dfc1=d1.reshape(hid, C), dfc2=d2.reshape(C, hid), dw7=d7.reshape(2, 7, 7))
    return {k: v.detach() for k, v in out.items()}


# --------------------------------------------------------------------------------------------- #
# the whole tail: out = conv1x1(z, wc) + bc + skip
# --------------------------------------------------------------------------------------------- #

E2E_NAMES = ('out', 'du', 'dskip', 'dfc1', 'dfc2', 'dw7', 'dwc', 'dbc')


def e2e_ref(t, arg=None, argc=None):
    """fp64: tail_fwd_ref / tail_bwd_ref composed with an fp64 1x1 conv.  t: tail_inputs(); g = the gradient at out."""
    f = tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    wc, g = t['wc'].double().reshape(C, C), t['g'].double()
    out = torch.einsum('oc,bchw->bohw', wc, f['z']) + t['bc'].double().view(1, C, 1, 1) + t['skip'].double()
    dz = torch.einsum('oc,bohw->bchw', wc, g)
    du, dfc1, dfc2, dw7 = tail_bwd_ref(dz, t['u'], t['fc1'], t['fc2'], t['w7'], arg, argc)
    return dict(out=out, du=du, dskip=g, dfc1=dfc1, dfc2=dfc2, dw7=dw7, dwc=torch.einsum('bohw,bchw->oc', g, f['z']), dbc=g.sum((0, 2, 3)))


def e2e_torch32(t, arg, argc, conv_fwd=None, conv_dgrad=None, conv_wgrad=None):
    """The yardstick of the end-to-end check: tail_torch in fp32 around a 1x1 conv.  conv_* None: stock fp32 torch; else the three
    contractions of the conv as callables returning what the kernel's arithmetic computes (tests/conv_emulation.py's split-bf16
    emulation), laid out as the kernels use them: the conv's input operand is y = s u, the gate m multiplies its result."""
    f = tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], None, torch.float32, arg, argc)
    n, c, h, w = t['u'].shape
    wc, g = t['wc'].float().reshape(C, C, 1, 1), t['g'].float()
    y = f['s'].reshape(n, c, 1, 1) * t['u'].float()
    m = f['m'].reshape(n, 1, h, w)
    conv_fwd = conv_fwd or (lambda x, k: F.conv2d(x, k))
    conv_dgrad = conv_dgrad or (lambda d, k: F.conv_transpose2d(d, k))
    conv_wgrad = conv_wgrad or (lambda x, d: torch.einsum('bohw,bchw->oc', d, x).reshape(C, C, 1, 1))
    out = conv_fwd(y, wc).float() * m + t['bc'].float().view(1, C, 1, 1) + t['skip'].float()
    dz = conv_dgrad(g, wc).float()
    b = tail_torch(t['u'], t['fc1'], t['fc2'], t['w7'], dz, torch.float32, arg, argc)
    return dict(out=out, du=b['du'], dskip=g, dfc1=b['dfc1'], dfc2=b['dfc2'], dw7=b['dw7'],
                dwc=conv_wgrad(f['z'], g).float().reshape(C, C), dbc=g.sum((0, 2, 3)))


# --------------------------------------------------------------------------------------------- #
# margins: how far an input is from an arg-max or ReLU decision that fp32 rounding could flip
# --------------------------------------------------------------------------------------------- #


def _top2_gap(x, dim):
    """(largest - second largest) / max(|largest|, |second|) along dim; inf where there is no finite second value."""
    if x.shape[dim] < 2:
        return torch.full(x.amax(dim).shape, float('inf'), dtype=torch.float64)
    t = x.topk(2, dim).values
    a, b = t.select(dim, 0), t.select(dim, 1)
    gap = (a - b) / torch.maximum(a.abs(), b.abs()).clamp_min(1e-300)
    return torch.where(torch.isfinite(b), gap, torch.full_like(gap, float('inf')))


def channel_margin(u, fc1, fc2, exempt=None):
    """[n, hw]: per pixel, the relative gap between the two largest s u over the channels.  exempt: bool [n, 64, hw], elements left
    out (the constructed, bit-exact ties of a tie family)."""
    fc1, fc2, _ = _mats(fc1, fc2, torch.zeros(98))
    n, c, h, w = u.shape
    uf = u.detach().double().reshape(n, c, h * w)
    y = _scale(uf.mean(2), uf.amax(2), fc1, fc2)[:, :, None] * uf
    if exempt is not None:
        y = y.masked_fill(exempt, float('-inf'))
    return _top2_gap(y, 1)


def pixel_margin(u, exempt=None):
    """[n, 64]: per channel, the relative gap between its two largest values over the pixels."""
    n, c, h, w = u.shape
    uf = u.detach().double().reshape(n, c, h * w)
    if exempt is not None:
        uf = uf.masked_fill(exempt, float('-inf'))
    return _top2_gap(uf, 2)


def relu_margin(u, fc1, fc2=None):
    """[2, n, hidden]: |fc1 avg| and |fc1 mx| of every hidden unit relative to the row's sum |w x|."""
    fc1 = fc1.detach().double().reshape(-1, C)
    n, c, h, w = u.shape
    uf = u.detach().double().reshape(n, c, h * w)
    out = []
    for x in (uf.mean(2), uf.amax(2)):
        out.append((x @ fc1.t()).abs() / (x.abs() @ fc1.abs().t()).clamp_min(1e-300))
    return torch.stack(out)


def margins(t):
    """(channel, pixel, relu) minima of one tail_inputs() case, the constructed ties exempt."""
    return (float(channel_margin(t['u'], t['fc1'], t['fc2'], t['exempt_c']).min()), float(pixel_margin(t['u'], t['exempt_p']).min()),
            float(relu_margin(t['u'], t['fc1']).min()))


def assert_margins(t, what=''):
    cm, pm, rm = margins(t)
    assert cm > CHANNEL_MARGIN and pm > PIXEL_MARGIN and rm > RELU_MARGIN, \
        '%s: input too close to a flip: channel %.3g (> %g), pixel %.3g (> %g), relu %.3g (> %g)' % (
            what, cm, CHANNEL_MARGIN, pm, PIXEL_MARGIN, rm, RELU_MARGIN)


# --------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------- #

FAMILIES = ('normal', 'late_max', 'all_negative', 'pixel_ties', 'channel_ties')
CONST_C, CONST_VALUE = 5, 0.625          # pixel_ties: the constant channel (every pixel ties: pixel 0 must win)
TIE_C = 9                                # pixel_ties: the channel whose maximum occurs at two pixels of different pooling segments
CHANNEL_TIES = ((3, 40), (17, 18))       # channel_ties: (c1, c2) pairs, c2 a bit-exact copy of c1; lanes far apart / the same lane


def tie_pixels(hw):
    """The two pixels of pixel_ties' TIE_C maximum: the first in pooling segment 1, the second in segment 20 -- which another lane
    of the segment merge (20 % 4 = 0) meets BEFORE the lane of segment 1 delivers the first."""
    per = (hw + POOL_SEGMENTS - 1) // POOL_SEGMENTS
    p1, p2 = per + min(1, per - 1), 20 * per + min(2, per - 1)
    assert p1 < p2 < hw and p1 // per != p2 // per
    return p1, p2


def tail_inputs(family, n, h, w, hidden=4, seed=0):
    """fp32 inputs of one case, all drawn from a CPU generator: u, fc1, fc2, w7, dz (the gradient at z); for the whole tail wc, bc,
    skip, g (the gradient at out); pre_w7 / pre_fc1 / pre_fc2 (what the accumulating calls find in their outputs); exempt_p /
    exempt_c (bool [n, 64, hw]: the constructed ties, left out of pixel_margin / channel_margin).
      normal         N(0, 1)
      late_max       every channel's maximum sits in the last pixel (the last one of the last pooling segment)
      all_negative   every element <= -1: the -inf a maximum starts from must not leak
      pixel_ties     channel CONST_C constant; channel TIE_C's maximum at the two pixels tie_pixels(hw), bit-equal
      channel_ties   for (c1, c2) in CHANNEL_TIES: u, the fc1 column and the fc2 row of c2 are copies of c1's, so s u is bit-equal in
                     any arithmetic"""
    hw = h * w
    g = torch.Generator().manual_seed(100003 * seed + 7919 * FAMILIES.index(family) + 131 * hidden + 17 * n + 1009 * h + w)
    r = lambda *shape: torch.randn(*shape, generator=g)
    u = r(n, C, h, w)
    fc1, fc2, w7 = 0.3 * r(hidden, C), 0.3 * r(C, hidden), 0.2 * r(1, 2, 7, 7)
    t = dict(dz=r(n, C, h, w), wc=0.1 * r(C, C, 1, 1), bc=0.1 * r(C), skip=r(n, C, h, w), g=r(n, C, h, w), pre_w7=r(1, 2, 7, 7),
             pre_fc1=r(hidden, C), pre_fc2=r(C, hidden))
    exempt_p = torch.zeros(n, C, hw, dtype=torch.bool)
    exempt_c = torch.zeros(n, C, hw, dtype=torch.bool)
    uf = u.view(n, C, hw)
    if family == 'late_max':
        uf[:, :, hw - 1] = uf.amax(2) + 0.5 + torch.rand(n, C, generator=g)
    elif family == 'all_negative':
        u.clamp_(max=4.0).sub_(5.0)
    elif family == 'pixel_ties':
        p1, p2 = tie_pixels(hw)
        uf[:, CONST_C, :] = CONST_VALUE
        exempt_p[:, CONST_C, 1:] = True
        top = uf[:, TIE_C, :].amax(1) + 1.5
        uf[:, TIE_C, p1] = top
        uf[:, TIE_C, p2] = top
        exempt_p[:, TIE_C, p2] = True
    elif family == 'channel_ties':
        for c1, c2 in CHANNEL_TIES:
            uf[:, c2, :] = uf[:, c1, :]
            fc1[:, c2] = fc1[:, c1]
            fc2[c2, :] = fc2[c1, :]
            exempt_c[:, c2, :] = True
    t.update(u=u, fc1=fc1, fc2=fc2, w7=w7, exempt_p=exempt_p, exempt_c=exempt_c, family=family, hidden=hidden)
    return t


# --------------------------------------------------------------------------------------------- #
# the cases of tests/test_attn_tail_gpu.py: (family, n, h, w, hidden) -> seed.  The seeds are chosen so that the fp64 reference
# alone shows the margins above (tests/test_attn_tail_ref_cpu.py asserts it for every entry); a case that is not listed is an error.
# --------------------------------------------------------------------------------------------- #

SHAPES = [(1, 1, 1),         # 31 empty pooling segments, 47 empty backward blocks, the halo entirely outside the image
          (2, 3, 5),         # hw < 16: one partial 16-pixel group, W < 7
          (3, 10, 12),       # the oracle tests' shape, n not a power of two
          (2, 5, 70),        # W > 64
          (2, 13, 70),       # strips of 8 rows with a ragged last strip
          (1, 33, 35),       # 37 pixels per segment: the unrolled 8-load loop and its scalar tail
          (2, 54, 54),       # the benchmark tile
          (1, 4, 430)]       # the wide-image fallback of the backward (dynamic LDS > 60 KB)
WIDEST_FUSED = (1, 4, 422)   # the last width on the other side of that threshold: dynamic LDS = 60 KB exactly, 64 KB with the static part
TIE_SHAPES = [(3, 10, 12), (1, 33, 35)]
HIDDEN_SHAPE, HIDDENS = (3, 10, 12), (1, 5, 16)
ACC_SHAPES = STANDALONE_SHAPES = [(3, 10, 12), (2, 13, 70)]
PLANE_SHAPES = [(2, 13, 70), (2, 54, 54)]
E2E_SHAPES = [(2, 13, 70), (1, 33, 35)]
EVAL_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 13, 70), (1, 4, 430)]

MAIN_CASES = [(f, n, h, w, 4) for (n, h, w) in SHAPES for f in FAMILIES[:3]] + [(f, n, h, w, 4) for (n, h, w) in TIE_SHAPES for f in FAMILIES[3:]]
HIDDEN_CASES = [('normal',) + HIDDEN_SHAPE + (hid,) for hid in HIDDENS]
ALL_CASES = MAIN_CASES + HIDDEN_CASES + [('normal',) + WIDEST_FUSED + (4,)]        # every other test re-uses the 'normal' case of its shape

SEEDS = {                                   # minima in the fp64 reference: channel, pixel, relu margin
    ('normal', 1, 1, 1, 4): 0,              # 0.14 inf 0.063
    ('late_max', 1, 1, 1, 4): 0,            # 0.14 inf 0.015
    ('all_negative', 1, 1, 1, 4): 0,        # 0.77 inf 0.008
    ('normal', 2, 3, 5, 4): 0,              # 0.019 0.0014 0.0072
    ('late_max', 2, 3, 5, 4): 0,            # 0.006 0.19 0.016
    ('all_negative', 2, 3, 5, 4): 1,        # 0.28 0.00078 0.085
    ('normal', 3, 10, 12, 4): 0,            # 0.0021 0.001 0.018
    ('late_max', 3, 10, 12, 4): 1,          # 0.0006 0.15 0.051
    ('all_negative', 3, 10, 12, 4): 1,      # 0.79 0.00068 0.033
    ('normal', 2, 5, 70, 4): 15,            # 0.00044 0.00087 0.0059
    ('late_max', 2, 5, 70, 4): 0,           # 0.00063 0.13 0.022
    ('all_negative', 2, 5, 70, 4): 1,       # 0.76 0.0024 0.0065
    ('normal', 2, 13, 70, 4): 0,            # 0.00057 0.00059 0.0068
    ('late_max', 2, 13, 70, 4): 2,          # 0.00032 0.12 0.021
    ('all_negative', 2, 13, 70, 4): 0,      # 0.77 0.0012 0.032
    ('normal', 1, 33, 35, 4): 1,            # 0.00069 0.00058 0.042
    ('late_max', 1, 33, 35, 4): 4,          # 0.001 0.13 0.076
    ('all_negative', 1, 33, 35, 4): 0,      # 0.0022 0.0053 0.028
    ('normal', 2, 54, 54, 4): 17,           # 0.00023 0.0012 0.018   (5832 pixels: one seed in a few hundred clears 2e-4)
    ('late_max', 2, 54, 54, 4): 322,        # 0.00039 0.13 0.0086
    ('all_negative', 2, 54, 54, 4): 0,      # 0.93 0.0013 0.039
    ('normal', 1, 4, 430, 4): 0,            # 0.00063 0.00062 0.0053
    ('late_max', 1, 4, 430, 4): 4,          # 0.00031 0.13 0.044
    ('all_negative', 1, 4, 430, 4): 1,      # 0.0014 0.0029 0.016
    ('pixel_ties', 3, 10, 12, 4): 2,        # 0.00039 0.00092 0.012
    ('channel_ties', 3, 10, 12, 4): 3,      # 0.00074 0.00078 0.0041
    ('pixel_ties', 1, 33, 35, 4): 0,        # 0.00051 0.0015 0.0057
    ('channel_ties', 1, 33, 35, 4): 0,      # 0.00035 0.0073 0.0034
    ('normal', 3, 10, 12, 1): 2,            # 0.00083 0.002 0.021
    ('normal', 3, 10, 12, 5): 5,            # 0.00045 0.0013 0.0094
    ('normal', 3, 10, 12, 16): 1,           # 0.00096 0.00077 0.0036
    ('normal', 1, 4, 422, 4): 1,            # 0.00035 0.00042 0.0078
}


def case_inputs(family, n, h, w, hidden=4):
    return tail_inputs(family, n, h, w, hidden, SEEDS[(family, n, h, w, hidden)])


def case_id(case):
    return '%s-%dx%dx%d-h%d' % case
