"""fp64 reference (plain torch, no kernels) of the forward and the backward of every ablation of the RAB / ResGroup attention tail --
csrc/attn_variants.hip -- in the style of tests/attn_tail_ref.py, whose helpers, input families and margins it re-uses.

    Chan_P(a):  avg_c = mean_p a, mx_c = max_p a, arg_c = the FIRST pixel attaining it;  s = sigmoid(sum_{q in P} fc2 relu(fc1 stat_q))
    Spat_P(a):  pa_p = mean_c a, pm_p = max_c a, argc_p = the FIRST channel attaining it; m = sigmoid(conv7x7(present maps, Avg first))

    CA-SA  s = Chan(u), m = Spat(s u), z = m (s u)        SA-CA  m = Spat(u), s = Chan(m u), z = s (m u)
    CA     s = Chan(u), z = s u          SA  m = Spat(u), z = m u          CA|SA  s = Chan(u), m = Spat(u), z = cat[s u, m u]

P (`pool`) is 'Avg', 'Max' or 'Avg|Max' for both gates.  A case's 7x7 kernel is the family's w7 [1, 2, 7, 7] restricted to the rows
of P, so one draw serves the three pool sets.  Shapes as in attn_tail_ref; pooled is [n, hw, |P|]; entries a variant does not have
are None."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import attn_tail_ref as A

C = A.C
MODES = ('CA-SA', 'SA-CA', 'CA', 'SA', 'CA|SA')
ORDER = {m: i for i, m in enumerate(MODES)}            # SRHIP_ATTN_* of include/sradsgan_hip.h
POOLS = ('Avg', 'Max', 'Avg|Max')
POOL_BITS = {'Avg': 1, 'Max': 2, 'Avg|Max': 3}
# the 21 non-trivial (la_mode, pool, addconv) combinations: addconv only changes a '-' mode
VARIANTS = ([(m, p, True) for m in ('CA', 'SA', 'CA|SA') for p in POOLS]
            + [(m, p, a) for m in ('CA-SA', 'SA-CA') for p in POOLS for a in (True, False)])
FORWARDS = [(m, p) for m in MODES for p in POOLS]      # what the forward kernels can tell apart


def variant_id(v):
    return '-'.join(str(x).replace('|', '+') for x in v)


def pool_rows(pool):
    return [i for i, name in enumerate(('Avg', 'Max')) if name in pool.split('|')]


def w7_of(w7, pool):
    """The rows of a [1, 2, 7, 7] kernel that the pool set keeps: [1, |P|, 7, 7]."""
    return w7.reshape(1, 2, 7, 7)[:, pool_rows(pool)].contiguous()


def _chan(a, fc1, fc2, pool):
    """a [n, 64, hw] fp64 -> dict avg, mx, arg (None outside the pool set), s."""
    out = dict(avg=None, mx=None, arg=None)
    logit = 0
    if 'Avg' in pool:
        out['avg'] = a.mean(2)
        logit = logit + torch.relu(out['avg'] @ fc1.t()) @ fc2.t()
    if 'Max' in pool:
        out['mx'], out['arg'] = a.amax(2), A.first_argmax(a, 2)
        logit = logit + torch.relu(out['mx'] @ fc1.t()) @ fc2.t()
    out['s'] = torch.sigmoid(logit)
    return out


def _conv7(p, w7):
    """p [n, k, h, w], w7 [k, 7, 7] -> [n, h, w]: cross-correlation with zero padding 3, tap by tap."""
    n, k, h, w = p.shape
    pp = F.pad(p, (3, 3, 3, 3))
    out = torch.zeros(n, h, w, dtype=p.dtype)
    for kh in range(7):
        for kw in range(7):
            out += (w7[:, kh, kw].view(1, k, 1, 1) * pp[:, :, kh:kh + h, kw:kw + w]).sum(1)
    return out


def _spat(a, w7, pool, h, w):
    """a [n, 64, hw] fp64 -> dict pooled [n, hw, |P|], argc (None without Max), m [n, hw]."""
    n = a.shape[0]
    maps, argc = [], None
    if 'Avg' in pool:
        maps.append(a.mean(1))
    if 'Max' in pool:
        maps.append(a.amax(1))
        argc = A.first_argmax(a, 1)
    pooled = torch.stack(maps, 2)
    m = torch.sigmoid(_conv7(pooled.permute(0, 2, 1).reshape(n, len(maps), h, w), w7)).reshape(n, h * w)
    return dict(pooled=pooled, argc=argc, m=m)


def variant_fwd_ref(u, fc1, fc2, w7, mode, pool):
    """fp64 forward.  w7: the family's [1, 2, 7, 7] kernel (restricted here).  Returns avg, mx, arg, s, pooled, argc, m (None where the
    variant has none), z [n, 64 or 128, h, w], and chan_in / spat_in [n, 64, hw]: the tensors the two gates pooled."""
    n, c, h, w = u.shape
    assert c == C
    uf = u.detach().double().reshape(n, c, h * w)
    fc1 = fc1.detach().double().reshape(-1, C)
    fc2 = fc2.detach().double().reshape(C, fc1.shape[0])
    k7 = w7_of(w7.detach().double(), pool)[0]
    out = dict.fromkeys(('avg', 'mx', 'arg', 's', 'pooled', 'argc', 'm', 'chan_in', 'spat_in'))
    if mode == 'CA-SA':
        out.update(_chan(uf, fc1, fc2, pool), chan_in=uf)
        y = out['s'][:, :, None] * uf
        out.update(_spat(y, k7, pool, h, w), spat_in=y)
        z = out['m'][:, None, :] * y
    elif mode == 'SA-CA':
        out.update(_spat(uf, k7, pool, h, w), spat_in=uf)
        y = out['m'][:, None, :] * uf
        out.update(_chan(y, fc1, fc2, pool), chan_in=y)
        z = out['s'][:, :, None] * y
    elif mode == 'CA':
        out.update(_chan(uf, fc1, fc2, pool), chan_in=uf)
        z = out['s'][:, :, None] * uf
    elif mode == 'SA':
        out.update(_spat(uf, k7, pool, h, w), spat_in=uf)
        z = out['m'][:, None, :] * uf
    else:
        out.update(_chan(uf, fc1, fc2, pool), chan_in=uf)
        out.update(_spat(uf, k7, pool, h, w), spat_in=uf)
        z = torch.cat([out['s'][:, :, None] * uf, out['m'][:, None, :] * uf], 1)
    out['z'] = z.reshape(n, -1, h, w)
    return out


def variant_torch(u, fc1, fc2, w7, mode, pool, dtype=torch.float32):
    """The straightforward stock-torch formulation in `dtype` (adaptive pools, mean / max over dim 1, F.conv2d): the error yardstick
    of the GPU tests in fp32.  A pooled VALUE does not depend on which of several equal elements torch picks.  Returns avg, mx, s,
    pooled, m, z in variant_fwd_ref's shapes (None where absent)."""
    n, c, h, w = u.shape
    hw = h * w
    hid = fc1.numel() // C
    uu = u.detach().to(dtype)
    a1, a2 = fc1.detach().to(dtype).reshape(hid, C, 1, 1), fc2.detach().to(dtype).reshape(C, hid, 1, 1)
    k7 = w7_of(w7.detach().to(dtype), pool)
    mlp = lambda t: F.conv2d(F.relu(F.conv2d(t, a1)), a2)
    out = dict.fromkeys(('avg', 'mx', 's', 'pooled', 'm'))

    def chan(a):
        logit = 0
        if 'Avg' in pool:
            avg = F.adaptive_avg_pool2d(a, 1)
            out['avg'], logit = avg.reshape(n, c), logit + mlp(avg)
        if 'Max' in pool:
            mx = F.adaptive_max_pool2d(a, 1)
            out['mx'], logit = mx.reshape(n, c), logit + mlp(mx)
        s = torch.sigmoid(logit)
        out['s'] = s.reshape(n, c)
        return s * a

    def spat(a):
        maps = []
        if 'Avg' in pool:
            maps.append(a.mean(1, keepdim=True))
        if 'Max' in pool:
            maps.append(a.max(1, keepdim=True)[0])
        pooled = torch.cat(maps, 1)
        m = torch.sigmoid(F.conv2d(pooled, k7, padding=3))
        out['pooled'], out['m'] = pooled.reshape(n, len(maps), hw).permute(0, 2, 1), m.reshape(n, hw)
        return m * a

    if mode == 'CA-SA':
        z = spat(chan(uu))
    elif mode == 'SA-CA':
        z = chan(spat(uu))
    elif mode == 'CA':
        z = chan(uu)
    elif mode == 'SA':
        z = spat(uu)
    else:
        z = torch.cat([chan(uu), spat(uu)], 1)
    out['z'] = z
    return out


def variant_grads(dz, u, fc1, fc2, w7, mode, pool, arg=None, argc=None, dtype=torch.float64):
    """du, dfc1 [hidden, 64], dfc2 [64, hidden], dw7 [|P|, 7, 7] (None where the variant has no such parameter) for the gradient dz
    at z ([n, 64 or 128, h, w]), by autograd in `dtype` of the formulation whose max pools are GATHERS at the given first-arg-max
    indices (None: the fp64 reference's own) -- the gradient goes where the caller says, never where torch breaks a tie.  fp64: the
    reference of the GPU tests; fp32 with the observed indices: their yardstick."""
    n, c, h, w = u.shape
    hw = h * w
    hid = fc1.numel() // C
    if arg is None or argc is None:
        f = variant_fwd_ref(u, fc1, fc2, w7, mode, pool)
        arg = f['arg'] if arg is None else arg
        argc = f['argc'] if argc is None else argc
    uu = u.detach().to(dtype).requires_grad_()
    a1 = fc1.detach().to(dtype).reshape(hid, C, 1, 1).requires_grad_()
    a2 = fc2.detach().to(dtype).reshape(C, hid, 1, 1).requires_grad_()
    k7 = w7_of(w7.detach().to(dtype), pool).requires_grad_()
    mlp = lambda t: F.conv2d(F.relu(F.conv2d(t, a1)), a2)

    def chan(a):
        logit = 0
        if 'Avg' in pool:
            logit = logit + mlp(a.mean((2, 3), keepdim=True))
        if 'Max' in pool:
            mx = a.reshape(n, c, hw).gather(2, arg.detach().cpu().long().reshape(n, c, 1)).reshape(n, c, 1, 1)
            logit = logit + mlp(mx)
        return torch.sigmoid(logit) * a

    def spat(a):
        maps = []
        if 'Avg' in pool:
            maps.append(a.mean(1, keepdim=True))
        if 'Max' in pool:
            maps.append(a.gather(1, argc.detach().cpu().long().reshape(n, 1, h, w)))
        return torch.sigmoid(F.conv2d(torch.cat(maps, 1), k7, padding=3)) * a

    z = {'CA-SA': lambda: spat(chan(uu)), 'SA-CA': lambda: chan(spat(uu)), 'CA': lambda: chan(uu), 'SA': lambda: spat(uu),
         'CA|SA': lambda: torch.cat([chan(uu), spat(uu)], 1)}[mode]()
    wrt = [uu] + ([a1, a2] if 'CA' in mode else []) + ([k7] if 'SA' in mode else [])
    gs = list(torch.autograd.grad(z, wrt, dz.detach().to(dtype)))
    out = dict(du=gs.pop(0), dfc1=None, dfc2=None, dw7=None)
    if 'CA' in mode:
        out['dfc1'], out['dfc2'] = gs.pop(0).reshape(hid, C), gs.pop(0).reshape(C, hid)
    if 'SA' in mode:
        out['dw7'] = gs.pop(0).reshape(-1, 7, 7)
    return out


def case_dz(t, mode):
    """The gradient at z of a case: [n, 64, h, w], or [n, 128, h, w] for CA|SA (the case's dz and g side by side)."""
    return torch.cat([t['dz'], t['g']], 1) if mode == 'CA|SA' else t['dz']


# --------------------------------------------------------------------------------------------- #
# margins: every decision of a forward -- the pixel arg-max of the tensor the channel gate pooled, the channel arg-max of the tensor
# the spatial gate pooled, the ReLU inputs of each present pool -- away from a flip, in the fp64 reference alone
# --------------------------------------------------------------------------------------------- #


def margins(t, mode, pool):
    """(channel, pixel, relu) minima of one forward configuration; inf where the configuration takes no such decision.  The constructed
    bit-exact ties are exempt where they ARE ties: a pixel tie of u is none in m u (SA-CA pools that), so nothing is exempt there;
    the channel ties survive every gate (the tied channels share u, their fc1 column and their fc2 row)."""
    f = variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)
    inf = float('inf')
    cm = pm = rm = inf
    has_max = 'Max' in pool
    if f['spat_in'] is not None and has_max:
        cm = float(A._top2_gap(f['spat_in'].masked_fill(t['exempt_c'], -inf), 1).min())
    if f['chan_in'] is not None:
        if has_max:
            a = f['chan_in'] if mode == 'SA-CA' else f['chan_in'].masked_fill(t['exempt_p'], -inf)
            pm = float(A._top2_gap(a, 2).min())
        fc1 = t['fc1'].double().reshape(-1, C)
        for key in ('avg', 'mx'):
            if f[key] is not None:
                x = f[key]
                rm = min(rm, float(((x @ fc1.t()).abs() / (x.abs() @ fc1.abs().t()).clamp_min(1e-300)).min()))
    return cm, pm, rm


def case_margins(t):
    """The minima over all 15 forward configurations."""
    ms = [margins(t, m, p) for m, p in FORWARDS]
    return tuple(min(x[i] for x in ms) for i in range(3))


def assert_margins(t, what=''):
    cm, pm, rm = case_margins(t)
    assert cm > A.CHANNEL_MARGIN and pm > A.PIXEL_MARGIN and rm > A.RELU_MARGIN, \
        '%s: input too close to a flip: channel %.3g (> %g), pixel %.3g (> %g), relu %.3g (> %g)' % (
            what, cm, A.CHANNEL_MARGIN, pm, A.PIXEL_MARGIN, rm, A.RELU_MARGIN)


# --------------------------------------------------------------------------------------------- #
# the cases of tests/test_attn_variants_gpu.py: (family, n, h, w) -> seed of attn_tail_ref.tail_inputs (hidden = 4).  One input serves
# all 15 forward configurations, so a seed must show the margins in every one of them; tests/test_attn_variants_ref_cpu.py asserts it.
# --------------------------------------------------------------------------------------------- #

SHAPES = [(1, 1, 1),         # empty pooling segments, one partial 16-lane pixel group, the 7x7 halo entirely outside the image
          (2, 3, 5),         # hw < 16, W < 7
          (3, 10, 12),       # n not a power of two
          (2, 13, 70)]       # W > 64, 57 pixels per segment with a ragged last one
TIE_SHAPE = (3, 10, 12)
CASES = [(f,) + s for s in SHAPES for f in A.FAMILIES[:3]] + [(f,) + TIE_SHAPE for f in A.FAMILIES[3:]]

SEEDS = {                                   # minima over the 15 configurations in the fp64 reference: channel, pixel, relu margin
    ('normal', 1, 1, 1): 0,                 # 0.012 inf 0.063
    ('late_max', 1, 1, 1): 0,               # 0.07 inf 0.015
    ('all_negative', 1, 1, 1): 0,           # 0.11 inf 0.008
    ('normal', 2, 3, 5): 0,                 # 0.0044 0.0014 0.0072
    ('late_max', 2, 3, 5): 0,               # 0.0022 0.12 0.016
    ('all_negative', 2, 3, 5): 1,           # 0.0015 0.00078 0.085
    ('normal', 3, 10, 12): 7,               # 0.00056 0.00049 0.0064
    ('late_max', 3, 10, 12): 1,             # 0.0006 0.0023 0.017
    ('all_negative', 3, 10, 12): 7,         # 0.00033 0.00055 0.032
    ('normal', 2, 13, 70): 198,             # 0.0003 0.00028 0.0053
    ('late_max', 2, 13, 70): 14,            # 0.00029 0.0006 0.0035
    ('all_negative', 2, 13, 70): 28,        # 0.00024 0.0024 0.0058
    ('pixel_ties', 3, 10, 12): 16,          # 0.00063 0.00072 0.02
    ('channel_ties', 3, 10, 12): 16,        # 0.0003 0.00051 0.0025
}


HIDDEN_SHAPE, HIDDENS = (3, 10, 12), (1, 5, 16)     # the MLP kernels at other hidden sizes ('normal' family): one unit, no power of two, the limit
HIDDEN_SEEDS = {                                    # hidden -> seed; the same minima
    1: 8,                                           # 0.00025 0.0003 0.011
    5: 5,                                           # 0.00045 0.00078 0.0094
    16: 15,                                         # 0.00027 0.0012 0.0021
}


def case_inputs(family, n, h, w, hidden=4):
    """attn_tail_ref.tail_inputs at the tabulated seed, plus wc2 [64, 128, 1, 1]: the closing conv of CA|SA.  hidden != 4: the
    HIDDEN_SHAPE cases of HIDDEN_SEEDS."""
    if hidden == 4:
        seed = SEEDS[(family, n, h, w)]
    else:
        assert (family, n, h, w) == ('normal',) + HIDDEN_SHAPE
        seed = HIDDEN_SEEDS[hidden]
    t = A.tail_inputs(family, n, h, w, hidden, seed)
    g = torch.Generator().manual_seed(7 + seed)
    t['wc2'] = 0.1 * torch.randn(C, 2 * C, 1, 1, generator=g)
    return t


def case_id(case):
    return '%s-%dx%dx%d' % case


# --------------------------------------------------------------------------------------------- #
# the generator ablations recorded from the reference in tests/golden/gen_ablation.npz (tools/make_golden_ablation.py):
# (rla_mode, bla_mode, ga_mode, pool_mode, addconv) of a 2-group x 1-block x2 generator on a (2, 3, 12, 12) input
# --------------------------------------------------------------------------------------------- #

GEN_CONFIGS = [('CA-SA', 'CA-SA', 'CA-SA', 'Avg', True),
               ('CA-SA', 'CA-SA', 'CA-SA', 'Max', True),
               ('SA-CA', 'SA-CA', 'SA-CA', 'Avg|Max', True),
               ('CA|SA', 'CA|SA', 'CA|SA', 'Avg|Max', True),
               ('CA', 'SA', 'CA', 'Max', True),
               ('', '', '', 'Avg|Max', True),
               ('CA-SA', 'SA-CA', 'SA', 'Avg', False)]
GEN_SHAPE, GEN_SCALE, GEN_GROUPS, GEN_BLOCKS = (2, 3, 12, 12), 2, 2, 1
GEN_RTOL, GEN_ATOL = 1e-3, 2e-5               # the bar of the recorded digests, as tests/test_oracle_golden.py holds gradients to


def gen_tag(cfg):
    return 'abl_' + '_'.join(str(x).replace('|', 'p').replace('-', 'm') or 'none' for x in cfg)


def gen_kwargs(cfg):
    rla, bla, ga, pool, addconv = cfg
    return dict(n_residual_blocks=GEN_GROUPS, n_basic_blocks=GEN_BLOCKS, rla_mode=rla, bla_mode=bla, ga_mode=ga, pool_mode=pool,
                addconv=addconv, upscale_factor=GEN_SCALE)


def small_digest(t, keep=126):
    """oracle.sradsgan_ref.digest cut to its first `keep` samples and its trailing [sum, l2 norm]: a whole generator's gradients in a
    few hundred KB."""
    from oracle import sradsgan_ref as O
    d = O.digest(t)
    return d if d.size <= keep + 2 else np.concatenate([d[:keep], d[-2:]])


def gen_run(module, cfg):
    """det_init_, forward on the recorded input, backward of the recorded cotangent.  Returns (y, the module)."""
    from oracle import sradsgan_ref as O
    tag = gen_tag(cfg)
    O.det_init_(module, prefix=tag + '.')
    y = module(O.det_fill('abl.x', GEN_SHAPE, 0.5, 0.5))
    y.backward(O.det_fill(tag + '.dy', tuple(y.shape), 1.0))
    return y, module
