"""HAT at its published widths (embed_dim 144 / 180, six heads of 24 / 30, window 16): the fixtures' case table, the fp64
restatement's configuration (tests/hat_ref.py is already written in terms of the tensors' widths), and the float64 references, case
tables and refusal lists of csrc/hat_wide.hip and the wide channel attention of csrc/hat.hip (the srhip_hatw_* entry points), in the
manner of tests/attn_kernels_ref.py, whose bars, generators, channel-attention formulas and GPU protocol they reuse."""
import torch
import torch.nn.functional as F

from tests import attn_kernels_ref as A
from tests import hat_ref as H

DEPTHS = (2, 2)
WS = 16
# fixture -> (embed_dim, scale, input shape, (compress_ratio, squeeze_factor, mlp_ratio)), as tools/make_golden_hat_wide.py
CASES = {
    'hat180_x4': (180, 4, (2, 3, 32, 48), (3, 30, 2.)),
    'hat144_x2': (144, 2, (1, 3, 32, 32), (24, 24, 2.)),
    'hat180_x4pad': (180, 4, (1, 3, 20, 37), (3, 30, 2.)),
    'hat180_x3': (180, 3, (1, 3, 16, 32), (3, 30, 2.)),
}


def model_kwargs(name):
    """GeneratorResNet arguments of a fixture, without depths and num_heads (the fixtures use (2, 2), the full network (6,) * 6)."""
    dim, scale, _, (cr, sf, mlp) = CASES[name]
    return dict(upscale=scale, embed_dim=dim, window_size=WS, compress_ratio=cr, squeeze_factor=sf, mlp_ratio=mlp)


def config(name, depths=DEPTHS):
    """hat_ref.forward's configuration for a fixture."""
    dim, scale = CASES[name][:2]
    cfg = H.config(scale, WS, depths)
    cfg['dim'] = dim
    return cfg


# --------------------------------------------------------------------------------------------- #
# window attention at any (head width, heads, window)
# --------------------------------------------------------------------------------------------- #

SA, OCA = 0, 1


def attn_terms(qkv, table, kind, ws, shift, heads):
    """attn_kernels_ref.hat_attn_terms on qkv [n][h][w][3 heads d]: logits a [windows][heads][nq][nk] and v."""
    n, h, w, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    if kind == SA:
        t = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift else qkv
        tw = H.window_partition(t, ws).view(-1, ws * ws, 3 * c)
        b_, nq, _ = tw.shape
        p = tw.reshape(b_, nq, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = p[0] * d ** -0.5, p[1], p[2]
        rpi, nk = H.rpi_sa(ws), nq
    else:
        ows = ws + ws // 2
        q = H.window_partition(qkv[..., :c].contiguous(), ws).view(-1, ws * ws, c)
        kv = F.unfold(qkv[..., c:].permute(0, 3, 1, 2), (ows, ows), stride=ws, padding=(ows - ws) // 2)
        nw = kv.shape[-1]
        kv = kv.view(n, 2, c, ows * ows, nw).permute(1, 0, 4, 3, 2).reshape(2, n * nw, ows * ows, c)
        b_, nq, _ = q.shape
        nk = ows * ows
        q = q.reshape(b_, nq, heads, d).permute(0, 2, 1, 3) * d ** -0.5
        k = kv[0].reshape(b_, nk, heads, d).permute(0, 2, 1, 3)
        v = kv[1].reshape(b_, nk, heads, d).permute(0, 2, 1, 3)
        rpi = H.rpi_oca(ws)
    a = q @ k.transpose(-2, -1) + table[rpi.view(-1)].view(nq, nk, -1).permute(2, 0, 1).unsqueeze(0)
    if kind == SA and shift:
        m = H.shift_mask(h, w, ws, shift).to(a.dtype)
        nw = m.shape[0]
        a = (a.view(b_ // nw, nw, heads, nq, nk) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, nq, nk)
    return a, v


def attn_eval(inp, dtype):
    """out [n][h][w][C], lse [n][h][w][heads], dqkv, dtable for the cotangent inp['dout']."""
    kind, ws, shift, heads = inp['kind'], inp['ws'], inp['shift'], inp['heads']
    qkv, table = A._leaf(inp['qkv'], dtype), A._leaf(inp['table'], dtype)
    n, h, w, c3 = qkv.shape
    a, v = attn_terms(qkv, table, kind, ws, shift, heads)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(a.shape[0], a.shape[2], c3 // 3)
    out = A._unwindow(o, kind, ws, shift, h, w)
    lse = A._unwindow(torch.logsumexp(a.detach(), -1).transpose(1, 2), kind, ws, shift, h, w)
    dqkv, dtable = A._grads(out, [qkv, table], inp['dout'].to(dtype))
    return {'out': out.detach(), 'lse': lse, 'dqkv': dqkv, 'dtable': dtable}


# (kind, head width, heads, shift, n, h, w, family)
ATTN_CASES = [
    (SA, 30, 1, 0, 1, 16, 16, 'random'),       # one window, one head: the minimum
    (SA, 30, 6, 8, 1, 32, 48, 'random'),       # every mask-region pair; heads at 120-byte offsets
    (SA, 24, 6, 8, 2, 32, 32, 'random'),       # the other head width
    (OCA, 30, 6, 0, 1, 32, 48, 'random'),      # zero padding on all four borders; pixels held by one, two and four windows
    (OCA, 24, 6, 0, 1, 16, 16, 'random'),      # a single window whose key window is mostly padding
    (SA, 30, 6, 8, 3, 80, 80, 'random'),       # 75 windows > the dq kernel's 64 blocks per head: blocks that walk two windows
    (OCA, 30, 6, 0, 3, 80, 80, 'random'),
    (SA, 30, 6, 0, 3, 32, 32, 'x6'),           # logits of tens
    (SA, 30, 6, 0, 3, 32, 32, 'ascending'),    # the online soft-max rescales at every key tile ...
    (SA, 30, 6, 0, 3, 32, 32, 'descending'),   # ... or never
]
ATTN_UNCAPPED = ('x6', 'ascending', 'descending')


def attn_id(case):
    kind, d, heads, shift, n, h, w, family = case
    return '%s-d%d-h%d-s%d-%dx%dx%d-%s' % ('OCA' if kind else 'SA', d, heads, shift, n, h, w, family)


def attn_inputs(case):
    """attn_kernels_ref.hat_attn_inputs at window 16: random (qkv amplitude 1.5, table 0.5), x6 (amplitude 9), ascending / descending
    (q channels in [0.9, 1.1], k = 0.1 j (0.1 (255 - j)) for key slot j + noise below 0.005, table 0.05: the logit D^-0.5 q.k + bias
    moves by at least 0.4 per key, so every 32-key tile raises the running maximum, or none after the first does)."""
    kind, d, heads, shift, n, h, w, family = case
    c = d * heads
    g = A._gen(kind, d, heads, shift, n, h, w, len(family))
    amp = 9.0 if family == 'x6' else 1.5
    qkv = amp * A._u(g, n, h, w, 3 * c)
    table = 0.5 * A._u(g, A.hat_table_rows(kind, WS), heads)
    if family in ('ascending', 'descending'):
        assert kind == SA and shift == 0
        slot = (torch.arange(h) % WS).view(h, 1) * WS + (torch.arange(w) % WS).view(1, w)
        ramp = slot.float() if family == 'ascending' else (WS * WS - 1) - slot.float()
        qkv[..., :c] = 1.0 + 0.1 * A._u(g, n, h, w, c)
        qkv[..., c:2 * c] = (0.1 * ramp).view(1, h, w, 1) + 0.005 * A._u(g, n, h, w, c)
        table = 0.1 * table
    return {'qkv': qkv, 'table': table, 'dout': A._u(g, n, h, w, c), 'kind': kind, 'ws': WS, 'shift': shift, 'heads': heads}


# --------------------------------------------------------------------------------------------- #
# LayerNorm at C = 144, 180
# --------------------------------------------------------------------------------------------- #

LN_DIMS = (144, 180)
LN_TOKENS = (1, 5, 2049, 4099)            # a lone wave, a tail block; past the 512-block cap: blocks that walk two and three tokens
LN_CASES = [(c, f, t) for c in LN_DIMS for t in LN_TOKENS for f in A.LN_FAMILIES]


def ln_inputs(family, tokens, c):
    """attn_kernels_ref.ln_inputs at width c (mean_1000: c / 2 integers k / 8 and their negatives, shuffled)."""
    g = A._gen(tokens, c, 3 + A.LN_FAMILIES.index(family))
    x = A._u(g, tokens, c) + 0.3
    if family == 'constant_token':
        x[tokens // 2] = 0.75
    elif family == 'mean_1000':
        k = torch.randint(-4, 5, (tokens, c // 2), generator=g).float()
        k[:, 0] = 4.0
        k = torch.cat([k, -k], 1)
        order = torch.rand(tokens, c, generator=g).argsort(1)
        x = 1000.0 + k.gather(1, order) / 8
    return {'x': x, 'gamma': 1.0 + 0.2 * A._u(g, c), 'beta': 0.1 * A._u(g, c), 'dy': A._u(g, tokens, c), 'dadd': A._u(g, tokens, c)}


def ln_eval(inp, dtype, with_dadd):
    """attn_kernels_ref.ln_eval at the inputs' own width (float64: F.layer_norm; float32: the definition written out)."""
    x, gamma, beta = (A._leaf(inp[k], dtype) for k in ('x', 'gamma', 'beta'))
    if dtype == torch.float64:
        y = F.layer_norm(x, (x.shape[-1],), gamma, beta, 1e-5)
    else:
        mu = x.mean(-1, keepdim=True)
        y = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * gamma + beta
    dx, dg, db = A._grads(y, [x, gamma, beta], inp['dy'].to(dtype))
    xd = x.detach()
    mean = xd.mean(-1)
    rstd = 1.0 / torch.sqrt(((xd - mean.unsqueeze(-1)) ** 2).mean(-1) + 1e-5)
    return {'y': y.detach(), 'mean': mean, 'rstd': rstd, 'dx': dx + inp['dadd'].to(dtype) if with_dadd else dx, 'dgamma': dg, 'dbeta': db}


# --------------------------------------------------------------------------------------------- #
# channel attention and combine at C = 144, 180 (inputs and formulas: attn_kernels_ref.ca_inputs / ca_eval, any width)
# --------------------------------------------------------------------------------------------- #

CA_DIMS = ((144, 6), (180, 6), (180, 16))
CA_HW = (1, 7, 8, 9, 256)
CA_N = (1, 3)
CA_ZERO_UNIT = (3, 9, 180, 6)


# --------------------------------------------------------------------------------------------- #
# calls every new entry point must refuse on the host
# --------------------------------------------------------------------------------------------- #


def refusals(lib, p):
    """[(label, expected code, call)] for made-up or guarded addresses p['a'] .. p['l'], p['ws'] (p['ws_bytes'] bytes)."""
    out = []

    def add(entry, label, call, code=A.ERR_ARG):
        out.append(('%s: %s' % (entry, label), code, call))

    # LayerNorm
    a = dict(x=p['a'], gamma=p['b'], beta=p['c'], y=p['d'], mean=p['e'], rstd=p['f'])
    a2 = dict(dy=p['a'], x=p['b'], gamma=p['c'], mean=p['e'], rstd=p['f'], dadd=None, dx=p['d'], part=p['g'], dgamma=p['h'], dbeta=p['i'])

    def ln_fwd(t, tk=8, c=180):
        return lib.srhip_hatw_ln_fwd(t['x'], t['gamma'], t['beta'], t['y'], t['mean'], t['rstd'], tk, c, None)

    def ln_bwd(t, tk=8, c=180):
        return lib.srhip_hatw_ln_bwd(t['dy'], t['x'], t['gamma'], t['mean'], t['rstd'], t['dadd'], t['dx'], t['part'], t['dgamma'], t['dbeta'],
                                     tk, c, None)

    for label, b in A._variants(None, a, ('x', 'gamma', 'beta', 'y', 'mean', 'rstd'), ()):
        add('hatw_ln_fwd', label, lambda b=b: ln_fwd(b))
    for label, b in A._variants(None, a2, ('dy', 'x', 'gamma', 'mean', 'rstd', 'dx', 'part'), ()):
        add('hatw_ln_bwd', label, lambda b=b: ln_bwd(b))
    for tk in (0, -3):
        add('hatw_ln_fwd', 'tokens = %d' % tk, lambda tk=tk: ln_fwd(a, tk))
        add('hatw_ln_bwd', 'tokens = %d' % tk, lambda tk=tk: ln_bwd(a2, tk))
    for c in (96, 128, 146, 196, 0, -180):
        add('hatw_ln_fwd', 'C = %d' % c, lambda c=c: ln_fwd(a, 8, c))
        add('hatw_ln_bwd', 'C = %d' % c, lambda c=c: ln_bwd(a2, 8, c))

    # window attention
    geo = dict(kind=0, n=1, h=16, w=32, c=180, heads=6, ws=16, shift=8)
    f1 = dict(qkv=p['a'], table=p['b'], out=p['c'], lse=p['d'])
    f2 = dict(f1, dout=p['e'], dqkv=p['f'], dtable=p['g'])
    need_a = lib.srhip_hatw_attn_bwd_workspace(0, 1, 16, 32, 180, 6, 16)
    need_o = lib.srhip_hatw_attn_bwd_workspace(1, 1, 16, 32, 180, 6, 16)
    assert 0 < need_a < need_o <= p['ws_bytes']

    def attn_fwd(t, **kw):
        d = dict(geo, **kw)
        return lib.srhip_hatw_attn_fwd(t['qkv'], t['table'], t['out'], t['lse'], d['kind'], d['n'], d['h'], d['w'], d['c'], d['heads'], d['ws'],
                                       d['shift'], None)

    def attn_bwd(t, wsp=p['ws'], wb=None, **kw):
        d = dict(geo, **kw)
        wb = p['ws_bytes'] if wb is None else wb
        return lib.srhip_hatw_attn_bwd(t['qkv'], t['table'], t['out'], t['dout'], t['lse'], t['dqkv'], t['dtable'], wsp, wb, d['kind'], d['n'],
                                       d['h'], d['w'], d['c'], d['heads'], d['ws'], d['shift'], None)

    bad_geo = [('window 8', dict(ws=8, shift=4)), ('window 9', dict(ws=9, shift=0)), ('window 32', dict(ws=32, h=32, shift=0)),
               ('h = 24', dict(h=24)), ('w = 40', dict(w=40)), ('shift 4', dict(shift=4)), ('shift 16', dict(shift=16)),
               ('shift -8', dict(shift=-8)), ('OCA with a shift', dict(kind=1)), ('kind 2', dict(kind=2, shift=0)),
               ('heads of 16', dict(c=96)), ('heads of 32', dict(c=192)), ('heads of 30.17', dict(c=181)), ('no heads', dict(heads=0)),
               ('7 heads of 30', dict(c=210, heads=7)), ('9 heads of 24', dict(c=216, heads=9)), ('64 heads of 30', dict(c=1920, heads=64)),
               ('n = 0', dict(n=0)), ('n = -1', dict(n=-1)), ('h = 0', dict(h=0)), ('h = -16', dict(h=-16)), ('w = 0', dict(w=0)),
               ('w = -16', dict(w=-16))]
    for entry, fn, args, req, al in (('hatw_attn_fwd', attn_fwd, f1, ('qkv', 'table', 'out', 'lse'), ('qkv', 'out')),
                                     ('hatw_attn_bwd', attn_bwd, f2, ('qkv', 'table', 'out', 'dout', 'lse', 'dqkv', 'dtable'),
                                      ('qkv', 'out', 'dout', 'dqkv'))):
        for label, b in A._variants(None, args, req, al):
            add(entry, label, lambda b=b, fn=fn: fn(b))
        for label, kw in bad_geo:
            add(entry, label, lambda kw=kw, fn=fn, args=args: fn(args, **kw))
    add('hatw_attn_bwd', 'workspace 4 bytes off', lambda: attn_bwd(f2, wsp=p['ws'] + 4))
    add('hatw_attn_bwd', 'null workspace', lambda: attn_bwd(f2, wsp=None), A.ERR_WORKSPACE)
    add('hatw_attn_bwd', 'workspace one element short', lambda: attn_bwd(f2, wb=need_a - 4), A.ERR_WORKSPACE)
    add('hatw_attn_bwd', 'OCA workspace one element short', lambda: attn_bwd(f2, wb=need_o - 4, kind=1, shift=0), A.ERR_WORKSPACE)

    # channel attention and the combine's backward
    n, hw, c, hid = 2, 16, 180, 6
    need_k = lib.srhip_hat_combine_bwd_workspace(n, c, hid)
    c1 = dict(u=p['a'], w1=p['b'], b1=p['c'], w2=p['d'], b2=p['e'], s=p['f'], mz=p['g'])
    c3 = dict(g=p['a'], kb=p['b'], u=p['c'], s=p['d'], mz=p['e'], w1=p['f'], w2=p['g'], da=p['h'], du=p['i'], dw1=p['j'], db1=p['k'],
              dw2=p['l'], db2=p['b'])

    def ca_fwd(t, d=(n, hw, c, hid)):
        return lib.srhip_hatw_ca_fwd(t['u'], t['w1'], t['b1'], t['w2'], t['b2'], t['s'], t['mz'], *d, None)

    def cmb_bwd(t, ws=p['ws'], wb=None, d=(n, hw, c, hid)):
        return lib.srhip_hatw_combine_bwd(t['g'], t['kb'], t['u'], t['s'], t['mz'], t['w1'], t['w2'], t['da'], t['du'], t['dw1'], t['db1'],
                                          t['dw2'], t['db2'], ws, p['ws_bytes'] if wb is None else wb, A.CS, *d, None)

    for label, b in A._variants(None, c1, ('u', 'w1', 'w2', 's', 'mz'), ('u',)):
        add('hatw_ca_fwd', label, lambda b=b: ca_fwd(b))
    for label, b in A._variants(None, c3, ('g', 'u', 's', 'mz', 'w1', 'w2'), ('g', 'da', 'u', 's', 'du')):
        add('hatw_combine_bwd', label, lambda b=b: cmb_bwd(b))
    for label, d in (('C = 96', (n, hw, 96, hid)), ('C = 128', (n, hw, 128, hid)), ('C = 196', (n, hw, 196, hid)), ('C = 182', (n, hw, 182, hid)),
                     ('hidden 0', (n, hw, c, 0)), ('hidden 17', (n, hw, c, 17)), ('n = 0', (0, hw, c, hid)), ('hw = 0', (n, 0, c, hid)),
                     ('hw = -4', (n, -4, c, hid))):
        add('hatw_ca_fwd', label, lambda d=d: ca_fwd(c1, d))
        add('hatw_combine_bwd', label, lambda d=d: cmb_bwd(c3, d=d))
    add('hatw_combine_bwd', 'workspace 4 bytes off', lambda: cmb_bwd(c3, ws=p['ws'] + 4))
    add('hatw_combine_bwd', 'null workspace', lambda: cmb_bwd(c3, ws=None), A.ERR_WORKSPACE)
    add('hatw_combine_bwd', 'workspace one element short', lambda: cmb_bwd(c3, wb=need_k - 4), A.ERR_WORKSPACE)
    return out
