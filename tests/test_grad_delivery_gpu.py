"""Where ops.py delivers parameter gradients, op by op (the table: tests/grad_delivery_cases.py; the queue and the scopes without a
device: tests/test_grad_delivery_cpu.py).

TrainStep runs every backward inside ops.direct_param_grads(side, group=2): a parameter gradient is then not returned to autograd but
accumulated into the parameter's .grad by the kernel, by a grouped launch, by the plane path, by an add_ behind the plain kernel, or
by a norm / attention kernel through its accumulate slot.  The kernel tests call the ops in plain autograd mode; this file runs every
row of the table

  A  plain (no context, .grad None): g_A per parameter against the row's fp64 reference at the bar of the op's own kernel test --
     which ties everything below to a reference and not only to the code under test;
  B  under direct_param_grads with (no side stream, 1), (side, 1), (side, 2) and a random non-zero prior G0 in every .grad:
       .grad == G0 + reference within the bar plus one fp32 rounding of |G0 + g|,
       .grad == fp32(G0 + g_A) bit for bit where the route adds the same fp32 sum once (the row's `exact`),
       dx bit-identical to A,
       autograd saw a gradient for a parameter exactly when no slot was used (tensor hooks on the leaves),

then the cases a single row cannot show: mixed slots, one parameter used twice (the repeated-slot race of the grouped launch, fixed in
_WgradQueue.add), odd partner counts, ageing, pruning by backward_scope / no_param_grads, and the two carry_open branches
tests/test_model_gpu.py leaves out.  Fixed seeds, random upstream gradients, the table's small shapes throughout; every figure is
printed before it is asserted (-s)."""
import contextlib
import importlib
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import conv_emulation as E
from tests import grad_delivery_cases as C
from tests import reduction_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
U = E.U24
CL = torch.channels_last


def _imp(spec):
    mod, name = spec.split(':')
    return getattr(importlib.import_module(mod), name)


def _tau(arith):
    return _imp(C.CONV_BAR)[arith]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _r(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _cl(t):
    t = t.to(DEV)
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()


def _rows(t):
    """[n, c, h, w] -> the [n, hw, c] rows the references are written on (CPU)."""
    n, c, h, w = t.shape
    return t.detach().cpu().permute(0, 2, 3, 1).reshape(n, h * w, c)


def _lib():
    from sradsgan_amd import _hip
    return _hip.lib()


def rel_tol(ref, y32):
    """The bar of tests/reduction_ref.py (8 x the error of stock fp32 torch, floor 32 * 2^-24) as an absolute tolerance for one tensor."""
    ref = torch.as_tensor(ref).detach().cpu().double()
    return R.bound(R.err(y32, ref)) * max(float(ref.abs().max()), 1e-30)


def conv_tol(ref, absref, arith):
    return E.bound(ref, absref, _tau(arith))


def plane_halves(t):
    """(hi, lo) as [n, c, h, w] float64 of a weight-gradient operand: the halves a padded-plane buffer STORES (include/sradsgan_hip.h: per 8
    channels 8 hi | 8 lo, pixel (b, y, x) at row guard + (b (H + 1) + y)(W + 1) + x), or the split of an fp32 operand (ops._to_planes)."""
    from sradsgan_amd import ops
    if not isinstance(t, ops.PP):
        return E.split_bf16(t)
    n, c, h, w = t.shape
    b, y, x = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing='ij')
    rows = (_lib().srhip_pp_guard(w) + (b * (h + 1) + y) * (w + 1) + x).reshape(-1).to(DEV)
    planes = t.buf.view(-1, c // 8, 2, 8)[rows].double()
    img = lambda v: v.reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    return img(planes[:, :, 0, :]), img(planes[:, :, 1, :])


# ================================================================================================================================ #
# builders: row -> tensors, forward, reference
# ================================================================================================================================ #
class Built:
    """params / inputs: name -> device tensor (the data every run clones its leaves from); dx: the inputs whose gradient is compared;
    forward(P, X) -> y; reference(A) -> name -> (fp64 reference, absolute tolerance: a float or a tensor of the reference's shape)."""
    dx = ('x',)

    def __init__(self, row):
        self.row = row

    def check(self, lib, ops):
        for pred in self.row['pred']:
            ok, got = C.predicate_holds(pred, lib, ops)
            assert ok, '%s: predicate %s answers %s: the row has left its route' % (self.row['id'], pred, got)


class Conv(Built):
    """conv2d and what rides on a conv's weight gradient: conv2d_pool, pixel_shuffle_act behind a conv, conv2d_dil, linear."""

    def __init__(self, row, tag=0, shape=None, bias=True):
        super().__init__(row)
        n, cin, h, w, cout = shape or row['shape']
        g = _gen(row['id'], tag)
        self.lin = bool(row.get('linear'))
        self.k, self.pad = (1, 0) if self.lin else (3, row.get('dilation', 1))
        wshape = (cout, cin) if self.lin else (cout, cin, 3, 3)
        self.inputs = dict(x=_cl(_r(g, n, cin, h, w)))
        self.params = dict(w=_r(g, *wshape, scale=(cin * self.k * self.k) ** -0.5).to(DEV))
        if bias:
            self.params['b'] = _r(g, cout, scale=0.1).to(DEV)
        r, _ = row.get('shuffle', (1, None))
        self.gout = _cl(_r(g, n, cout // (r * r), h * r, w * r))
        self.dx = ('x',) if row.get('want_dx', True) else ()
        self.wshape4 = (cout, cin, self.k, self.k)

    def check(self, lib, ops):
        super().check(lib, ops)
        if self.row.get('pool'):
            assert ops.pool_epilogue_ok(self.inputs['x'], self.params['w']), 'conv2d_pool would fall back on conv2d'

    def forward(self, P, X):
        from sradsgan_amd import ops
        row, b = self.row, P.get('b')
        if row.get('pool'):
            y, pool = ops.conv2d_pool(X['x'], P['w'], b)
            assert pool is not None
            return y
        if 'dilation' in row:
            return ops.conv2d_dil(X['x'], P['w'], b, row['dilation'])
        if self.lin:
            return ops.linear(X['x'], P['w'], b)
        y = ops.conv2d(X['x'], P['w'], b, 1, 1, act_slope=row.get('slope'))
        if 'shuffle' in row:
            y = ops.pixel_shuffle_act(y, *row['shuffle'])
        return y

    def grad_at_conv(self, y, gout=None):
        """The gradient at the conv's own output, in the fp32 operations of the kernels behind it (one multiply by the slope)."""
        from tests import pointwise_ref as PW
        row = self.row
        gout = self.gout if gout is None else gout
        if 'shuffle' in row:
            r, slope = row['shuffle']
            nhwc = lambda t: t.detach().cpu().permute(0, 2, 3, 1).contiguous()
            return PW.pixel_shuffle_bwd_ref(nhwc(gout), nhwc(y), r, slope).permute(0, 3, 1, 2).to(DEV)
        if row.get('slope') is not None:
            return torch.where(y.detach() > 0, gout, gout * torch.tensor(row['slope'], device=DEV))
        return gout

    def wgrad_ref(self, x, g):
        row = self.row
        ref, absref = E.conv_wgrad(x, g, self.wshape4, 1, self.pad, row['arith'], dil=row.get('dilation', 1))
        out = dict(w=(ref.reshape(self.params['w'].shape), conv_tol(ref, absref, row['arith']).reshape(self.params['w'].shape)))
        if 'b' in self.params:
            gb, ab = g.double().sum((0, 2, 3)), g.double().abs().sum((0, 2, 3))
            out['b'] = (gb, conv_tol(gb, ab, 'fp32'))
        return out

    def reference(self, A):
        return self.wgrad_ref(self.inputs['x'], self.grad_at_conv(A.y))


class Norm(Built):
    def __init__(self, row):
        super().__init__(row)
        n, c, h, w = row['shape']
        t = R.bn_inputs('normal', n * h * w, c, seed=3)
        back = lambda v: _cl(v.reshape(n, h, w, c).permute(0, 3, 1, 2))
        self.t, self.dims = t, (n, c, h, w)
        self.inputs, self.gout = dict(x=back(t['x'])), back(t['dy'])
        self.gn = row['op'] == 'group_norm_act'
        self.params = {}
        if row.get('affine', True):
            shape = (1, c, 1, 1) if self.gn else (c,)
            self.params = dict(gamma=t['gamma'].reshape(shape).to(DEV), beta=t['beta'].reshape(shape).to(DEV))

    def forward(self, P, X):
        from sradsgan_amd import ops
        row = self.row
        if self.gn:
            return ops.group_norm_act(X['x'], row['groups'], P.get('gamma'), P.get('beta'), 1e-5, row['unbiased'], row['slope'])
        c = self.dims[1]
        bn = types.SimpleNamespace(training=True, weight=P['gamma'], bias=P['beta'], running_mean=torch.zeros(c, device=DEV),
                                   running_var=torch.ones(c, device=DEV), eps=1e-5, momentum=0.1, num_batches_tracked=torch.zeros((), dtype=torch.long))
        return ops.batch_norm_act(X['x'], bn, row['slope'])

    def reference(self, A):
        if not self.params:
            return {}
        row, t = self.row, self.t
        n, c, h, w = self.dims
        mask = _rows(A.y) > 0                                          # the LeakyReLU mask as observed, as the kernel tests take it
        if self.gn:
            from tests import groupnorm_ref as G
            x3, dy3 = t['x'].reshape(n, h * w, c), t['dy'].reshape(n, h * w, c)
            _, dg, db = G.gn_bwd_ref(dy3, x3, t['gamma'], mask, row['groups'], row['unbiased'], 1e-5, row['slope'])
            a64, a32 = (G.gn_autograd(x3, t['gamma'], t['beta'], dy3, t['u'].reshape(n, h * w, c), row['groups'], row['unbiased'], 1e-5, row['slope'], d)
                        for d in (torch.float64, torch.float32))
        else:
            _, dg, db = R.bn_bwd_ref(t['dy'], t['x'], t['gamma'], mask.reshape(-1, c), 1e-5, row['slope'])
            a64, a32 = (R.bn_autograd(t['x'], t['gamma'], t['beta'], t['dy'], t['u'], 1e-5, row['slope'], d) for d in (torch.float64, torch.float32))
        shape = self.params['gamma'].shape
        tol = lambda k: R.bound(R.err(a32[k], a64[k])) * float(a64[k].abs().max())      # torch's error under its own mask
        return dict(gamma=(dg.reshape(shape), tol('dgamma')), beta=(db.reshape(shape), tol('dbeta')))


class Gam(Built):
    """cgam / sgam on the inputs of tests/attn_kernels_ref.py."""

    def __init__(self, row):
        super().__init__(row)
        from tests import attn_kernels_ref as AK
        n, c, h, w = row['shape']
        self.sg = row['op'] == 'sgam'
        self.inp = inp = AK.sgam_inputs('random', n, h * w) if self.sg else AK.cgam_inputs(n, h * w, 0.3)
        img = lambda v: _cl(v.reshape(n, h, w, -1).permute(0, 3, 1, 2))
        self.inputs = {k: img(inp[k]) for k in (('x', 'q', 'k', 'v') if self.sg else ('x',))}
        self.params, self.gout = dict(gamma=inp['gamma'].clone().to(DEV)), img(inp['dy'])
        self.dx = tuple(self.inputs)

    def forward(self, P, X):
        from sradsgan_amd import ops
        return ops.sgam(X['x'], X['q'], X['k'], X['v'], P['gamma']) if self.sg else ops.cgam(X['x'], P['gamma'])

    def reference(self, A):
        from tests import attn_kernels_ref as AK
        ev = AK.sgam_eval if self.sg else AK.cgam_eval
        ref, t32 = ev(self.inp, torch.float64), ev(self.inp, torch.float32)
        if self.sg:
            bars = AK.bars(ref, t32, 'sgam', True, AK.sgam_split_emulation(self.inp), AK.sgam_scales(self.inp))
        else:
            bars = AK.bars(ref, t32, 'cgam')
        return dict(gamma=(ref['dgamma'].reshape(1), bars['dgamma'][0] * float(ref['dgamma'].abs().max())))


def _tail_params(t):
    from tests.test_attn_tail_gpu import _ops_params
    return dict(zip(('fc1', 'fc2', 'w7', 'wc', 'bc'), _ops_params(t)))


def _tail_reference(t, arg, argc, arith):
    """name -> (reference, tolerance) of the tail's five parameters: attn_tail_ref.e2e_ref against the yardstick of
    tests/test_attn_tail_gpu.py (stock fp32 torch around the emulated 1x1 conv)."""
    from tests import attn_tail_ref as A
    from tests.test_attn_tail_gpu import _emulated
    want, y32 = A.e2e_ref(t, arg, argc), A.e2e_torch32(t, arg, argc, **_emulated(arith))
    hid = t['hidden']
    shapes = dict(fc1=(hid, A.C, 1, 1), fc2=(A.C, hid, 1, 1), w7=(1, 2, 7, 7), wc=(A.C, A.C, 1, 1), bc=(A.C,))
    return {k: (want['d' + k].reshape(shapes[k]), rel_tol(want['d' + k], y32['d' + k].reshape(want['d' + k].shape))) for k in shapes}, want


def _assert_indices(saved, t, what):
    """The kernels' arg-maxes are the fp64 reference's: the references below differentiate the maxima at the reference's own indices."""
    from tests import attn_tail_ref as A
    f = A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    n = t['u'].shape[0]
    assert torch.equal(saved[2].cpu().long(), f['arg']) and torch.equal(saved[5].cpu().long().view(n, -1), f['argc']), '%s: an arg-max differs from fp64' % what
    return f['arg'], f['argc']


class Tail(Built):
    def __init__(self, row):
        super().__init__(row)
        from tests import attn_tail_ref as A
        n, _, h, w = row['shape']
        self.t = t = A.case_inputs('normal', n, h, w, 4)
        self.inputs = dict(u=_cl(t['u']), skip=_cl(t['skip']))
        self.params, self.gout = _tail_params(t), _cl(t['g'])
        self.dx = ('u', 'skip')

    def forward(self, P, X):
        from sradsgan_amd import ops
        return ops.attention_tail(X['u'], X['skip'], P['fc1'], P['fc2'], P['w7'], P['wc'], P['bc'])

    def reference(self, A):
        from sradsgan_amd import ops
        with torch.no_grad():
            _, saved = ops._tail_forward(self.inputs['u'], self.inputs['skip'], *self.params.values())
        arg, argc = _assert_indices(saved, self.t, self.row['id'])
        return _tail_reference(self.t, arg, argc, ops.get_conv_math())[0]


class Variant(Built):
    def __init__(self, row):
        super().__init__(row)
        from tests import attn_variants_ref as V
        n, _, h, w = row['shape']
        self.t = t = V.case_inputs('normal', n, h, w)
        self.mode, self.pool = row['la_mode'], row['pool_mode']
        self.inputs = dict(u=_cl(t['u']), skip=_cl(t['skip']))
        self.gout = _cl(t['dz'])                                       # no closing conv: the gradient at out is the gradient at z
        p = {}
        if 'CA' in self.mode:
            p.update(fc1=t['fc1'].reshape(4, V.C, 1, 1).to(DEV), fc2=t['fc2'].reshape(V.C, 4, 1, 1).to(DEV))
        if 'SA' in self.mode:
            p.update(w7=V.w7_of(t['w7'], self.pool).to(DEV))
        self.params, self.dx = p, ('u', 'skip')

    def forward(self, P, X):
        from sradsgan_amd import ops
        assert ops.attention_variant_supported(X['u'], self.mode, P.get('fc1'), P.get('w7'))
        return ops.attention_variant(X['u'], X['skip'], self.mode, self.pool, P.get('fc1'), P.get('fc2'), P.get('w7'), None, None)

    def reference(self, A):
        from tests import attn_variants_ref as V
        t = self.t
        r64, r32 = (V.variant_grads(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], self.mode, self.pool, dtype=d) for d in (torch.float64, torch.float32))
        return {k: (r64['d' + k].reshape(p.shape), rel_tol(r64['d' + k], r32['d' + k])) for k, p in self.params.items()}


class Rab(Built):
    """rab_block.  One autograd node: its intermediates never leave it, so the plain run records the operands the block hands to its own
    stages (capture) and every stage is held to fp64 on THOSE: the tail's five parameters to attn_tail_ref on the block's u (arg-max
    indices asserted equal, margins asserted), the two 3x3 weight gradients to tests/conv_emulation.py on the block's (t, du) and (x, dt)
    -- on the plane path the decoded planes.  (The kernels that produce t, u, du, dt have tests of their own.)"""

    def __init__(self, row):
        super().__init__(row)
        n, c, h, w = row['shape']
        cm = row['cmid']
        g = _gen(row['id'], row['seed'])
        self.inputs = dict(x=_cl(_r(g, n, c, h, w)))
        self.t0 = dict(fc1=0.3 * _r(g, 4, c), fc2=0.3 * _r(g, c, 4), w7=0.2 * _r(g, 1, 2, 7, 7), wc=0.1 * _r(g, c, c, 1, 1), bc=0.1 * _r(g, c), hidden=4)
        self.params = dict(w1=_r(g, cm, c, 3, 3, scale=(9 * c) ** -0.5).to(DEV), b1=_r(g, cm, scale=0.1).to(DEV),
                           w2=_r(g, c, cm, 3, 3, scale=(9 * cm) ** -0.5).to(DEV), b2=_r(g, c, scale=0.1).to(DEV), **_tail_params(self.t0))
        self.gout = _cl(_r(g, n, c, h, w))
        self.seen = {}

    def check(self, lib, ops):
        super().check(lib, ops)
        want = self.row['route'] == 'planes'
        assert bool(ops.rab_planes_ok(self.inputs['x'], self.params['w1'], self.params['w2'])) == want, 'rab_planes_ok: the row has left its route'

    @contextlib.contextmanager
    def capture(self):
        """Records, while the plain run's backward runs, the operands of every weight gradient (by weight shape) and the tail's u and
        saved tensors."""
        from sradsgan_amd import ops
        real_w, real_t, seen = ops.wgrad_for_params, ops._tail_backward, self.seen

        def wgrad(w, b, x, dy, *a, **k):
            seen[tuple(w.shape)] = (x.detach().clone(), dy.detach().clone())
            return real_w(w, b, x, dy, *a, **k)

        def tail(g, u, fc1_w, fc2_w, w7, wc, bc, saved, *a, **k):
            seen['tail'] = (u.detach().clone(), [t.detach().clone() for t in saved])
            return real_t(g, u, fc1_w, fc2_w, w7, wc, bc, saved, *a, **k)
        ops.wgrad_for_params, ops._tail_backward = wgrad, tail
        try:
            yield
        finally:
            ops.wgrad_for_params, ops._tail_backward = real_w, real_t

    @contextlib.contextmanager
    def capture_planes(self):
        """Records the halves of the operands of every ops.wgrad_pp_for_params request (by weight shape), at the request: the pooled
        plane buffers go back to the pool once the launch is enqueued."""
        from sradsgan_amd import ops
        real, seen = ops.wgrad_pp_for_params, self.seen

        def wgrad_pp(w, b, x, dy, *a, **k):
            seen['pp', tuple(w.shape)] = (plane_halves(x), plane_halves(dy))
            return real(w, b, x, dy, *a, **k)
        ops.wgrad_pp_for_params = wgrad_pp
        try:
            yield
        finally:
            ops.wgrad_pp_for_params = real

    def plane_reference(self):
        """The references of the two 3x3 convs for the flat kernel: xh dyh + xh dyl + xl dyh in fp64 on the halves the planes hold (a
        plane's lo need not be the split of hi + lo's fp32 sum, which is all the plain run's decoded operand can tell); db from hi + lo."""
        out = {}
        for wk, bk in (('w2', 'b2'), ('w1', 'b1')):
            shape = tuple(self.params[wk].shape)
            (xh, xl), (yh, yl) = self.seen['pp', shape]
            wg = lambda a, b, **k: E.conv_wgrad(a, b, shape, 1, 1, 'fp32', **k)
            ref = wg(xh, yh, with_abs=False)[0] + wg(xh, yl, with_abs=False)[0] + wg(xl, yh, with_abs=False)[0]
            _, absref = wg(xh + xl, yh + yl)
            for name, (h, l) in (('x', (xh, xl)), ('dy', (yh, yl))):
                ch, cl = E.split_bf16((h + l).float())
                print('%s %s operand %s: %d of %d plane elements are not the split of their fp32 sum' % (
                    self.row['id'], wk, name, int(((ch != h) | (cl != l)).sum()), h.numel()))
            gb, ab = (yh + yl).sum((0, 2, 3)), (yh + yl).abs().sum((0, 2, 3))
            out[wk], out[bk] = (ref, conv_tol(ref, absref, 'bf16x3')), (gb, conv_tol(gb, ab, 'fp32'))
        return out

    def forward(self, P, X):
        from sradsgan_amd import ops
        return ops.rab_block(X['x'], *[P[k] for k in C.RAB_PARAMS])

    def reference(self, A):
        from tests import attn_tail_ref as AT
        p, x, arith = self.params, self.inputs['x'], self.row['arith']
        u, saved = self.seen['tail']
        td = dict(self.t0, u=u.cpu().contiguous(), skip=x.cpu().contiguous(), g=self.gout.cpu().contiguous(), family='normal',
                  exempt_p=torch.zeros(u.shape[0], AT.C, u.shape[2] * u.shape[3], dtype=torch.bool))
        td['exempt_c'] = td['exempt_p']
        AT.assert_margins(td, self.row['id'])
        arg, argc = _assert_indices(saved, td, self.row['id'])
        out, _ = _tail_reference(td, arg, argc, arith)
        for wk, bk in (('w2', 'b2'), ('w1', 'b1')):
            xo, go = self.seen[tuple(p[wk].shape)]
            ref, absref = E.conv_wgrad(xo, go, tuple(p[wk].shape), 1, 1, arith)
            gb, ab = go.double().sum((0, 2, 3)), go.double().abs().sum((0, 2, 3))
            out[wk], out[bk] = (ref, conv_tol(ref, absref, arith)), (gb, conv_tol(gb, ab, 'fp32'))
        assert torch.equal(self.seen[tuple(p['w1'].shape)][0], x), 'conv1\'s weight gradient reads the block input'
        return out


class Spectral(Built):
    """conv2d on the effective weight W = weight_bar / sigma of ops.spectral_weights; u and v restart from the same vectors in every run."""

    def __init__(self, row):
        super().__init__(row)
        from tests import spectral_ref as SR
        n, cin, h, w, cout = row['shape']
        g = _gen(row['id'])
        self.inputs = dict(x=_cl(_r(g, n, cin, h, w)))
        self.params = dict(wbar=_r(g, cout, cin, 3, 3, scale=0.02).to(DEV), b=_r(g, cout, scale=0.1).to(DEV))
        self.u0, self.v0 = SR.l2normalize(_r(g, cout)).to(DEV), SR.l2normalize(_r(g, cin * 9)).to(DEV)
        self.gout = _cl(_r(g, n, cout, h, w))
        self.last = None

    def forward(self, P, X):
        from sradsgan_amd import ops
        table = ops.SpectralTable([(P['wbar'], self.u0.clone(), self.v0.clone())])
        (W,) = ops.spectral_weights(table)
        assert not W.is_leaf
        W.retain_grad()
        self.last = (table, W)
        return ops.conv2d(X['x'], W, P['b'], 1, 1)

    def stage(self, run):
        """(weight_bar, dW as the conv delivered it, u, v, sigma as the pass left them) of one run, as matrices / vectors."""
        table, W = run.extra
        u, v, sigma = table.snapshot(table.last_out, 0)
        return self.params['wbar'].reshape(W.shape[0], -1), W.grad.reshape(W.shape[0], -1), u, v, sigma

    def reference(self, A):
        """Two stages: the conv's weight gradient at W (kept by retain_grad) against the emulation, then -- check_slot -- the projection
        of THAT gradient into weight_bar with the (u, v, sigma) the pass left, by the formula and under the bar of
        tests/test_spectral_gpu.py::test_projection_against_fp64."""
        _, W = A.extra
        arith = self.row['arith']
        ref, absref = E.conv_wgrad(self.inputs['x'], self.gout, tuple(W.shape), 1, 1, arith)
        E.assert_conv_close(W.grad, ref, absref, _tau(arith), what='spectral: dW of the conv on the effective weight')
        gb = self.gout.double().sum((0, 2, 3))
        return dict(b=(gb, conv_tol(gb, self.gout.double().abs().sum((0, 2, 3)), 'fp32')))

    def check_slot(self, what, run, G0):
        """weight_bar's .grad (prior G0, None: zeros) as tests/test_spectral_gpu.py checks a projected slot: its bar, on the slot's contents."""
        from tests.test_spectral_gpu import _bar
        w2, g2, u, v, sigma = self.stage(run)
        proj = lambda w, g, u, v, sg, s0: s0 + (g / sg - (g * w).sum() / (sg * sg) * torch.outer(u, v))      # noqa: E731
        s0 = torch.zeros_like(w2) if G0 is None else G0.reshape(w2.shape)
        exact = proj(w2.double(), g2.double(), u.double(), v.double(), sigma.double(), s0.double())
        bad = []
        _bar(what, run.grads['wbar'].reshape(w2.shape), proj(w2, g2, u, v, sigma, s0), exact, bad)
        assert not bad, bad


class Leaf(Built):
    """layer_norm, prelu, gamma_residual, ca_residual: their parameter gradients always go back to autograd."""

    def __init__(self, row):
        super().__init__(row)
        from tests import attn_kernels_ref as AK
        from tests import leaf_kernels_ref as L
        n, c, h, w = row['shape']
        op = self.op = row['op']
        img = lambda v: _cl(v.reshape(n, h, w, c).permute(0, 3, 1, 2))
        if op == 'layer_norm':
            self.inp = inp = AK.ln_inputs('random', n * h * w)
            self.inputs, self.gout = dict(x=img(inp['x'])), img(inp['dy'])
            self.params = dict(gamma=inp['gamma'].to(DEV), beta=inp['beta'].to(DEV))
        elif op == 'prelu':
            g, z = L.clean_rows(n * h * w, c)
            self.inp = dict(g=g, z=z)
            self.inputs, self.gout, self.params = dict(x=img(z)), img(g), dict(slope=torch.tensor([0.25], device=DEV))
        elif op == 'gamma_residual':
            a, b, g = (v.reshape(n * h * w, c) for v in L.gamma_inputs(n * h * w * c))
            self.inp = dict(b=b, g=g)
            self.inputs, self.gout, self.params = dict(x=img(a), b=img(b)), img(g), dict(gamma=torch.tensor([L.GAMMA], device=DEV))
            self.dx = ('x', 'b')
        else:
            t = L.ca_inputs(n, h * w)
            m = L.ca_mlp_inputs('mixed', n, 4, 1)
            self.inp = dict(u=t['u'], x=t['x'], g=t['g'], fc1=m['fc1'], b1=m['b1'], fc2=m['fc2'], b2=m['b2'])
            self.inputs, self.gout = dict(x=img(t['u']), res=img(t['x'])), img(t['g'])
            self.params = dict(fc1=m['fc1'].reshape(4, c, 1, 1).to(DEV), fc2=m['fc2'].reshape(c, 4, 1, 1).to(DEV), b1=m['b1'].to(DEV), b2=m['b2'].to(DEV))
            self.dx = ('x', 'res')

    def forward(self, P, X):
        from sradsgan_amd import ops
        if self.op == 'layer_norm':
            return ops.layer_norm(X['x'], P['gamma'], P['beta'])
        if self.op == 'prelu':
            return ops.prelu(X['x'], P['slope'])
        if self.op == 'gamma_residual':
            return ops.gamma_residual(X['x'], X['b'], P['gamma'])
        return ops.ca_residual(X['x'], X['res'], P['fc1'], P['fc2'], None, P['b1'], P['b2'])

    def reference(self, A):
        from tests import attn_kernels_ref as AK
        from tests import leaf_kernels_ref as L
        i, d64, d32 = self.inp, torch.float64, torch.float32
        if self.op == 'layer_norm':
            r64, r32 = AK.ln_eval(i, d64, False), AK.ln_eval(i, d32, False)
            return {k: (r64['d' + k], rel_tol(r64['d' + k], r32['d' + k])) for k in ('gamma', 'beta')}
        if self.op == 'prelu':
            return dict(slope=(L.prelu_slope_eval(i['g'], i['z'], d64), rel_tol(L.prelu_slope_eval(i['g'], i['z'], d64), L.prelu_slope_eval(i['g'], i['z'], d32))))
        if self.op == 'gamma_residual':
            return dict(gamma=(L.gamma_sum_eval(i['g'], i['b'], d64), rel_tol(L.gamma_sum_eval(i['g'], i['b'], d64), L.gamma_sum_eval(i['g'], i['b'], d32))))
        r64, r32 = (L.ca_chain_ref(i['u'], i['x'], i['fc1'], i['b1'], i['fc2'], i['b2'], i['g'], d) for d in (d64, d32))
        return {k: (r64[n].reshape(self.params[k].shape), rel_tol(r64[n], r32[n])) for k, n in (('fc1', 'dfc1'), ('fc2', 'dfc2'), ('b1', 'db1'), ('b2', 'db2'))}


class Dense(Built):
    def __init__(self, row):
        super().__init__(row)
        from tests import ndsrgan_ref as N
        n, c, h, w = row['shape']
        torch.manual_seed(zlib.crc32(row['id'].encode()))
        self.net = N.Dense()
        convs = [cl[0] for cl in self.net.CL_blocks] + [self.net.conv]
        g = _gen(row['id'])
        self.x0, self.g0 = _r(g, n, c, h, w), _r(g, n, c, h, w)
        self.inputs, self.gout = dict(x=_cl(self.x0)), _cl(self.g0)
        self.params = {}
        for i, cv in enumerate(convs, 1):
            self.params['w%d' % i], self.params['b%d' % i] = cv.weight.detach().clone().to(DEV), cv.bias.detach().clone().to(DEV)
        self.convs = convs

    def forward(self, P, X):
        from sradsgan_amd import ops
        return ops.dense_block(X['x'], [P[k] for k in self.params])

    def reference(self, A):
        import copy
        out = {}
        runs = []
        for d in (torch.float64, torch.float32):
            net = copy.deepcopy(self.net).to(d)
            net(self.x0.to(d)).backward(self.g0.to(d))
            convs = [cl[0] for cl in net.CL_blocks] + [net.conv]
            runs.append({('%s%d' % (k, i)): getattr(cv, a).grad for i, cv in enumerate(convs, 1) for k, a in (('w', 'weight'), ('b', 'bias'))})
        for k in self.params:
            out[k] = (runs[0][k], rel_tol(runs[0][k], runs[1][k]))
        return out


BUILDERS = dict(conv=Conv, norm=Norm, gam=Gam, tail=Tail, variant=Variant, rab=Rab, spectral=Spectral, leaf=Leaf, dense=Dense)


# ================================================================================================================================ #
# runs
# ================================================================================================================================ #
class Run:
    def __init__(self, P, X, y, fired, extra):
        self.P, self.X, self.y, self.fired, self.extra = P, X, y, fired, extra
        self.grads = {k: p.grad for k, p in P.items()}
        self.dx = {k: x.grad for k, x in X.items()}


def prior(built, tag='G0'):
    """A random non-zero prior per parameter (fixed seed)."""
    g = _gen(built.row['id'], tag)
    return {k: _r(g, *p.shape).to(DEV) for k, p in built.params.items()}


def leaves(built, G0=None, none=()):
    fired = {k: 0 for k in built.params}
    P = {}
    for k, v in built.params.items():
        p = v.clone().requires_grad_()
        p.register_hook(lambda g, k=k: fired.__setitem__(k, fired[k] + (g is not None)))      # autograd was handed a gradient for this leaf (None: the op kept it)
        if G0 is not None and k not in none:
            p.grad = G0[k].clone()
        P[k] = p
    X = {k: v.clone().requires_grad_(k in built.dx) for k, v in built.inputs.items()}
    return P, X, fired


@contextlib.contextmanager
def delivery(ctx):
    """direct_param_grads of one of C.CONTEXTS (None: no context); the side stream is fresh, and joined before anything is read."""
    from sradsgan_amd import ops
    if ctx is None:
        yield None
        torch.cuda.synchronize()
        return
    _, side, group = ctx
    S = torch.cuda.Stream() if side else None
    if S is not None:
        S.wait_stream(torch.cuda.current_stream())
    with ops.direct_param_grads(S, group=group):
        yield S
    if S is not None:
        torch.cuda.current_stream().wait_stream(S)
    torch.cuda.synchronize()


def run(built, ctx=None, G0=None, none=(), scope=None, inputs_only=False):
    """inputs_only: backward(inputs = the data inputs), as TrainStep asks for the generator's gradients through the discriminator: autograd
    then drops every parameter gradient an op RETURNS, and only what an op writes into a slot itself can reach a .grad."""
    from sradsgan_amd import ops
    P, X, fired = leaves(built, G0, none)
    with ops.conv_math(built.row['math']), delivery(ctx):
        with (scope(P, X) if scope is not None else contextlib.nullcontext()):
            y = built.forward(P, X)
            if inputs_only:
                torch.autograd.backward(y, built.gout, inputs=[X[k] for k in built.dx])
            else:
                y.backward(built.gout)
    return Run(P, X, y.detach(), fired, getattr(built, 'last', None))


_CACHE = {}


def case(rid):
    """(built, plain run A, reference) of a row: computed once, shared by every test, never changed."""
    if rid not in _CACHE:
        from sradsgan_amd import ops
        row = C.BY_ID[rid]
        built = BUILDERS[row['build']](row)
        with ops.conv_math(row['math']):
            built.check(_lib(), ops)
            with getattr(built, 'capture', contextlib.nullcontext)():
                A = run(built)
            ref = built.reference(A)
        _CACHE[rid] = (built, A, ref)
    return _CACHE[rid]


def _worst(got, ref, tol):
    """largest |got - ref| / tol; tol a float or a tensor."""
    d = (got.detach().double().to(ref.device) - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=ref.device)
    r = torch.nan_to_num(d / tol, nan=float('inf'))
    return float(r.max())


def check_close(what, got, ref, tol, bad):
    ref = ref.to(got.device) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    ratio = _worst(got, ref, tol)
    print('%-64s err / bar %.3f%s' % (what, ratio, '' if ratio <= 1 else '   <-- FAIL'))
    if not ratio <= 1:
        bad.append((what, ratio))


def with_prior(ref, tol, G0, roundings=1):
    """(G0 + reference, bar + `roundings` fp32 roundings of |G0 + g|)."""
    tot = G0.double().to(ref.device) + ref if isinstance(ref, torch.Tensor) else G0.double() + ref
    tol = torch.as_tensor(tol, dtype=torch.float64, device=tot.device)
    return tot, tol + roundings * U * tot.abs()


# ================================================================================================================================ #
# A and B, row by row
# ================================================================================================================================ #
ROW_PARAMS = [pytest.param(r['id'], id=r['id']) for r in C.ROWS]


@pytest.mark.parametrize('rid', ROW_PARAMS)
def test_plain_run_against_the_fp64_reference(rid):
    built, A, ref = case(rid)
    row, bad = built.row, []
    assert set(ref) | ({'wbar'} if row['build'] == 'spectral' else set()) == set(built.params), 'a parameter without a reference'
    assert all(n == 1 for n in A.fired.values()), 'plain mode: every parameter gradient goes through autograd once: %s' % A.fired
    for k, (r, tol) in ref.items():
        check_close('%s plain %s' % (rid, k), A.grads[k], r, tol, bad)
    if row['build'] == 'spectral':
        built.check_slot('%s plain wbar' % rid, A, None)
    for k in built.dx:
        assert A.dx[k] is not None and bool(torch.isfinite(A.dx[k]).all())
    assert not bad, bad


@pytest.mark.parametrize('ctx', C.CONTEXTS, ids=[c[0] for c in C.CONTEXTS])
@pytest.mark.parametrize('rid', ROW_PARAMS)
def test_delivery_into_the_slots(rid, ctx):
    built, A, ref = case(rid)
    row, bad = built.row, []
    G0 = prior(built)
    planes = row['route'] == 'planes'
    with (built.capture_planes() if planes else contextlib.nullcontext()):
        B = run(built, ctx, G0)
    if planes:                                                          # what the flat kernel was handed, half by half
        ref = dict(ref, **built.plane_reference())
    for k in built.params:
        slot = k in row['slots']
        assert B.fired[k] == (0 if slot else 1), '%s %s: autograd saw %d gradient(s) for a parameter that %s a slot' % (rid, k, B.fired[k], 'uses' if slot else 'has no')
        assert B.P[k].grad.data_ptr() == B.grads[k].data_ptr()
        if k in row['exact']:
            same = torch.equal(B.grads[k], G0[k] + A.grads[k])
            print('%-64s fp32(G0 + g_A) bit for bit: %s' % ('%s %s %s' % (rid, ctx[0], k), same))
            if not same:
                bad.append((k, 'bits', float((B.grads[k] - (G0[k] + A.grads[k])).abs().max())))
        if k in ref:
            tot, tol = with_prior(ref[k][0], ref[k][1], G0[k])
            check_close('%s %s %s' % (rid, ctx[0], k), B.grads[k], tot, tol, bad)
    if row['build'] == 'spectral':
        built.reference(B)                                              # this run's own dW against the emulation
        built.check_slot('%s %s wbar' % (rid, ctx[0]), B, G0['wbar'])
    assert row['dx'] == 'bits'
    for k in built.dx:
        assert torch.equal(B.dx[k], A.dx[k]), '%s %s: the data gradient at %s differs from the plain run' % (rid, ctx[0], k)
    assert not bad, bad


MIXED = [pytest.param(r['id'], id=r['id']) for r in C.ROWS if r['pair']]


@pytest.mark.parametrize('rid', MIXED)
def test_mixed_slots_fall_back_on_autograd_for_both(rid):
    """One parameter of the pair owns a dense .grad and the other has none (and the reverse): no slot is used, both totals arrive through
    autograd -- the prior plus the plain run's gradient in one in-place add, and the plain run's gradient itself."""
    built, A, ref = case(rid)
    G0 = prior(built)
    for missing in built.row['pair']:
        B = run(built, C.CONTEXTS[2], G0, none=(missing,))
        for k in built.row['pair']:
            assert B.fired[k] == 1, (rid, missing, k, B.fired)
            want = A.grads[k] if k == missing else G0[k] + A.grads[k]
            assert torch.equal(B.grads[k], want), '%s without a .grad for %s: %s is off by %.3e' % (rid, missing, k, float((B.grads[k] - want).abs().max()))
        for k in built.dx:
            assert torch.equal(B.dx[k], A.dx[k])


# ================================================================================================================================ #
# one parameter, two uses; odd partner counts; ageing
# ================================================================================================================================ #
SQUARE = (4, 128, 19, 27, 128)         # GROUPED_SHAPE with as many input as output channels: conv(lrelu(conv(x))) with ONE weight


def _launches(ops):
    """Records the job lists of _WgradQueue.run_fp32 / run_planes while they run for real."""
    log = []
    real = (ops._WgradQueue.run_fp32, ops._WgradQueue.run_planes)

    def fp32(self, jobs):
        log.append(('fp32', [j.gw.data_ptr() for j in jobs]))
        return real[0](self, jobs)

    def planes(self, jobs):
        log.append(('planes', [j.gw.data_ptr() for j in jobs]))
        return real[1](self, jobs)
    return log, real, (fp32, planes)


@contextlib.contextmanager
def recorded():
    from sradsgan_amd import ops
    log, real, fake = _launches(ops)
    ops._WgradQueue.run_fp32, ops._WgradQueue.run_planes = fake
    try:
        yield log
    finally:
        ops._WgradQueue.run_fp32, ops._WgradQueue.run_planes = real


def test_one_weight_used_twice_in_one_graph():
    """y = conv(lrelu(conv(x, w, b)), w, b) under (side, group 2): both requests have one key AND one slot.  Together in one grouped
    launch their reduces would race on it; the queue sends the first out before it takes the second.  Both contributions must be in
    w.grad / b.grad on top of the prior.  (Run once: tests/test_grad_delivery_cpu.py is the deterministic check of the pairing.)"""
    from sradsgan_amd import ops
    n, c, h, w, _ = SQUARE
    assert _lib().srhip_conv2d_wgrad_multi_ok(n, h, w, c, c, 3, 3, 1, 1) >= 2 and _lib().srhip_conv2d_wgrad_can_accumulate(c, c, 3, 3)
    row = dict(C.BY_ID['conv-grouped'], id='two-uses', slope=None)
    cv = Conv(row, shape=SQUARE)
    G0 = prior(cv)
    P, X, fired = leaves(cv, G0)
    with recorded() as log, delivery(C.CONTEXTS[2]):
        y1 = ops.conv2d(X['x'], P['w'], P['b'], 1, 1, act_slope=0.2)
        y2 = ops.conv2d(y1, P['w'], P['b'], 1, 1)
        y2.backward(cv.gout)
    assert [len(l[1]) for l in log] == [1, 1] and fired == dict(w=0, b=0), (log, fired)
    with torch.no_grad():
        g1 = ops.lrelu_bwd_raw(ops.conv2d_dgrad_raw(cv.gout, P['w'].detach(), tuple(y1.shape), 1, 1), y1.detach(), 0.2)
    r2, r1 = cv.wgrad_ref(y1.detach(), cv.gout), cv.wgrad_ref(X['x'].detach(), g1)
    bad, tol_w = [], None
    for k in ('w', 'b'):
        tot, tol = with_prior(r1[k][0] + r2[k][0], r1[k][1] + r2[k][1], G0[k], roundings=2)
        check_close('two uses in one graph %s' % k, P[k].grad, tot, tol, bad)
        tol_w = tol if k == 'w' else tol_w
    lone, _ = with_prior(r2['w'][0], 0.0, G0['w'])
    assert _worst(P['w'].grad, lone, tol_w) > 100, 'the check could not tell a lost contribution'
    assert not bad, bad


def test_one_conv_in_two_successive_backward_calls_of_one_context():
    """TrainStep._backward_terms: one backward per term of the discriminator's loss inside ONE context, so the real and the fake pass
    ask for the same slots one after the other and the queue outlives both."""
    from sradsgan_amd import ops
    row = dict(C.BY_ID['conv-grouped'], id='two-terms')
    a, b = Conv(row, tag=1), Conv(row, tag=2)
    G0 = prior(a)
    P, X, fired = leaves(a, G0)
    xb = b.inputs['x'].clone()
    with recorded() as log, delivery(C.CONTEXTS[2]):
        ya, yb = ops.conv2d(X['x'], P['w'], P['b'], 1, 1), ops.conv2d(xb, P['w'], P['b'], 1, 1)
        for y, g in ((ya, a.gout), (yb, b.gout)):
            torch.autograd.backward(y, g, inputs=[P['w'], P['b']])
    assert [len(l[1]) for l in log] == [1, 1] and fired == dict(w=0, b=0), (log, fired)
    ra, rb = a.wgrad_ref(a.inputs['x'], a.gout), a.wgrad_ref(xb, b.gout)
    bad = []
    for k in ('w', 'b'):
        tot, tol = with_prior(ra[k][0] + rb[k][0], ra[k][1] + rb[k][1], G0[k], roundings=2)
        check_close('two backward calls, one context %s' % k, P[k].grad, tot, tol, bad)
    assert not bad, bad


def test_three_partners_under_group_two():
    """Three convs of one shape, three weights: two leave in one grouped launch, the third alone when the context ends."""
    from sradsgan_amd import ops
    row = C.BY_ID['conv-grouped']
    cvs = [Conv(dict(row, id='three'), tag=i) for i in range(3)]
    sets = [leaves(cv, prior(cv, 'G0-%d' % i)) for i, cv in enumerate(cvs)]
    with recorded() as log, delivery(C.CONTEXTS[2]):
        ys = [ops.conv2d(X['x'], P['w'], P['b'], 1, 1) for P, X, _ in sets]
        torch.autograd.backward(ys, [cv.gout for cv in cvs])
    assert sorted(len(l[1]) for l in log) == [1, 2], log
    bad = []
    for i, (cv, (P, X, fired)) in enumerate(zip(cvs, sets)):
        ref = cv.wgrad_ref(cv.inputs['x'], cv.gout)
        G0 = prior(cv, 'G0-%d' % i)
        for k in ('w', 'b'):
            tot, tol = with_prior(ref[k][0], ref[k][1], G0[k])
            check_close('three partners: conv %d %s' % (i, k), P[k].grad, tot, tol, bad)
        assert fired == dict(w=0, b=0)
    assert not bad, bad


def test_four_plane_requests_under_the_plane_group():
    """ops.wgrad_pp_for_params, four requests of one shape: _PP_GROUP = 3 leave together, the fourth with the flush."""
    from sradsgan_amd import ops
    row = C.BY_ID['rab-planes']
    n, c, h, w = row['shape']
    shape = (n, c, h, w, row['cmid'])
    assert ops._PP_GROUP == 3 and _lib().srhip_conv2d_wgrad_pp_ok(n, h, w, c, row['cmid']) & 4
    cvs = [Conv(dict(C.BY_ID['conv-grouped'], id='four-planes'), tag=i, shape=shape) for i in range(4)]
    sets = [leaves(cv, prior(cv, 'G0-%d' % i)) for i, cv in enumerate(cvs)]
    with recorded() as log, delivery(C.CONTEXTS[2]):
        for cv, (P, X, _) in zip(cvs, sets):
            assert ops.wgrad_pp_for_params(P['w'], P['b'], cv.inputs['x'], cv.gout, True) is True
    assert [(l[0], len(l[1])) for l in log] == [('planes', 3), ('planes', 1)], log
    bad = []
    for i, (cv, (P, X, _)) in enumerate(zip(cvs, sets)):
        ref = cv.wgrad_ref(cv.inputs['x'], cv.gout)
        G0 = prior(cv, 'G0-%d' % i)
        for k in ('w', 'b'):
            tot, tol = with_prior(ref[k][0], ref[k][1], G0[k])
            check_close('four plane requests: conv %d %s' % (i, k), P[k].grad, tot, tol, bad)
    assert not bad, bad


def test_a_request_without_a_partner_ages_out_and_is_right():
    """One grouped-eligible conv, then more than _WGRAD_MAX_AGE requests of another shape: the conv leaves alone from tick(), before the
    context ends, and its slot is right; so are the first and the last of the others."""
    from sradsgan_amd import ops
    big = Conv(dict(C.BY_ID['conv-grouped'], id='aged'))
    small = [Conv(dict(C.BY_ID['conv-accumulate'], id='ager', slope=None), tag=i) for i in range(ops._WGRAD_MAX_AGE + 1)]
    sets = [leaves(cv, prior(cv)) for cv in [big] + small]
    with recorded() as log, delivery(C.CONTEXTS[2]):
        ys = [ops.conv2d(X['x'], P['w'], P['b'], 1, 1) for P, X, _ in sets]
        ys[0].backward(big.gout)
        assert len(ops._state.wgrads.pending) == 1 and not log
        for y, cv in zip(ys[1:], small):
            y.backward(cv.gout)
        assert not ops._state.wgrads.pending and [len(l[1]) for l in log] == [1], 'the conv must have left from tick(): %s' % log
    bad = []
    for cv, (P, X, _) in ((big, sets[0]), (small[0], sets[1]), (small[-1], sets[-1])):
        ref, G0 = cv.wgrad_ref(cv.inputs['x'], cv.gout), prior(cv)
        for k in ('w', 'b'):
            tot, tol = with_prior(ref[k][0], ref[k][1], G0[k])
            check_close('ageing: %s %s' % (cv.row['id'], k), P[k].grad, tot, tol, bad)
    assert not bad, bad


# ================================================================================================================================ #
# pruning
# ================================================================================================================================ #
PRUNED = ('conv-accumulate', 'conv-add-3to64', 'conv-pool', 'rab-fp32', 'rab-planes', 'attention-tail', 'variant-clam', 'variant-slam', 'cgam', 'sgam',
          'batch-norm', 'group-norm-affine')
STOPS = {'conv-accumulate', 'conv-add-3to64'}          # the rows whose op reads stop_ids: conv2d's backward is the only reader


def _bits(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@pytest.mark.parametrize('rid', PRUNED)
def test_skip_params_keeps_the_listed_parameters_untouched(rid):
    """The G step's pattern: backward(inputs = data inputs only) through a discriminator whose parameters own slots.  autograd drops
    whatever an op returns for a parameter, but a slot is written behind autograd's back -- so WITHOUT the scope every slot receives its
    gradient, and backward_scope(skip_params=[first parameter]) must keep every slot of the op at G0 bit for bit (an op prunes all its
    parameter gradients when one of them is listed: a conv's bias goes with its weight, a norm's beta with its gamma, a fused block's
    parameters together).  dx is the unpruned run's bit for bit; a list that names none of the op's parameters prunes nothing; the same
    graph rebuilt without the scope gives the full gradients again."""
    from sradsgan_amd import ops
    built, A, ref = case(rid)
    G0 = prior(built)
    ctx = C.CONTEXTS[0]
    full = run(built, ctx, G0)
    unpruned = run(built, ctx, G0, inputs_only=True)
    for k in built.row['slots']:
        assert torch.equal(unpruned.grads[k], full.grads[k]), '%s: slot %s is written whatever autograd was asked for' % (rid, k)
    first = next(iter(built.params))
    pruned = run(built, ctx, G0, inputs_only=True, scope=lambda P, X: ops.backward_scope(skip_params=[P[first]]))
    for k in built.params:
        assert torch.equal(pruned.grads[k], G0[k]) and pruned.fired[k] == 0, '%s: %s changed under skip_params=[%s]' % (rid, k, first)
    for k in built.dx:
        assert torch.equal(pruned.dx[k], full.dx[k]) and torch.equal(pruned.dx[k], A.dx[k])
    assert ops._state.skip_ids == frozenset()
    again = run(built, ctx, G0)
    assert all(torch.equal(again.grads[k], full.grads[k]) for k in built.params) and all(torch.equal(again.dx[k], full.dx[k]) for k in built.dx)
    other = run(built, ctx, G0, inputs_only=True, scope=lambda P, X: ops.backward_scope(skip_params=[torch.zeros(1, device=DEV)]))
    assert all(torch.equal(other.grads[k], unpruned.grads[k]) for k in built.params), 'a list that names none of the parameters pruned something'


@pytest.mark.parametrize('rid', PRUNED)
def test_no_param_grads_changes_no_slot(rid):
    """The penalty's first-order pass: autograd.grad with respect to the data input only, inside no_param_grads()."""
    from sradsgan_amd import ops
    built, A, ref = case(rid)
    G0 = prior(built)
    for ctx in (C.CONTEXTS[0], C.CONTEXTS[2]):
        pruned = run(built, ctx, G0, inputs_only=True, scope=lambda P, X: ops.no_param_grads())
        for k in built.params:
            assert torch.equal(pruned.grads[k], G0[k]) and pruned.fired[k] == 0, '%s: %s changed under no_param_grads()' % (rid, k)
        for k in built.dx:
            assert torch.equal(pruned.dx[k], A.dx[k])
        assert ops._state.skip_param_grads is False
    again, full = run(built, C.CONTEXTS[0], G0), run(built, C.CONTEXTS[0], G0)
    assert all(torch.equal(again.grads[k], full.grads[k]) and not torch.equal(again.grads[k], G0[k]) for k in built.params)


@pytest.mark.parametrize('alias', [False, True], ids=['same-tensor', 'detached-alias'])
@pytest.mark.parametrize('rid', PRUNED)
def test_stop_at_cuts_the_data_gradient_of_a_conv_by_address(rid, alias):
    """stop_at=(x,) matches by data_ptr(): conv2d's backward -- the only reader -- computes no gradient for an input at that address,
    also when the op was fed x.detach().requires_grad_() (how TrainStep hands gen_hr to the discriminator); every other op's data
    gradient, and every parameter gradient, is the unpruned run's bit for bit."""
    from sradsgan_amd import ops
    built, A, ref = case(rid)
    if not built.dx:
        return
    G0 = prior(built)
    ctx = C.CONTEXTS[0]
    full = run(built, ctx, G0)
    name = built.dx[0]
    P, X, fired = leaves(built, G0)
    listed = X[name]
    if alias:
        X[name] = listed.detach().requires_grad_()
        assert X[name].data_ptr() == listed.data_ptr() and X[name] is not listed
    with ops.conv_math(built.row['math']), delivery(ctx), ops.backward_scope(stop_at=(listed,)):
        built.forward(P, X).backward(built.gout)
    torch.cuda.synchronize()
    if rid in STOPS:
        assert X[name].grad is None and listed.grad is None, '%s: a gradient reached the tensor listed in stop_at' % rid
    else:
        assert torch.equal(X[name].grad, full.dx[name])
    for k in built.dx[1:]:
        assert torch.equal(X[k].grad, full.dx[k])
    for k in built.params:
        assert torch.equal(P[k].grad, full.grads[k]), (rid, k)
    assert ops._state.stop_ids == frozenset()
    again = run(built, ctx, G0)
    assert all(torch.equal(again.dx[k], full.dx[k]) for k in built.dx)


def test_stop_at_leaves_a_second_input_at_another_address_alone():
    """conv2d with a fused residual: the input is cut, the residual at another address still gets its gradient (the upstream one)."""
    from sradsgan_amd import ops
    built, A, ref = case('conv-add-64to3')
    P, X, _ = leaves(built, prior(built))
    res = torch.zeros_like(built.gout).requires_grad_()
    with delivery(C.CONTEXTS[0]), ops.backward_scope(stop_at=(X['x'],)):
        ops.conv2d(X['x'], P['w'], P['b'], 1, 1, residual=res).backward(built.gout)
    assert X['x'].grad is None and torch.equal(res.grad, built.gout)
    with delivery(C.CONTEXTS[0]), ops.backward_scope(stop_at=(res,)):
        ops.conv2d(X['x'], P['w'], P['b'], 1, 1, residual=res).backward(built.gout)
    assert torch.equal(X['x'].grad, A.dx['x']), 'a residual listed in stop_at is no conv input: the cut is for the address of x'


# ================================================================================================================================ #
# carry_open: the two branches tests/test_model_gpu.py leaves out
# ================================================================================================================================ #
def _group():
    from sradsgan_amd import model as M
    torch.manual_seed(5)
    grp = M.ResGroup(M.RAB, n_blocks=1).to(DEV)
    g = _gen('carry')
    return grp, _cl(_r(g, 1, 64, 12, 12)), _cl(_r(g, 1, 64, 12, 12))


def _group_grads(grp, x0, gout, carry=True, differentiable=False):
    from sradsgan_amd import ops
    old, ops._CARRY = ops._CARRY, carry
    try:
        for p in grp.parameters():
            p.grad = None
        x = x0.clone().requires_grad_()
        y = grp(x * 1.0)
        if differentiable:
            (dx,) = torch.autograd.grad(y, x, gout, create_graph=True)
        else:
            y.backward(gout)
            dx = x.grad
        torch.cuda.synchronize()
        return dx.detach().clone()
    finally:
        ops._CARRY = old


def test_a_differentiable_backward_hands_the_carried_gradient_to_autograd():
    """A consumer that committed at forward time runs its backward under torch.enable_grad() (create_graph): it must not stash -- autograd
    has to see the edge -- and must take its commitment back, so that the RAB's count of stashes against commitments still balances."""
    from sradsgan_amd import ops
    from tests.test_model_gpu import _close
    grp, x0, gout = _group()
    ops._state.carry, ops._state.carry_expect = {}, {}
    t0 = ops._state.carry_token
    dx = _group_grads(grp, x0, gout, differentiable=True)
    assert ops._state.carry_token > t0, 'the group did not open a carry: the test would check nothing'
    assert not ops._state.carry and not ops._state.carry_expect, 'a stash or a commitment was left behind'
    plain = _group_grads(grp, x0, gout, carry=False)
    _close(dx.cpu(), plain.cpu(), tol=1e-5, msg='dx of the differentiable backward')
    assert torch.equal(dx, _group_grads(grp, x0, gout, carry=False, differentiable=True)), 'the same kernels as with the mechanism off'


def test_tokens_of_a_forward_without_a_backward_do_not_reach_the_next_graph():
    from sradsgan_amd import ops
    grp, x0, gout = _group()
    ops._state.carry, ops._state.carry_expect = {}, {}
    clean = _group_grads(grp, x0, gout)
    assert not ops._state.carry and not ops._state.carry_expect
    stale = grp(x0.clone().requires_grad_() * 1.0)                    # commits, never runs a backward
    assert len(ops._state.carry_expect) >= 1 and not ops._state.carry
    left = dict(ops._state.carry_expect)
    dx = _group_grads(grp, x0, gout)
    assert torch.equal(dx, clean)
    assert ops._state.carry_expect == left and not ops._state.carry, 'the new graph consumed exactly its own tokens'
    del stale
    ops._state.carry.clear(); ops._state.carry_expect.clear()
