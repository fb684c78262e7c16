"""Geometric self-ensemble ("+" inference; Lim et al., EDSR, CVPRW 2017, section 4.3; the evaluation protocol of EDSR, RCAN and
the HAT family): the generator runs on the eight dihedral views of the LR image, every output is mapped back and the eight are
averaged.  The views and the merge are HIP kernels (csrc/augment.hip); everything between them is the generator.

Ops are numbered as in include/sradsgan_hip.h and data.DIHEDRAL_OP: bit 0 transpose, bit 1 flip top-bottom, bit 2 flip left-right,
applied in that order.  The merged value is (((v_0 + v_1) + v_2) + ...) * (1 / m) in fp32, views in the order of `ops`, each read
through the inverse of its op: one pass, fixed order, so two runs give the same bits.

A transposing view of an h x w input is w x h, so the views go through the generator in two stacks unless `chunk` says
otherwise.  Stacking changes the batch size the generator sees, and with it the tiling its convolutions choose: a stacked run
agrees with a view-by-view run (chunk=1) to rounding, not bit for bit."""
import ctypes
import operator

import torch

from . import _hip

N_OPS = 8


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require(t, what):
    if not (torch.is_tensor(t) and t.dim() == 4 and t.dtype == torch.float32):
        raise TypeError('%s expects a float32 [N, C, H, W] tensor' % what)
    if not t.is_cuda:
        raise RuntimeError('%s: runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback' % (what, t.device.type))


def _strides(t):
    return (ctypes.c_long * 4)(*t.stride())


def _check_op(op, what):
    try:
        value = operator.index(op)
    except TypeError:
        value = -1
    if not 0 <= value < N_OPS:
        raise ValueError('%s: op must be an integer in 0..7, got %r' % (what, op))
    return value


def _empty_like_format(x, shape):
    channels_last = x.shape[1] > 1 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    return torch.empty(shape, device=x.device, dtype=torch.float32,
                       memory_format=torch.channels_last if channels_last else torch.contiguous_format)


def dihedral(x, op):
    """op applied to the last two axes of x [N, C, H, W] (float32 on the device, any strides: NCHW-dense and channels_last are
    read as they are).  Returns a new tensor in x's memory format, [N, C, W, H] for a transposing op."""
    _require(x, 'dihedral')
    op = _check_op(op, 'dihedral')
    if any(s < 0 for s in x.stride()) or x.numel() == 0:
        raise ValueError('dihedral: needs a non-empty tensor with non-negative strides')
    n, c, h, w = x.shape
    y = _empty_like_format(x, (n, c, w, h) if op & 1 else (n, c, h, w))
    _hip.check(_hip.lib().srhip_dihedral_f32(_p(x), _strides(x), _p(y), _strides(y), n, c, h, w, op, _stream()), 'dihedral_f32')
    return y


def merge(views, ops):
    """views[k] = a tensor of the shape of ops[k] applied to the result [N, C, H, W] (float32 on the device, any strides).  Returns
    (((inv_0(v_0) + inv_1(v_1)) + ...) + inv_{m-1}(v_{m-1})) * (1 / m), inv_k undoing ops[k], fp32 in index order."""
    views, ops = list(views), [_check_op(op, 'merge') for op in ops]
    m = len(views)
    if not 1 <= m <= N_OPS or len(ops) != m:
        raise ValueError('merge: takes 1..8 views and as many ops, got %d views and %d ops' % (m, len(ops)))
    for v in views:
        _require(v, 'merge')
    n, c, a, b = views[0].shape
    h, w = (b, a) if ops[0] & 1 else (a, b)
    for v, op in zip(views, ops):
        want = (n, c, w, h) if op & 1 else (n, c, h, w)
        if tuple(v.shape) != want or any(s < 0 for s in v.stride()) or v.device != views[0].device:
            raise ValueError('merge: the view of op %d must be %s on %s, got %s' % (op, want, views[0].device, tuple(v.shape)))
    out = _empty_like_format(views[0], (n, c, h, w))
    ptrs = (ctypes.c_void_p * m)(*[v.data_ptr() for v in views])
    strides = (ctypes.c_long * (4 * m))(*[s for v in views for s in v.stride()])
    _hip.check(_hip.lib().srhip_ensemble_merge_f32(ptrs, strides, (ctypes.c_int * m)(*ops), m, _p(out), _strides(out), n, c, h, w,
                                                   _stream()), 'ensemble_merge_f32')
    return out


def self_ensemble(generator, lr, ops=range(N_OPS), chunk=None):
    """The average of generator(op(lr)) mapped back, over `ops` (distinct, in this order; all eight by default), under no_grad.
    chunk: how many views of one shape are stacked along the batch axis per generator call; None = all non-transposing views
    in one call and all transposing ones in another.  The generator is used as it is (call .eval() yourself)."""
    ops = [_check_op(op, 'self_ensemble') for op in ops]
    if not ops or len(set(ops)) != len(ops):
        raise ValueError('self_ensemble: ops must be a non-empty list of distinct ops, got %r' % (ops,))
    if chunk is not None and int(chunk) < 1:
        raise ValueError('self_ensemble: chunk must be at least 1, got %r' % (chunk,))
    _require(lr, 'self_ensemble')
    n = lr.shape[0]
    with torch.no_grad():
        outs = [None] * len(ops)
        for transposing in (0, 1):
            idx = [k for k, op in enumerate(ops) if op & 1 == transposing]
            step = len(idx) if chunk is None else int(chunk)
            for c0 in range(0, len(idx), max(step, 1)):
                part = idx[c0:c0 + step]
                views = [lr if ops[k] == 0 else dihedral(lr, ops[k]) for k in part]
                sr = generator(views[0] if len(part) == 1 else torch.cat(views, dim=0))
                if not (torch.is_tensor(sr) and sr.dim() == 4 and sr.shape[0] == n * len(part)):
                    raise ValueError('self_ensemble: the generator must return [N, C, H, W] for every input row')
                for q, k in enumerate(part):
                    outs[k] = sr[q * n:(q + 1) * n]
        return merge(outs, ops)


class SelfEnsemble(torch.nn.Module):
    """generator -> the module whose forward is self_ensemble(generator, lr, ops, chunk): goes wherever a generator goes
    (validate.evaluate, scene.super_resolve_scene, classify.classify_sr, the trainers' mfe_test_single)."""

    def __init__(self, generator, ops=range(N_OPS), chunk=None):
        super().__init__()
        self.generator, self.ops, self.chunk = generator, list(ops), chunk

    def forward(self, lr):
        return self_ensemble(self.generator, lr, self.ops, self.chunk)
