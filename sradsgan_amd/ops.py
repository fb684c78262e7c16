"""torch.autograd wrappers over the C ABI (include/sradsgan_hip.h).

Every op here replaces an ATen call the reference makes implicitly through torch.nn
(SRADSGAN/model/sradsgan.py:35-508).  Activations are NHWC in memory (torch `channels_last`
tensors keep the reference's logical NCHW shape at the module boundary); parameters stay OIHW so
state_dicts stay interchangeable.  All backward passes are themselves built from these Functions,
so the discriminator can be differentiated twice (gradient penalty, sradsgan.py:621,639).

No CPU path exists: a CPU tensor raises.
"""
import contextlib
import ctypes
import os
import threading
import weakref
from typing import NamedTuple

import torch
from torch.autograd import Function

from . import _hip

EPI_BIAS, EPI_LRELU, EPI_RESIDUAL, EPI_ROWSCALE, EPI_CHANSCALE, EPI_GRADDATA = 1, 2, 4, 8, 16, 64
CL = torch.channels_last

class _State:
    # a plain global, not threading.local: autograd runs Function.backward on its own device thread
    skip_param_grads = False
    wgrads = None                   # the _WgradQueue of the running direct_param_grads() context (None outside one)
    skip_ids = frozenset()          # id()s of parameters whose gradients the current backward must not produce
    stop_ids = frozenset()          # data_ptr()s of tensors the current backward must not propagate into
    capturing = False               # a stream capture is being recorded (TrainStep._capture): side-stream forks go through torch events
    last_out_pp = None              # _RabBlock.forward -> rab_block(): the output's padded planes (emit_pp)
    carry = None                    # token -> [gradients stashed for a block input by its other consumers] (carry_open)
    carry_expect = None             # token -> number of consumers that committed to stash at forward time
    carry_token = 0


_state = _State()


def _skip_param_grads(*params):
    """True when the running backward must not produce gradients for these parameters."""
    if _state.skip_param_grads:
        return True
    return bool(_state.skip_ids) and any(p is not None and id(p) in _state.skip_ids for p in params)


@contextlib.contextmanager
def backward_scope(skip_params=(), stop_at=()):
    """Prunes a backward pass that autograd cannot prune inside custom Functions: parameters listed in
    `skip_params` get no weight gradient (their wgrad kernels are not launched), and the data gradient
    is not propagated into the tensors listed in `stop_at`.  `skip_params` match by identity, and an op decides once per node: a
    listed parameter prunes every slot write of its op (a conv's bias with its weight, a norm's beta with its gamma, the parameters
    of a fused block together); what an op returns to autograd instead is autograd's to drop (backward(inputs=...)).  `stop_at`
    matches by data_ptr() -- a detached alias of a listed tensor is cut too -- and is read by conv2d's backward only: list the
    tensor a conv consumes (TrainStep lists the discriminator's input)."""
    prev = (_state.skip_ids, _state.stop_ids)
    _state.skip_ids = frozenset(id(p) for p in skip_params)
    _state.stop_ids = frozenset(t.data_ptr() for t in stop_at)
    try:
        yield
    finally:
        _state.skip_ids, _state.stop_ids = prev


@contextlib.contextmanager
def no_param_grads():
    """Inside this context conv backward computes only the data gradient.  Used for the first-order
    pass of the gradient penalty (autograd.grad w.r.t. the interpolates only, sradsgan.py:621): a
    custom Function cannot see which outputs the engine needs, so the caller says it."""
    prev = _skip_param_grads()
    _state.skip_param_grads = True
    try:
        yield
    finally:
        _state.skip_param_grads = prev


@contextlib.contextmanager
def direct_param_grads(side_stream=None, group=1):
    """Inside this context the fused backward kernels ACCUMULATE parameter gradients straight into the
    parameters' existing .grad buffers (the gradient arena of dp.ParamArena) and hand autograd None for
    them: one wgrad launch per conv instead of wgrad + one `grad += new` launch per parameter
    (~600 tiny launches per step).  Only valid when every such parameter already owns a dense .grad
    and nobody asks autograd for these gradients explicitly (TrainStep guarantees both)."""
    prev, _state.wgrads = _state.wgrads, _WgradQueue(side_stream, group)
    try:
        yield
        flush_pending_wgrads()
        if _state.wgrads.pending:                      # before the restore below wipes the evidence
            raise RuntimeError('direct_param_grads: %d grouped weight gradient(s) still waiting for a partner after the flush'
                               % len(_state.wgrads.pending))
    finally:
        _state.wgrads = prev


_HOLD = int(os.environ.get('SRHIP_HOLD', '1'))     # 1: passed-through gradients (default); 2: every side-stream operand; 0: off (test knob)


def _hold_for_side(side, *tensors):
    """SRHIP_HOLD=2 only: keeps EVERY operand gradient of a side-stream launch referenced until the backward ends (see
    _passed_through for why a reference matters).  The default holds only the gradients that are known to be aliased; holding
    all of them costs 1.5 % of the step (the allocator hands out cold blocks instead of the ones just freed:
    profiles/r04_step_ab_small_changes.txt) and protects against graph shapes the model does not have -- a gradient that one
    producer hands to several consumers (torch's AddBackward, ops._SumN) is shared until the last of them has run, and the
    trunk's bus gradient is held by the head convs' buffers until the end of the backward."""
    if _HOLD >= 2 and _state.wgrads is not None:
        _state.wgrads.held.extend(t for t in tensors if t is not None)


def _passed_through(g):
    """Call on an incoming gradient that a backward returns UNCHANGED as the gradient of one of its inputs while a weight-gradient
    kernel on the side stream reads it.  record_stream() protects the tensor's MEMORY; this protects its CONTENTS: autograd's
    input buffer adds later contributions IN PLACE into a gradient it holds the only reference to
    (torch/csrc/autograd/input_buffer.cpp, use_count() == 1), on the main stream, which the side stream may trail by a
    millisecond.  The attention tail hands `g` back as the gradient of `skip`, a conv with a fused residual hands it back as the
    residual's: when the ResGroup's first RAB delivered its data gradient 1 ms later the engine ran `g += dx` under the tail
    conv's weight-gradient kernel -- ResGroup tail conv gradients off by 10-30 % whenever the side stream lagged
    (tests/test_model_gpu.py: the first-step test after two pool streams, and the lagging-side-stream test).  With a second
    reference alive until the backward ends the engine allocates the sum instead, which is what it does for every gradient
    that is not aliased (12 + a few tensors of 24 MB per step)."""
    q = _state.wgrads
    if _HOLD and q is not None and q.side is not None and g is not None:
        q.held.append(g)
    return g


_CARRY = os.environ.get('SRHIP_CARRY', '1') == '1'          # A/B knob: 0 = autograd sums the gradients of a group input (two add passes per group)


def carry_open(x):
    """Called by a consumer structure (model.ResGroup) on a block input `x` whose FIRST consumer is a fused RAB (rab_block): the input's
    other consumers -- the group's skip connection (attention_tail) and the trunk's bus (sum_tensors) -- then do not hand their gradient
    to autograd (which would add the three contributions with two element-wise passes over the 24 MB tensor) but stash it, and the RAB's
    conv1 data gradient, computed last, takes them as extra residuals of its epilogue (srhip_conv2d_dgrad_res3 / _pp_res3).  The order of
    the backward makes this safe: the RAB's backward depends on the group tail's, and the whole trunk's on the bus's; it is CHECKED:
    the RAB counts the stashes it finds against the consumers that committed at forward time and raises when one is missing.
    The tag travels as an attribute of the tensor object (a fresh token per call: no stale matches)."""
    if not _CARRY or not x.is_cuda or not (torch.is_grad_enabled() and x.requires_grad):
        return
    if _state.carry is None or len(_state.carry_expect) > 4096:     # (forwards that never ran a backward leave their counters behind)
        _state.carry, _state.carry_expect = {}, {}
    _state.carry_token += 1
    x._srhip_carry = _state.carry_token
    _state.carry_expect[_state.carry_token] = 0


def _carry_commit(t):
    """forward time, a consumer that can stash: returns the token it will stash under (None: the tensor carries no tag)."""
    token = getattr(t, '_srhip_carry', None) if _CARRY else None
    if token is None or _state.carry_expect is None or token not in _state.carry_expect or not (torch.is_grad_enabled() and t.requires_grad):
        return None
    _state.carry_expect[token] += 1
    return token


def _carry_stash(token, g):
    """backward time: True = `g` is stashed for the RAB (return None to autograd), False = hand it to autograd as usual."""
    if token is None or token not in _state.carry_expect:
        return False
    if torch.is_grad_enabled():                                  # a differentiable backward: autograd must see the edge
        _state.carry_expect[token] -= 1
        return False
    _state.carry.setdefault(token, []).append(g)
    return True


def _carry_take(token):
    if token is None or _state.carry_expect is None:
        return ()
    extras = _state.carry.pop(token, [])
    expect = _state.carry_expect.pop(token, 0)
    if len(extras) != expect:
        raise RuntimeError('rab_block backward: %d of %d gradients of the block input have arrived -- a consumer that committed to '
                           'stash its gradient (ops.carry_open) has not run its backward yet' % (len(extras), expect))
    return tuple(extras)


def _grad_slot(p):
    """The buffer to accumulate into, or None when direct accumulation is off / impossible for p."""
    if _state.wgrads is None or p is None or not p.requires_grad or not p.is_leaf:     # (a spectral conv's effective weight is no leaf:
        return None                                                                    # its gradient goes to autograd, ops.spectral_weights projects it)
    g = p.grad
    if g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.device != p.device:
        return None
    return g


# --------------------------------------------------------------------------------------------- #
# plumbing
# --------------------------------------------------------------------------------------------- #


CONV_MATH_MODES = {'fp32': 0, 'bf16x3': 1, 'half': 2}


def set_conv_math(mode):
    """Arithmetic of the conv contraction (include/sradsgan_hip.h, srhip_set_conv_math): 'fp32' = fp32 MFMA, 'bf16x3' =
    split-bf16 (three bf16 MFMA products per fp32 product, fp32 accumulate), 'half' = ONE 16-bit product (fp16 for
    activations, bf16 wherever gradients are multiplied; BASELINE configs[4], outside the 1e-3 parity contract).  Stands
    where torch.backends.cudnn.allow_tf32 stands for the reference's nn.Conv2d.  Returns the previous mode."""
    if mode not in CONV_MATH_MODES:
        raise ValueError('conv math mode must be one of %s' % sorted(CONV_MATH_MODES))
    lib = _hip.lib()
    prev = lib.srhip_get_conv_math()
    _hip.check(lib.srhip_set_conv_math(CONV_MATH_MODES[mode]))
    return [k for k, v in CONV_MATH_MODES.items() if v == prev][0]


def get_conv_math():
    return [k for k, v in CONV_MATH_MODES.items() if v == _hip.lib().srhip_get_conv_math()][0]


@contextlib.contextmanager
def conv_math(mode):
    prev = set_conv_math(mode)
    try:
        yield
    finally:
        set_conv_math(prev)


def _require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError('%s: sradsgan_amd ops run on the MI355X HIP path only (got a %s tensor); '
                           'there is no CPU fallback' % (what, t.device))
    if t.dtype != torch.float32:
        raise TypeError('%s: fp32 tensors only, got %s' % (what, t.dtype))


def nhwc(t):
    """Dense NHWC memory for a logical NCHW tensor."""
    return t.contiguous(memory_format=CL)


def _dense16(t):
    """Dense memory (NHWC for a 4-d tensor) at a 16-byte aligned address, as the float4 reductions require: a copy when t is a
    non-contiguous view or a view whose storage offset breaks the alignment, t itself otherwise."""
    t = t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def empty_nhwc(n, c, h, w, like):
    return torch.empty((n, c, h, w), device=like.device, dtype=torch.float32, memory_format=CL)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    # the raw handle of torch's current stream: torch.cuda.current_stream() builds a Stream object per call (~9 us, 300
    # calls per step on each of the two launching threads)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


class _PackRegistry:
    """Persistent packed images of trainable conv weights.  Each (Parameter, mode) gets ONE buffer that is
    rewritten in place: by a single batched launch after every optimiser step (repack_all, called from
    bump_weight_epoch) instead of ~280 tiny pack launches scattered through the next iteration."""

    def __init__(self):
        self.entries = []        # [weakref(w), mode, packed, data_ptr, version, pack event or None, packing stream, streams that waited]
        self.table = None
        self.dirty = True


_registry = _PackRegistry()


class _Slots(dict):
    """mode -> registry entry, the `_srhip_packed` attribute of a Parameter.  An entry holds a weak reference, an event and a device
    buffer that belong to THIS Parameter object: a pickle (torch.save(module)) or a copy of the Parameter takes its __dict__ along,
    so the dict pickles and copies as an empty one -- the copy packs its own images on first use and registers them itself."""

    def __reduce__(self):
        return (_Slots, ())

    def __deepcopy__(self, memo):
        return _Slots()

    def __copy__(self):
        return _Slots()


def _wshape(w):
    """OIHW shape of a conv weight; a Linear weight [out, in] is the 1x1 conv [out, in, 1, 1] (same memory)."""
    return tuple(w.shape) if w.dim() == 4 else (w.shape[0], w.shape[1], 1, 1)


def _pack_now(w, mode, packed):
    cout, cin, kh, kw = _wshape(w)
    wd = w.detach().contiguous()
    _hip.check(_hip.lib().srhip_pack_weight(_p(wd), _p(packed), cout, cin, kh, kw, mode, _stream()), 'pack_weight')


def repack_all():
    reg = _registry
    if any(ent[0]() is None for ent in reg.entries):            # parameters of discarded models
        reg.entries = [ent for ent in reg.entries if ent[0]() is not None]
        reg.dirty = True
    if not reg.entries:
        return
    lib = _hip.lib()
    live = [ent[0]() for ent in reg.entries]
    if not reg.dirty:
        # a parameter re-homed since the table was built (dp.ParamArena adopting a net that has run, `p.data = ...`) and not used since:
        # the table would read the storage it has left
        reg.dirty = any(ent[3] != w.data_ptr() for ent, w in zip(reg.entries, live))
    if reg.dirty or reg.table is None:
        import struct
        assert lib.srhip_pack_entry_bytes() == 40
        blob = bytearray()
        for ent, w in zip(reg.entries, live):
            mode, packed = ent[1], ent[2]
            cout, cin, kh, kw = _wshape(w)
            fast = lib.srhip_packed_is_fast(cout, cin, kh, kw, mode)
            blob += struct.pack('<QQiiiiii', w.data_ptr(), packed.data_ptr(), cout, cin, kh, kw, mode, fast)
            ent[3] = w.data_ptr()
        reg.table = torch.frombuffer(blob, dtype=torch.uint8).to(live[0].device)
        reg.dirty = False
    _hip.check(lib.srhip_pack_weights_batched(_p(reg.table), len(reg.entries), _stream()), 'pack_weights_batched')
    for ent, w in zip(reg.entries, live):
        ent[4] = w._version
        ent[5] = None            # re-packed here, at the step boundary every other stream synchronises with (see _pack_fence)


def bump_weight_epoch():
    """Called by the fused optimiser (it updates parameters through raw pointers, which does not bump
    tensor._version): re-packs every registered conv weight in one launch."""
    repack_all()


def _pack_fence(ent):
    """A packed image is written by a kernel on the stream that first needed it (lazily, in the first step: the weight-
    gradient stream packs VGG's weights for the real batch, the D stream packs the discriminator's data-gradient images
    for the penalty's first-order backward) and read by every stream afterwards.  Nothing else orders those reads behind
    the pack kernel: in the first step of a model the main stream could run D(gen)'s data gradients on images the D stream
    had not packed yet -- zeros on fresh memory (a silently wrong first step), NaNs on recycled memory
    (tests/test_model_gpu.py::test_first_step_of_a_model_does_not_depend_on_allocator_history).  The entry carries the pack's event; a stream waits for it once."""
    ev = ent[5]
    if ev is None:
        return
    cs = torch.cuda.current_stream()
    sid = cs.cuda_stream
    if sid == ent[6] or sid in ent[7]:
        return
    if torch.cuda.is_current_stream_capturing():
        return                   # a capture starts long after the eager warm-up iteration that packed
    cs.wait_event(ev)
    ent[7].add(sid)


def _pack_event(ent):
    ev = torch.cuda.Event()
    ev.record()
    ent[5], ent[6], ent[7] = ev, torch.cuda.current_stream().cuda_stream, set()


_static_gen = 0                  # moves with every mark_static / mark_trainable: dp.ParamArena looks for static parameters again


def mark_static(module):
    """Parameters of `module` are never updated (VGG): pack once, keep out of the per-step batched repack."""
    global _static_gen
    for p in module.parameters():
        p._srhip_static = True
    _static_gen += 1


def mark_trainable(module):
    """The inverse of mark_static: the static mark goes, and packed images made so far (a frozen net that has run, or one that has
    trained before) are dropped and leave the batched re-pack, so that the next use packs the weights again and registers them."""
    global _static_gen
    _static_gen += 1
    dropped = set()
    for p in module.parameters():
        dropped.update(id(ent) for ent in getattr(p, '_srhip_packed', {}).values())
        for attr in ('_srhip_static', '_srhip_packed'):
            if hasattr(p, attr):
                delattr(p, attr)
    if any(id(ent) in dropped for ent in _registry.entries):
        _registry.entries = [ent for ent in _registry.entries if id(ent) not in dropped]
        _registry.dirty = True


def packed_weight(w, mode):
    """OIHW weight -> GEMM operand.  Parameters get a persistent buffer (see _PackRegistry); other tensors
    (e.g. the weight cotangent of a second-order pass) are packed on the fly."""
    cout, cin, kh, kw = _wshape(w)
    lib = _hip.lib()
    if not isinstance(w, torch.nn.Parameter):
        slots = getattr(w, '_srhip_eff_packed', None)
        if slots is not None:                      # an effective weight of ops.spectral_weights: one image per mode for the tensor's life
            return _eff_packed(w, slots, mode)
        packed = torch.empty(lib.srhip_packed_elems(cout, cin, kh, kw, mode), device=w.device, dtype=torch.float32)
        _pack_now(w, mode, packed)
        return packed
    slots = getattr(w, '_srhip_packed', None)
    if slots is None:
        slots = w._srhip_packed = _Slots()
    ent = slots.get(mode)
    if ent is None or ent[3] != w.data_ptr():
        packed = torch.empty(lib.srhip_packed_elems(cout, cin, kh, kw, mode), device=w.device, dtype=torch.float32)
        _pack_now(w, mode, packed)
        new = [weakref.ref(w), mode, packed, w.data_ptr(), w._version, None, 0, set()]
        if w.is_cuda and not torch.cuda.is_current_stream_capturing():
            _pack_event(new)
        if ent is not None:
            # by identity: `in` / `remove` compare entries with ==, which compares the weak references' live Parameters element-wise
            # and raises for every live entry in front of this one
            _registry.entries = [e for e in _registry.entries if e is not ent]
        slots[mode] = new
        if not getattr(w, '_srhip_static', False):
            _registry.entries.append(new)
            _registry.dirty = True
        return packed
    if ent[4] != w._version:                       # changed by a torch op (load_state_dict, torch optimiser, ...)
        _pack_fence(ent)                           # (write after the reads other streams may still have in flight is the caller's order)
        _pack_now(w, mode, ent[2])
        ent[4] = w._version
        if not torch.cuda.is_current_stream_capturing():
            _pack_event(ent)
    else:
        _pack_fence(ent)
    return ent[2]


def _parameters_of(things):
    seen, out = set(), []
    for t in things:
        for p in (t.parameters() if isinstance(t, torch.nn.Module) else (t,)):
            if not isinstance(p, torch.Tensor):
                raise TypeError('weights_changed: modules or parameters, got %s' % type(p).__name__)
            if id(p) not in seen:
                seen.add(id(p))
                out.append(p)
    return out


def invalidate_static(params):
    """Host only: the images of the static parameters among `params` are packed again at their next use.  For a writer that goes through
    raw pointers (dp.ParamArena.adam_step): static images are outside the batched re-pack that bump_weight_epoch runs."""
    for p in params:
        for ent in getattr(p, '_srhip_packed', {}).values():
            ent[4] = -1


def weights_changed(*modules_or_parameters):
    """Call after writing parameters in a way torch does not report: `p.data.normal_()`, `p.data.clamp_()`, `torch.nn.init.*_(p.data)`,
    `torch._foreach_*_([p.data])`, an EMA through `.data`, a raw-pointer kernel -- none of them moves `p._version` (INTEGRATION.md,
    "changing weights outside the trainer").  Brings every cached copy of the named parameters (all parameters of a module) up to date on
    the current stream: the packed images of both kinds, those of static nets included, and copies derived from a weight (the LPIPS stem).
    The images are rewritten in place, so a captured graph that reads them sees the new weights at its next replay.  Ordering: a stream
    that has already used an image waits for the new pack's event at its next use (_pack_fence); reads of the old image still in flight
    on another stream are the caller's to order, as for any write to the weights themselves."""
    capturing = torch.cuda.is_current_stream_capturing()
    for p in _parameters_of(modules_or_parameters):
        for got in getattr(p, '_srhip_derived', {}).values():
            _refresh_derived(p, got)
        eff = getattr(p, '_srhip_eff_packed', None)
        if eff:                                   # an effective weight of ops.spectral_weights that was edited: packed again at its next use
            eff.clear()
        slots = getattr(p, '_srhip_packed', None)
        if not slots:
            continue
        for mode, ent in list(slots.items()):
            if ent[3] != p.data_ptr():            # re-homed as well: packed_weight makes a new image and keeps the registry right
                packed_weight(p, mode)
                continue
            _pack_fence(ent)
            _pack_now(p, mode, ent[2])
            ent[4] = p._version
            if not capturing:
                _pack_event(ent)


def derived_weight(w, key, make):
    """A copy derived from parameter `w` (`make(w)`, e.g. the HWIO stem weight of lpips.LPIPS), kept on the parameter object and rebuilt
    when w's version or storage moves, or when weights_changed names w."""
    cache = getattr(w, '_srhip_derived', None)
    if cache is None:
        cache = w._srhip_derived = _Slots()
    got = cache.get(key)
    if got is None:
        got = cache[key] = [w._version, w.data_ptr(), make(w), make]
    elif got[0] != w._version or got[1] != w.data_ptr():
        _refresh_derived(w, got)
    return got[2]


def _refresh_derived(w, got):
    got[2].copy_(got[3](w))                       # in place: a captured graph reads this buffer
    got[0], got[1] = w._version, w.data_ptr()


eff_pack_stats = {'packed': 0, 'reused': 0}       # effective-weight images packed / found again (tests, tools/time_spectral.py)


def _eff_packed(w, slots, mode):
    """The packed image of an effective weight (a spectral conv's W = weight_bar / sigma of ONE pass: a fresh non-leaf tensor per pass,
    read by the pass's fprop, its first-order data gradient and the penalty's two second-order passes).  `slots` is a dict the tensor
    object carries (mode -> [image, pack event, packing stream, streams that waited]): packed on first use, alive exactly as long as
    the tensor, and -- like _pack_fence for parameters -- a stream other than the packing one waits for the pack's event once."""
    ent = slots.get(mode)
    cs = torch.cuda.current_stream()
    if ent is None:
        cout, cin, kh, kw = _wshape(w)
        packed = torch.empty(_hip.lib().srhip_packed_elems(cout, cin, kh, kw, mode), device=w.device, dtype=torch.float32)
        _pack_now(w, mode, packed)
        ev = None
        if not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event()
            ev.record()
        slots[mode] = [packed, ev, cs.cuda_stream, set()]
        eff_pack_stats['packed'] += 1
        return packed
    packed, ev, sid, waited = ent
    here = cs.cuda_stream
    if here != sid and here not in waited and ev is not None:
        cs.wait_event(ev)
        packed.record_stream(cs)
        waited.add(here)
    eff_pack_stats['reused'] += 1
    return packed


def _out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv2d_fwd_raw(x, w, bias, stride, pad, slope=None, residual=None, rowscale=None, chanscale=None, graddata=False, out_pp=None):
    """graddata: x holds gradients (a second-order pass): 'half' arithmetic then rounds to bf16 instead of fp16.
    out_pp: a PP buffer that ALSO receives y as padded planes (srhip_conv2d_fwd_dual; a conversion pass when the kernel that took the
    launch has no second destination)."""
    _require_gpu(x, 'conv2d_fwd')
    x = nhwc(x)
    n, cin, h, wd = x.shape
    cout, cin_w, kh, kw = _wshape(w)
    if cin_w != cin:
        raise ValueError('conv2d_fwd: weight expects %d input channels, got %d' % (cin_w, cin))
    ho, wo = _out_hw(h, wd, kh, stride, pad)
    y = empty_nhwc(n, cout, ho, wo, x)
    flags = 0
    if bias is not None:
        flags |= EPI_BIAS
        bias = bias.detach().contiguous()
    if slope is not None:
        flags |= EPI_LRELU
    if residual is not None:
        residual = nhwc(residual)
        flags |= EPI_RESIDUAL
    if rowscale is not None:
        rowscale = rowscale.contiguous()
        flags |= EPI_ROWSCALE
    if chanscale is not None:
        chanscale = chanscale.contiguous()
        flags |= EPI_CHANSCALE
    if graddata:
        flags |= EPI_GRADDATA
    lib = _hip.lib()
    if out_pp is not None:
        served = ctypes.c_int(0)
        _hip.check(lib.srhip_conv2d_fwd_dual(_p(x), _p(packed_weight(w, 0)), _p(bias), _p(residual), _p(rowscale),
                                             _p(chanscale), _p(y), _p(out_pp.buf), ctypes.byref(served),
                                             n, h, wd, cin, cout, kh, kw, stride, pad, cin, cout, cout,
                                             float(slope or 0.0), flags, _stream()), 'conv2d_fwd_dual')
        if not served.value:
            pp_from_f32(y, out=out_pp)
        return y
    _hip.check(lib.srhip_conv2d_fwd(_p(x), _p(packed_weight(w, 0)), _p(bias), _p(residual), _p(rowscale),
                                    _p(chanscale), _p(y),
                                    n, h, wd, cin, cout, kh, kw, stride, pad, cin, cout, cout,
                                    float(slope or 0.0), flags, _stream()), 'conv2d_fwd')
    return y


def pool_epilogue_ok(x, w):
    """RAB conv2 + its CLAM pooling partials in one call (srhip_conv2d_fwd_pool): split-bf16, stride-1 3x3 to 64 channels."""
    return (x.is_cuda and get_conv_math() == 'bf16x3' and tuple(w.shape[2:]) == (3, 3) and w.shape[0] == 64
            and w.shape[1] % 32 == 0)


def conv2d_fwd_pool_raw(x, w, bias):
    """y = conv3x3(x, w) + bias (stride 1, pad 1, 64 output channels) and the CLAM pooling partials of y.
    Returns (y, (pool, section_bytes, nseg)): pool = [sum | max | arg] sections, nseg partial segments per image."""
    _require_gpu(x, 'conv2d_fwd_pool')
    x = nhwc(x)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    y = empty_nhwc(n, cout, h, wd, x)
    lib = _hip.lib()
    sec = n * lib.srhip_clam_pool_max_segments() * 64 * 4
    pool = torch.empty(3 * sec // 4, device=x.device, dtype=torch.float32)
    nseg = ctypes.c_int(0)
    b = bias.detach().contiguous() if bias is not None else None
    _hip.check(lib.srhip_conv2d_fwd_pool(_p(x), _p(packed_weight(w, 0)), _p(b), _p(y), _p(pool), sec, ctypes.byref(nseg), n, h, wd, cin,
                                         cout, cin, cout, EPI_BIAS if b is not None else 0, _stream()), 'conv2d_fwd_pool')
    return y, (pool, sec, nseg.value)


def conv2d_dgrad_raw(dy, w, x_shape, stride, pad, residual=None, actmask=None, slope=0.0, extra=()):
    """dx = conv_transpose(dy, w) [* lrelu'(actmask)] [+ residual] [+ extra[0] + extra[1]]: the optional tail fuses the backward
    of the LeakyReLU that produced this conv's input and the skip-path gradient add; `extra`: up to two more gradients of dx's
    shape (ops.carry_open), added after the residual in the order given."""
    _require_gpu(dy, 'conv2d_dgrad')
    dy = nhwc(dy)
    n, cin, h, wd = x_shape
    cout, _, kh, kw = _wshape(w)
    dx = empty_nhwc(n, cin, h, wd, dy)
    if residual is not None:
        residual = nhwc(residual)
    if actmask is not None:
        actmask = nhwc(actmask)
    lib = _hip.lib()
    if extra:
        if residual is None or actmask is not None or len(extra) > 2:
            raise ValueError('conv2d_dgrad: extra residuals ride beside a residual, without an activation mask, at most two')
        extra = [nhwc(e) for e in extra]
        _hip.check(lib.srhip_conv2d_dgrad_res3(_p(dy), _p(packed_weight(w, 1)), _p(dx), _p(residual), _p(extra[0]),
                                               _p(extra[1]) if len(extra) > 1 else None, n, h, wd, cin, cout, kh, kw, stride, pad,
                                               _stream()), 'conv2d_dgrad_res3')
        return dx
    _hip.check(lib.srhip_conv2d_dgrad(_p(dy), _p(packed_weight(w, 1)), _p(dx), _p(residual), _p(actmask), float(slope),
                                      n, h, wd, cin, cout, kh, kw, stride, pad, cout, cin, cin, 0, _stream()),
               'conv2d_dgrad')
    return dx


_HEAD_BITS = os.environ.get('SRHIP_HEAD_BITS', '1') == '1'    # A/B knob: 0 = the head conv's LeakyReLU backward runs as passes of its own over the gradient and y


def head_mask_ok(x_shape, w_shape, stride, pad):
    """The head conv (3 -> 64, 3x3, full image size) whose forward can leave its activation record behind (srhip_conv2d_head_mask_ok)."""
    n, cin, h, wd = x_shape
    cout, _, kh, kw = w_shape
    return bool(_hip.lib().srhip_conv2d_head_mask_ok(n, h, wd, cin, cout, kh, kw, stride, pad))


def conv2d_fwd_head_mask_raw(x, w, bias, slope, bits=None):
    """bits None: (y, record) with y = lrelu(conv(x, w) + bias) and the record of y > 0, one 64-bit word per pixel.
    bits given: y = mask * conv(x, w) (no bias), mask = 1 where the record's bit is set, else slope."""
    _require_gpu(x, 'conv2d_fwd_head_mask')
    x = nhwc(x)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    y = empty_nhwc(n, cout, h, wd, x)
    lib = _hip.lib()
    made = bits is None
    if made:
        bits = torch.empty(n * h * wd, device=x.device, dtype=torch.int64)
        bias = bias.detach().contiguous()
    _hip.check(lib.srhip_conv2d_fwd_head_mask(_p(x), _p(packed_weight(w, 0)), _p(bias) if made else None, _p(y), _p(bits) if made else None,
                                              None if made else _p(bits), bits.numel() * 8, n, h, wd, cin, cout, cin, cout, float(slope),
                                              (EPI_BIAS | EPI_LRELU) if made else 0, _stream()), 'conv2d_fwd_head_mask')
    return (y, bits) if made else y


def conv2d_dgrad_head_mask_raw(dy, w, x_shape, bits, slope):
    """dx = conv_transpose(mask * dy, w): the head conv's data gradient from the gradient at its ACTIVATED output."""
    _require_gpu(dy, 'conv2d_dgrad_head_mask')
    dy = nhwc(dy)
    n, cin, h, wd = x_shape
    cout = w.shape[0]
    dx = empty_nhwc(n, cin, h, wd, dy)
    _hip.check(_hip.lib().srhip_conv2d_dgrad_head_mask(_p(dy), _p(packed_weight(w, 1)), _p(dx), _p(bits), bits.numel() * 8, float(slope),
                                                       n, h, wd, cin, cout, cout, cin, _stream()), 'conv2d_dgrad_head_mask')
    return dx


_SIDE_WS = {}


def _wgrad_workspace(nbytes, device, stream=None):
    """(split-K workspace, raw stream handle) of a weight-gradient launch.  On the current stream (stream=None): a fresh buffer.
    On a side stream: ONE persistent buffer per stream -- the kernels of one stream run in order, so they can share it, and a
    buffer that is never freed needs no record_stream (a per-call buffer allocated on the launching stream and used on the
    side stream would)."""
    need = (max(int(nbytes), 4) + 3) // 4
    if stream is None:
        return torch.empty(need, device=device, dtype=torch.float32), _stream()
    key = (device.index, stream.cuda_stream)
    ws = _SIDE_WS.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            ws.record_stream(stream)                     # kernels already enqueued may still use the old buffer
        ws = _SIDE_WS[key] = torch.empty(max(need, 1 << 20), device=device, dtype=torch.float32)
    return ws, ctypes.c_void_p(stream.cuda_stream)


def _wgrad_tables(items):
    """ctypes pointer tables (x, dy, dw, db) of a grouped launch: items are tuples or _Wgrad records, operands first."""
    tab = ctypes.c_void_p * len(items)
    cols = zip(*[(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None) for x, dy, dw, db, *_ in items])
    return [tab(*col) for col in cols]


def conv2d_wgrad_raw(x, dy, w_shape, stride, pad, with_bias=False, xrowscale=None, xchanscale=None, out=None, on_stream=None, head_bits=None):
    """(dw [OIHW], db [Cout] or None): the bias gradient comes out of the same kernel pass.
    out=(dw_buf, db_buf or None): accumulate into these buffers instead (dw_buf += dw, db_buf += db).
    on_stream: launch on this torch stream (already ordered behind the operands' producers by the caller) instead of the
    current one, with that stream's persistent workspace.
    head_bits=(record, slope): dy is the gradient at the head conv's ACTIVATED output; the kernel multiplies it by the LeakyReLU mask
    of the record as it reads it (srhip_conv2d_wgrad_head_mask)."""
    _require_gpu(x, 'conv2d_wgrad')
    x, dy = nhwc(x), nhwc(dy)
    n, cin, h, wd = x.shape
    cout, _, kh, kw = w_shape
    lib = _hip.lib()
    ws, st = _wgrad_workspace(lib.srhip_conv2d_wgrad_workspace(n, h, wd, cin, cout, kh, kw, stride, pad), x.device, on_stream)
    if out is None:
        dw = torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
        db = torch.empty(cout, device=x.device, dtype=torch.float32) if with_bias else None
    else:
        dw, db = out
    if head_bits is not None:
        if out is not None or xrowscale is not None or xchanscale is not None or (kh, kw, stride, pad) != (3, 3, 1, 1):
            raise ValueError('conv2d_wgrad: the activation record goes with the plain 3x3 head conv, not accumulated')
        bits, slope = head_bits
        _hip.check(lib.srhip_conv2d_wgrad_head_mask(_p(x), _p(dy), _p(bits), bits.numel() * 8, float(slope), _p(dw), _p(db), _p(ws),
                                                    ws.numel() * 4, n, h, wd, cin, cout, cin, cout, st), 'conv2d_wgrad_head_mask')
        return dw, db
    _hip.check(lib.srhip_conv2d_wgrad(_p(x), _p(dy), _p(dw), _p(db), _p(xrowscale), _p(xchanscale), int(out is not None), _p(ws),
                                      ws.numel() * 4, n, h, wd, cin, cout, kh, kw, stride, pad, cin, cout, st), 'conv2d_wgrad')
    return dw, db


def _fork_side(side, handles=None):
    """The side stream waits for everything enqueued so far on the current stream (and on the streams whose raw handles are
    given: the producers of operands that were queued for a grouped launch)."""
    hs = {_stream().value}
    if handles:
        hs.update(handles)
    hs.discard(side.cuda_stream)
    for h in hs:
        if _state.capturing:
            side.wait_stream(torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream())
        else:
            _hip.check(_hip.lib().srhip_stream_fork(ctypes.c_void_p(h), ctypes.c_void_p(side.cuda_stream)), 'stream_fork')


def conv2d_wgrad_multi_raw(items, on_stream=None):
    """items: [(x, dy, dw_buf, db_buf or None, stride, pad)] -- 2..4 weight gradients of ONE shape, accumulated into their
    buffers by one grouped launch (srhip_conv2d_wgrad_multi) on `on_stream` (default: the current stream)."""
    x0, dy0, dw0, _, stride, pad, *_ = items[0]
    n, cin, h, wd = x0.shape
    cout, _, kh, kw = dw0.shape
    lib = _hip.lib()
    xs, dys, dws, dbs = _wgrad_tables(items)
    ws, st = _wgrad_workspace(lib.srhip_conv2d_wgrad_workspace(n, h, wd, cin, cout, kh, kw, stride, pad), x0.device, on_stream)
    _hip.check(lib.srhip_conv2d_wgrad_multi(len(items), xs, dys, dws, dbs, 1, _p(ws), ws.numel() * 4, n, h, wd, cin, cout, kh, kw,
                                           stride, pad, cin, cout, st), 'conv2d_wgrad_multi')


# ---- padded split-bf16 planes (include/sradsgan_hip.h, ABI 9) ---------------------------------------------------------- #
class PP:
    """Padded planes of an NHWC tensor [n, c, h, w]: `buf` = bf16 [srhip_pp_plane_pixels(n, h, w), 2 c] (per 8 channels: 8 hi | 8 lo
    halves), pad / guard / tail rows zero.  The kernels never write those rows, so a buffer is zeroed ONCE (pp_empty) and can then be reused for any
    tensor of the same geometry."""
    __slots__ = ('buf', 'n', 'c', 'h', 'w')

    def __init__(self, buf, n, c, h, w):
        self.buf, self.n, self.c, self.h, self.w = buf, n, c, h, w

    @property
    def shape(self):
        return (self.n, self.c, self.h, self.w)

    def data_ptr(self):
        return self.buf.data_ptr()

    def record_stream(self, s):
        self.buf.record_stream(s)


def pp_empty(n, c, h, w, device):
    px = _hip.lib().srhip_pp_plane_pixels(n, h, w)
    return PP(torch.zeros(px, 2 * c, device=device, dtype=torch.bfloat16), n, c, h, w)


def pp_from_f32(x, out=None):
    """fp32 [n, c, h, w] (NHWC memory) -> padded planes (a stand-alone pass: tests, the bench's operand set-up)."""
    _require_gpu(x, 'pp_from_f32')
    x = nhwc(x)
    n, c, h, w = x.shape
    pp = out if out is not None else pp_empty(n, c, h, w, x.device)
    _hip.check(_hip.lib().srhip_pp_from_f32(_p(x), _p(pp.buf), n, h, w, c, c, _stream()), 'pp_from_f32')
    return pp


def pp_to_f32(pp):
    out = torch.empty(pp.n, pp.h, pp.w, pp.c, device=pp.buf.device, dtype=torch.float32).permute(0, 3, 1, 2)
    _hip.check(_hip.lib().srhip_pp_to_f32(_p(pp.buf), _p(out), pp.n, pp.h, pp.w, pp.c, pp.c, _stream()), 'pp_to_f32')
    return out


def conv2d_pp_ok(n, cin, h, w, cout):
    """The persistent patch kernel takes this 3x3 stride-1 pad-1 conv with padded-plane operands (split-bf16 mode)."""
    return bool(_hip.lib().srhip_conv2d_pp_ok(n, h, w, cin, cout))


def pp_sign_words(n, h, w, channels, device):
    """An (uninitialised) sign-word buffer for the LeakyReLU mask of an [n, channels, h, w] plane tensor (srhip_conv2d_pp_sign_bytes:
    1 bit per element, in the persistent patch kernel's own order), or None when the shape is not served."""
    nb = _hip.lib().srhip_conv2d_pp_sign_bytes(n, h, w, channels)
    return torch.empty(nb // 8, device=device, dtype=torch.int64) if nb else None


def conv2d_fwd_pp_raw(x, w, bias, slope=None, out_pp=None, pool=False, signs=None):
    """3x3 stride-1 pad-1 forward with padded-plane operands: x a PP or fp32 NHWC; out_pp = PP buffer to fill (then the result is that
    PP) or None (fp32 result).  pool=True (fp32 result of 64 channels): also the CLAM pooling partials, as conv2d_fwd_pool_raw.
    signs (pp_sign_words; bias + LeakyReLU onto planes): the launch also leaves the activation's sign words there."""
    cout, cin = w.shape[0], w.shape[1]
    n, _, h, wd = x.shape
    xpp = isinstance(x, PP)
    if not xpp:
        _require_gpu(x, 'conv2d_fwd_pp')
        x = nhwc(x)
    dev = x.buf.device if xpp else x.device
    if signs is not None:
        _hip.check(_hip.lib().srhip_conv2d_fwd_pp_signs(ctypes.c_void_p(x.data_ptr()), int(xpp), _p(packed_weight(w, 0)), _p(bias.detach().contiguous()),
                                                        ctypes.c_void_p(out_pp.data_ptr()), _p(signs), signs.numel() * 8, n, h, wd, cin, cout,
                                                        float(slope), _stream()), 'conv2d_fwd_pp_signs')
        return out_pp
    y = out_pp if out_pp is not None else torch.empty(n, h, wd, cout, device=dev, dtype=torch.float32).permute(0, 3, 1, 2)
    flags = 0
    b = None
    if bias is not None:
        flags |= EPI_BIAS
        b = bias.detach().contiguous()
    if slope is not None:
        flags |= EPI_LRELU
    lib = _hip.lib()
    pl, sec, nseg = None, 0, ctypes.c_int(0)
    if pool:
        sec = n * lib.srhip_clam_pool_max_segments() * 64 * 4
        pl = torch.empty(3 * sec // 4, device=dev, dtype=torch.float32)
    _hip.check(lib.srhip_conv2d_fwd_pp(ctypes.c_void_p(x.data_ptr()), int(xpp), _p(packed_weight(w, 0)), _p(b), ctypes.c_void_p(y.data_ptr()),
                                      int(out_pp is not None), _p(pl), sec, ctypes.byref(nseg), n, h, wd, cin, cout, float(slope or 0.0), flags,
                                      _stream()), 'conv2d_fwd_pp')
    return (y, (pl, sec, nseg.value)) if pool else y


def conv2d_dgrad_pp_raw(dy, w, residual=None, actmask=None, slope=0.0, out_pp=None, extra=(), signs=None):
    """3x3 stride-1 pad-1 data gradient with padded-plane operands: dy a PP or fp32 NHWC; out_pp = PP buffer to fill, with
    actmask = the PP of the LeakyReLU output that fed the forward conv, or signs = the sign words its producer left
    (conv2d_fwd_pp_raw(signs=)); or fp32 result (+ residual)."""
    cout, cin = w.shape[0], w.shape[1]
    n, _, h, wd = dy.shape
    ypp = isinstance(dy, PP)
    if not ypp:
        _require_gpu(dy, 'conv2d_dgrad_pp')
        dy = nhwc(dy)
    dev = dy.buf.device if ypp else dy.device
    if signs is not None:
        _hip.check(_hip.lib().srhip_conv2d_dgrad_pp_signs(ctypes.c_void_p(dy.data_ptr()), int(ypp), _p(packed_weight(w, 1)), ctypes.c_void_p(out_pp.data_ptr()),
                                                          _p(signs), signs.numel() * 8, float(slope), n, h, wd, cin, cout, _stream()), 'conv2d_dgrad_pp_signs')
        return out_pp
    dx = out_pp if out_pp is not None else torch.empty(n, h, wd, cin, device=dev, dtype=torch.float32).permute(0, 3, 1, 2)
    if residual is not None:
        residual = nhwc(residual)
    if extra:                                             # (ops.carry_open) up to two more gradients, added after the residual in this order
        if residual is None or actmask is not None or out_pp is not None or len(extra) > 2:
            raise ValueError('conv2d_dgrad_pp: extra residuals ride beside a residual of an fp32 destination, at most two')
        extra = [nhwc(e) for e in extra]
        _hip.check(_hip.lib().srhip_conv2d_dgrad_pp_res3(ctypes.c_void_p(dy.data_ptr()), int(ypp), _p(packed_weight(w, 1)), _p(dx), _p(residual),
                                                         _p(extra[0]), _p(extra[1]) if len(extra) > 1 else None, n, h, wd, cin, cout,
                                                         _stream()), 'conv2d_dgrad_pp_res3')
        return dx
    _hip.check(_hip.lib().srhip_conv2d_dgrad_pp(ctypes.c_void_p(dy.data_ptr()), int(ypp), _p(packed_weight(w, 1)), ctypes.c_void_p(dx.data_ptr()),
                                                int(out_pp is not None), _p(residual), ctypes.c_void_p(actmask.data_ptr()) if actmask is not None else None,
                                                float(slope), n, h, wd, cin, cout, _stream()), 'conv2d_dgrad_pp')
    return dx


def conv2d_wgrad_pp_raw(items, accumulate=True, on_stream=None):
    """items: [(x, dy, dw_buf, db_buf or None)] -- 1..4 weight gradients of ONE 3x3 stride-1 pad-1 shape by one launch of the flat
    kernels (srhip_conv2d_wgrad_pp): x and / or dy are PP objects (padded planes), an operand that is not is fp32 NHWC."""
    x0, dy0, dw0, *_ = items[0]
    cout, cin = dw0.shape[0], dw0.shape[1]
    n, _, h, wd = x0.shape
    lib = _hip.lib()
    xpp, ypp = int(isinstance(x0, PP)), int(isinstance(dy0, PP))
    for x, dy, *_ in items[1:]:
        if int(isinstance(x, PP)) != xpp or int(isinstance(dy, PP)) != ypp:
            raise RuntimeError('conv2d_wgrad_pp: the convolutions of one launch must share their operand formats (planes / fp32)')
    mask = lib.srhip_conv2d_wgrad_pp_ok(n, h, wd, cin, cout)
    want = 4 if (xpp and ypp) else 1 if ypp else 2 if xpp else 0
    if not (mask & want):
        raise RuntimeError('conv2d_wgrad_pp: shape %s -> %d not served with these operand formats (served mask %d)' % (tuple(x0.shape), cout, mask))
    k = len(items)
    xs, dys, dws, dbs = _wgrad_tables(items)
    ws, st = _wgrad_workspace(lib.srhip_conv2d_wgrad_pp_workspace(k, xpp, ypp, n, h, wd, cin, cout), dw0.device, on_stream)
    _hip.check(lib.srhip_conv2d_wgrad_pp(k, xs, dys, xpp, ypp, dws, dbs, 1 if accumulate else 0, _p(ws), ws.numel() * 4, n, h, wd, cin, cout,
                                        cout if xpp else cin, st), 'conv2d_wgrad_pp')


class _PlanePool:
    """Padded-plane buffers by geometry.  The kernels never write a buffer's pad / guard rows, so a buffer is zeroed once, when it
    is created, and handed out again for any tensor of its geometry.  A released buffer carries events of the streams that may
    still be reading it; get() takes the OLDEST released buffer whose events have completed and, when none has, a NEW buffer rather
    than a wait -- a wait would put the main stream behind the weight-gradient stream's last launch (the overlap the step lives on)."""

    def __init__(self):
        self.free = {}              # key -> [(PP, [events])], oldest first
        self.created = 0

    def get(self, n, c, h, w, device):
        key = (n, c, h, w, device.index)
        q = self.free.get(key)
        capturing = _state.capturing or torch.cuda.is_current_stream_capturing()
        if capturing:
            # a stream capture: buffers the capture creates live in the graph's private pool and must not leave it, buffers from
            # outside must not be queried (event queries are illegal while capturing): keep the two populations apart.  Inside the
            # capture a released buffer is taken back at once and the TAKING stream waits for the streams that may still read it
            # (wait_stream = record + wait, the one cross-stream primitive the capture already uses everywhere: it becomes a graph
            # edge) -- without it the side stream's weight-gradient node and the main stream's next writer of the same buffer were
            # unordered in the captured graph.  The wait covers everything the releasing stream has enqueued so far, not
            # just the reader: the replayed graph loses some overlap there, eager launches (the default) are not affected.
            # (Events recorded at release time and waited for here would be tighter, but an event that is recorded inside a capture
            # and never waited for -- a buffer nobody takes again -- crashed hipStreamEndCapture on ROCm 7.0.)
            key = key + ('capture',)
            q = self.free.get(key)
        if q:
            for i, (pp, evs) in enumerate(q):
                if capturing:
                    del q[i]
                    cur = torch.cuda.current_stream()
                    for st in evs:                      # (under capture the entries are the releasing STREAMS)
                        if st != cur:
                            cur.wait_stream(st)
                    return pp
                if all(ev.query() for ev in evs):
                    del q[i]
                    return pp
        self.created += 1
        return pp_empty(n, c, h, w, device)

    def release_all(self):
        """Drops every free buffer (after the streams that may still read them have passed their release events): a NEW model is
        about to run -- another scale of the chain sweep, another network -- and the old geometries' buffers would otherwise stay for
        the life of the process (chain sweep in one process: 115 -> 147 GB, profiles/r05_bench_chain_bf16x3.json)."""
        for key, q in self.free.items():
            for pp, evs in q:
                for ev in evs:
                    ev.synchronize()                   # (an event, or -- entries released inside a capture -- the stream itself)
        self.free.clear()

    def begin_capture(self):
        """A new stream capture starts: buffers (and the events they carry) of an earlier capture belong to that graph."""
        for key in [k for k in self.free if k[-1] == 'capture']:
            del self.free[key]

    def put(self, pp, streams=()):
        capturing = _state.capturing or torch.cuda.is_current_stream_capturing()
        evs = list(streams) if capturing else [s.record_event() for s in streams]
        key = (pp.n, pp.c, pp.h, pp.w, pp.buf.device.index) + (('capture',) if capturing else ())
        self.free.setdefault(key, []).append((pp, evs))


plane_pool = _PlanePool()
_X_PP = os.environ.get('SRHIP_X_PP', '1') == '1'                # A/B knob: 0 = a RAB's input never arrives as planes (conversion pass for its weight gradient)
_PP_SIGNS = os.environ.get('SRHIP_PP_SIGNS', '1') == '1'      # A/B knob: 0 = conv2's data gradient reads its LeakyReLU mask from t's hi plane (48 MB) instead of sign words (3 MB)


def rab_planes_ok(x, w1, w2):
    """The RAB keeps its two 256-channel tensors as padded planes: split-bf16 arithmetic, 64 -> Cmid -> 64 with both 3x3 convs and
    both weight gradients served on planes."""
    if not (x.is_cuda and get_conv_math() == 'bf16x3'):
        return False
    n, c, h, w = x.shape
    cm = w1.shape[0]
    lib = _hip.lib()
    return (tuple(w1.shape[2:]) == (3, 3) and tuple(w2.shape[2:]) == (3, 3) and w2.shape[0] == c and w2.shape[1] == cm
            and bool(lib.srhip_conv2d_pp_ok(n, h, w, c, cm)) and bool(lib.srhip_conv2d_pp_ok(n, h, w, cm, c))
            and (lib.srhip_conv2d_wgrad_pp_ok(n, h, w, c, cm) & 4) and (lib.srhip_conv2d_wgrad_pp_ok(n, h, w, cm, c) & 4))


def _to_planes(t, device):
    """fp32 NHWC operand of a weight gradient -> a pooled padded-plane copy (launched on the current stream)."""
    n, c, h, w = t.shape
    pp = plane_pool.get(n, c, h, w, device)
    return pp_from_f32(t, out=pp)


_WGRAD_MAX_AGE = 14    # weight-gradient calls a launch may wait for a partner
# RAB weight gradients of one shape per flat-kernel launch.  Round 6: 3 -- a ResGroup's three RABs -- instead of pairs: the launch keeps one
# block per CU, so every convolution gets a third instead of half of the split-K splits (28 instead of 42): a third fewer partial tiles written and
# reduced, and the launches line up with the group boundaries the exchange's parts are cut at.  +0.5 % same-box (profiles/r06_step_ab.txt; 4: the same)
_PP_GROUP = 3


class _Wgrad(NamedTuple):
    """One requested weight gradient: gw += wgrad(x, dy), gb += colsum(dy)."""
    x: object                       # operands: fp32 NHWC tensors, on the plane path also PP
    dy: object
    gw: torch.Tensor                # the parameters' gradient slots (gb: None = no bias gradient)
    gb: object
    stride: int
    pad: int
    release: tuple                  # pooled PP buffers that go back to the pool once the launch is enqueued
    producer: object                # raw handle of the stream the request came from: the one that produced the operands
    seq: int                        # the queue's request number at the request (the age of a pending launch, _WgradQueue.tick)


class _WgradQueue:
    """The weight gradients of one direct_param_grads() context: WHEN each is launched, BEHIND WHICH streams, and WHAT is kept alive until
    it has run.  Nothing reads a weight gradient before the optimiser, so they run on a side stream (`side`; None: the current stream,
    at once) beside the data gradients: the partially filled last wave of each data-gradient kernel and of each weight-gradient kernel
    overlap, and same-parameter accumulations stay ordered (one side stream).  Requests of one shape wait in `pending` for partners
    (`group` > 1) and go out in one launch."""

    def __init__(self, side, group):
        self.side = side
        self.capturing = _state.capturing               # (a stream capture wraps the whole context: TrainStep._capture)
        self.group = group if side is not None else 1   # weight gradients of one shape launched together (srhip_conv2d_wgrad_multi); 1 = off
        self.pending = {}                               # shape key -> [_Wgrad] waiting for partners
        self.held = []                                  # gradients kept referenced until the backward ends, see _passed_through
        self.seq = 0                                    # weight-gradient requests so far

    def job(self, x, dy, gw, gb, stride=1, pad=1, release=()):
        return _Wgrad(x, dy, gw, gb, stride, pad, release, _stream().value, self.seq)

    def run(self, jobs, launch, extra=(), by_handle=False):
        """The ONE place that runs something on the side stream: orders it behind the current stream and the jobs' producers, calls
        launch(on) -- on = the side stream when the launch takes it by raw handle (by_handle: no stream context, ~150 launches per step;
        not inside a capture, where the workspace must come from the capture's pool), else None = torch's current stream, which is
        then the side stream --, marks the fp32 operands (the jobs' x / dy and `extra`) as in use on it and holds the jobs' gradients
        (_hold_for_side).  Without a side stream: launch(None), at once."""
        side = self.side
        if side is None:
            launch(None)
            return
        _fork_side(side, [j.producer for j in jobs])
        if by_handle and not self.capturing:
            launch(side)
        else:
            with torch.cuda.stream(side):
                launch(None)
        for t in [t for j in jobs for t in (j.x, j.dy)] + list(extra):
            if t is not None and not isinstance(t, PP):
                t.record_stream(side)
        _hold_for_side(side, *[j.dy for j in jobs if not isinstance(j.dy, PP)])

    def run_fp32(self, jobs):
        """One launch for fp32 jobs of one shape (at most the step's group size: a pending list goes out the moment it is that long)."""
        def launch(on):
            if len(jobs) == 1:
                j, = jobs
                conv2d_wgrad_raw(j.x, j.dy, tuple(j.gw.shape), j.stride, j.pad, j.gb is not None, out=(j.gw, j.gb), on_stream=on)
            else:
                conv2d_wgrad_multi_raw(jobs, on_stream=on)
        self.run(jobs, launch, by_handle=True)

    def run_planes(self, jobs):
        """One launch of the flat kernel for plane jobs of one shape: fp32 operands are converted to planes (a pp_from_f32 pass of the
        64-channel operand: in-step +0.4 % over the kernel's own in-place split, profiles/r05_wgrad_flat.txt) and the flat kernel runs, all
        on the side stream (None: the current stream); pooled buffers go back to the pool with an event of that stream."""
        main = torch.cuda.current_stream()
        side = self.side
        run_on = side if side is not None else main

        def launch(_):
            conv, items = [], []
            for j in jobs:
                xo, dyo = j.x, j.dy
                if not isinstance(xo, PP):
                    xo = _to_planes(xo, j.gw.device)
                    conv.append(xo)
                if not isinstance(dyo, PP):
                    dyo = _to_planes(dyo, j.gw.device)
                    conv.append(dyo)
                items.append((xo, dyo, j.gw, j.gb))
            conv2d_wgrad_pp_raw(items, accumulate=True, on_stream=side)
            for pp in conv:
                plane_pool.put(pp, (run_on,))
            for j in jobs:
                for pp in j.release:
                    plane_pool.put(pp, (run_on,) if side is None else (run_on, main))
        self.run(jobs, launch)

    def tick(self):
        """Called at every weight-gradient request: a pending launch whose partner has not shown up within _WGRAD_MAX_AGE further requests
        goes out alone.  The RAB pairs meet within 4-5 requests; shapes that occur ONCE per backward (the up-sampler's conv at 54^2 and at
        108^2) used to wait for the flush at the END of the generator's backward and then ran, alone on the chip, for 0.5 ms after the
        main stream had finished (`tools/step_tail.py`, profiles/r05_step_tail_before.txt)."""
        self.seq += 1
        for key in [k for k, q in self.pending.items() if q and self.seq - q[0].seq > _WGRAD_MAX_AGE]:
            self.flush(key)

    def add(self, key, job, group):
        """`job` waits under `key` for partners of its shape; the `group`-th completes the launch.  A slot never appears twice in one
        launch (the problems of a grouped launch read, add and write their destinations unordered): a request for a slot that the
        waiting list already holds -- a weight used twice in one graph, the same conv in two successive backward calls of one context --
        sends that list out first, so the two contributions follow each other on the side stream."""
        q = self.pending.get(key)
        if q:
            taken = {t.data_ptr() for j in q for t in (j.gw, j.gb) if t is not None}
            if job.gw.data_ptr() in taken or (job.gb is not None and job.gb.data_ptr() in taken):
                self.flush(key)
        q = self.pending.setdefault(key, [])
        q.append(job)
        if len(q) >= group:
            self.flush(key)

    def flush(self, key):
        jobs = self.pending.pop(key, None)
        if jobs:
            (self.run_planes if key[0] == 'pp' else self.run_fp32)(jobs)

    def flush_all(self):
        for key in list(self.pending):
            self.flush(key)


def flush_pending_pp():
    """The RAB weight gradients of the flat kernel that are still waiting for partners go out now (end of a ResGroup's backward)."""
    q = _state.wgrads
    if q is not None:
        for key in [k for k in q.pending if k[0] == 'pp']:
            q.flush(key)


def flush_pending_wgrads():
    """Launches every weight gradient that is still waiting for a partner of its shape.  Called wherever something is about to
    order itself behind "all weight gradients so far": the exchange, the joins of the step, the end of direct_param_grads()."""
    if _state.wgrads is not None:
        _state.wgrads.flush_all()


def wgrad_pp_for_params(w, b, x, dy, want_b, release=()):
    """Weight (+ bias) gradient of a 3x3 stride-1 pad-1 conv whose 256-channel operand is a PP (the other fp32 NHWC), accumulated into
    the parameters' gradient slots by the flat kernel -- in groups on the weight-gradient stream like wgrad_for_params.  `release`:
    pooled PP buffers that go back to the pool once the launch is enqueued.  Returns False when direct accumulation is not possible
    (the caller converts and takes the fp32 path)."""
    gw = _grad_slot(w)
    gb = _grad_slot(b) if (want_b and b is not None) else None
    if gw is None or (want_b and b is not None and gb is None):
        return False
    q = _state.wgrads
    q.tick()
    job = q.job(x, dy, gw, gb, release=tuple(release))
    if q.group > 1:
        q.add(('pp', tuple(x.shape), w.shape[0], gb is not None, isinstance(x, PP), isinstance(dy, PP)), job, _PP_GROUP)   # one launch = one operand format
    else:
        q.run_planes([job])
    return True


def wgrad_for_params(w, b, x, dy, stride, pad, want_b, xrowscale=None, xchanscale=None, head_bits=None):
    """(dw, db) to return to autograd for parameters (w, b).  In direct_param_grads() mode the kernel
    accumulates into w.grad / b.grad, on the weight-gradient stream (_WgradQueue), and this returns (None, None).
    head_bits=(record, slope): dy is the gradient at the head conv's activated output (conv2d_wgrad_raw)."""
    cout, cin, kh, kw = w.shape
    gw = _grad_slot(w)
    gb = _grad_slot(b) if (want_b and b is not None) else None
    if gw is None or (want_b and gb is None):
        return conv2d_wgrad_raw(x, dy, tuple(w.shape), stride, pad, want_b, xrowscale, xchanscale, head_bits=head_bits)
    q = _state.wgrads
    x, dy = nhwc(x), nhwc(dy)
    lib = _hip.lib()
    if head_bits is None and lib.srhip_conv2d_wgrad_can_accumulate(cin, cout, kh, kw):
        q.tick()
        job = q.job(x, dy, gw, gb, stride, pad)
        if (q.group > 1 and xrowscale is None and xchanscale is None
                and lib.srhip_conv2d_wgrad_multi_ok(x.shape[0], x.shape[2], x.shape[3], cin, cout, kh, kw, stride, pad) >= q.group):
            # nothing reads a weight gradient before the optimiser: wait for a partner of the same shape (the next RAB's) and
            # launch them together -- one full wave of blocks serves both with half the split-K partials each
            q.add((tuple(x.shape), cout, stride, pad, gb is not None), job, q.group)
        else:
            # one C call forks the side stream behind the current one (event ring inside the library) and the kernel is
            # launched on it by handle: no torch Event, no stream context, no per-call workspace (~150 launches per step)
            q.run([job], lambda on: conv2d_wgrad_raw(x, dy, tuple(w.shape), stride, pad, want_b, xrowscale, xchanscale, out=(gw, gb), on_stream=on),
                  extra=(xrowscale, xchanscale), by_handle=True)
        return None, None

    # Shapes the accumulating kernel does not take (the 3- and 2-channel convs, the 64 -> 3 tail conv): add in program order
    # here rather than through autograd's AccumulateGrad, whose order among several contributions to one parameter
    # follows per-thread node counters (tests/test_graph_gpu.py) -- and, like the other weight gradients, on the side
    # stream: the 3 -> 64 head convs' gradients (0.2 - 0.3 ms each at 216 x 216) sat in the discriminator's serial chain
    def launch(_):
        dw, db = conv2d_wgrad_raw(x, dy, tuple(w.shape), stride, pad, want_b, xrowscale, xchanscale, head_bits=head_bits)
        gw.add_(dw)
        if db is not None:
            gb.add_(db)
    q.run([q.job(x, dy, gw, gb, stride, pad)], launch, extra=(xrowscale, xchanscale, head_bits[0] if head_bits is not None else None))
    return None, None


def _wgrad_act_direct(w, b, x, dy, y, slope, stride, pad):
    """Weight + bias gradient of a fused conv + LeakyReLU from the gradient at the activated output, accumulated into the
    parameters' arena slots on the weight-gradient stream (srhip_conv2d_wgrad_act).  False when the shape is not served."""
    cout, cin, kh, kw = w.shape
    gw, gb = _grad_slot(w), _grad_slot(b)
    if gw is None or gb is None:
        return False
    n, _, h, wd = x.shape
    lib = _hip.lib()
    if not lib.srhip_conv2d_wgrad_act_ok(n, h, wd, cin, cout, kh, kw, stride, pad):
        return False
    x, dy, y = nhwc(x), nhwc(dy), nhwc(y)

    def launch(_):
        ws, st = _wgrad_workspace(lib.srhip_conv2d_wgrad_workspace(n, h, wd, cin, cout, kh, kw, stride, pad), x.device)
        dw = torch.empty(tuple(w.shape), device=x.device, dtype=torch.float32)
        db = torch.empty(cout, device=x.device, dtype=torch.float32)
        _hip.check(lib.srhip_conv2d_wgrad_act(_p(x), _p(dy), _p(y), float(slope), _p(dw), _p(db), _p(ws), ws.numel() * 4,
                                              n, h, wd, cin, cout, kh, kw, stride, pad, cin, cout, st), 'conv2d_wgrad_act')
        gw.add_(dw)
        gb.add_(db)
    q = _state.wgrads
    q.run([q.job(x, dy, gw, gb, stride, pad)], launch, extra=(y,))
    return True


def colsum_raw(dy):
    """[N,C,H,W] (NHWC memory) -> [C] sum over N,H,W."""
    _require_gpu(dy, 'colsum')
    dy = nhwc(dy)
    n, c, h, w = dy.shape
    rows = n * h * w
    lib = _hip.lib()
    nbytes = lib.srhip_colsum_workspace(rows, c)
    ws = torch.empty((nbytes + 3) // 4, device=dy.device, dtype=torch.float32)
    out = torch.empty(c, device=dy.device, dtype=torch.float32)
    _hip.check(lib.srhip_colsum(_p(dy), _p(out), _p(ws), ws.numel() * 4, rows, c, c, _stream()), 'colsum')
    return out


def lrelu_bwd_raw(dy, y, slope):
    _require_gpu(dy, 'lrelu_bwd')
    dy, y = nhwc(dy), nhwc(y)
    dx = torch.empty_like(dy, memory_format=CL)
    _hip.check(_hip.lib().srhip_lrelu_bwd(_p(dy), _p(y), _p(dx), dy.numel(), float(slope), _stream()), 'lrelu_bwd')
    return dx


# --------------------------------------------------------------------------------------------- #
# differentiable (twice) convolution family: fwd <-> dgrad <-> wgrad are closed under autograd
# --------------------------------------------------------------------------------------------- #


_LRELU_BITS = os.environ.get('SRHIP_LRELU_BITS', '1') == '1'    # A/B knob: 0 = every application of a LeakyReLU backward reads y


def lrelu_bwd_bits_raw(dy, y, mask, slope):
    """dx = dy * LeakyReLU'(y) through srhip_lrelu_bwd_bits: y given -> reads y and WRITES its sign bits into `mask`; y None -> reads
    `mask` instead of y."""
    _require_gpu(dy, 'lrelu_bwd_bits')
    dy = nhwc(dy)
    dx = torch.empty_like(dy, memory_format=CL)
    _hip.check(_hip.lib().srhip_lrelu_bwd_bits(_p(dy), _p(nhwc(y)) if y is not None else None, _p(mask), _p(dx), dy.numel(), float(slope),
                                               _stream()), 'lrelu_bwd_bits')
    return dx


class _LReluBwd(Function):
    """g = dy * (y > 0 ? 1 : slope); linear in dy, the mask is a constant.  Applied under a recorded graph (create_graph: the gradient
    penalty's first-order pass) to a large activation it also leaves the SIGN BITS of y behind (1 / 32 of y's bytes), and its own
    backward -- the same mask on another tensor -- reads those instead of y (`mask` travels as a non-differentiable tensor argument)."""

    @staticmethod
    def forward(ctx, dy, y, slope, mask=None):
        ctx.slope = slope
        if mask is not None:                           # the double backward of an earlier application: y's sign bits instead of y
            ctx.save_for_backward(y, mask)
            return lrelu_bwd_bits_raw(dy, None, mask, slope)
        if (_LRELU_BITS and ctx.needs_input_grad[0] and dy.is_cuda and dy.numel() % 4 == 0
                and dy.numel() >= (1 << 22)):          # a graph is being recorded over this application: its backward will want the mask again
            nbytes = _hip.lib().srhip_lrelu_mask_bytes(dy.numel())
            mask = torch.empty((nbytes + 7) // 8, device=dy.device, dtype=torch.int64)
            ctx.save_for_backward(y, mask)
            return lrelu_bwd_bits_raw(dy, y, mask, slope)
        ctx.save_for_backward(y, None)
        return lrelu_bwd_raw(dy, y, slope)

    @staticmethod
    def backward(ctx, gg):
        y, mask = ctx.saved_tensors
        return _LReluBwd.apply(gg, y, ctx.slope, mask), None, None, None


class _ColSum(Function):
    @staticmethod
    def forward(ctx, dy):
        ctx.shape = dy.shape
        return colsum_raw(dy)

    @staticmethod
    def backward(ctx, g):
        return g.view(1, -1, 1, 1).expand(ctx.shape)


class _ConvFwd(Function):
    """y = act(conv(x, w) + b) [+ residual]   (act and residual are never combined by the model)."""

    @staticmethod
    def forward(ctx, x, w, b, residual, stride, pad, slope, graddata=False):
        if slope is not None and residual is not None:
            raise ValueError('conv2d: fused activation and residual are mutually exclusive')
        bits = None
        if (_HEAD_BITS and slope is not None and b is not None and not graddata and x.is_cuda and any(ctx.needs_input_grad[:3])
                and head_mask_ok(x.shape, w.shape, stride, pad)):
            # D's head conv with a backward to come: the forward leaves the activation record behind (1 bit per element of y), and the
            # kernels that consume the gradient at y apply the LeakyReLU mask from it -- no lrelu-backward pass, no re-read of y
            y, bits = conv2d_fwd_head_mask_raw(x, w, b, slope)
        else:
            y = conv2d_fwd_raw(x, w, b, stride, pad, slope, residual, graddata=graddata)
        ctx.stride, ctx.pad, ctx.slope = stride, pad, slope
        ctx.has_bias, ctx.has_res = b is not None, residual is not None
        ctx.save_for_backward(x, w, y if slope is not None else None, b, bits)
        return y

    @staticmethod
    def _backward_head_bits(ctx, dy, x, w, y, b, bits, need_dx, skip):
        """The backward of the head conv from its activation record; None where the record has no kernel for what is wanted (the caller
        then runs the passes over y)."""
        want_w = ctx.needs_input_grad[1] and not skip
        want_b = ctx.needs_input_grad[2] and not skip
        if want_b and not want_w:
            return None
        if torch.is_grad_enabled():                    # create_graph: the gradient penalty's first-order pass
            if want_w or not need_dx:
                return None
            return _HeadDgradMasked.apply(dy, w, y.detach(), bits, tuple(x.shape), ctx.slope), None, None, None, None, None, None, None
        dx = conv2d_dgrad_head_mask_raw(dy, w, tuple(x.shape), bits, ctx.slope) if need_dx else None
        dw = db = None
        if want_w and _state.wgrads is not None:
            dw, db = wgrad_for_params(w, b, x, dy, ctx.stride, ctx.pad, want_b, head_bits=(bits, ctx.slope))
        elif want_w:
            dw, db = conv2d_wgrad_raw(x, dy, tuple(w.shape), ctx.stride, ctx.pad, want_b, head_bits=(bits, ctx.slope))
        return dx, dw, db, None, None, None, None, None

    @staticmethod
    def backward(ctx, dy):
        x, w, y, b, bits = ctx.saved_tensors
        skip = _skip_param_grads(w)
        need_dx = ctx.needs_input_grad[0] and x.data_ptr() not in _state.stop_ids
        if bits is not None:
            out = _ConvFwd._backward_head_bits(ctx, dy, x, w, y, b, bits, need_dx, skip)
            if out is not None:
                return out
        if ctx.slope is not None and not need_dx and not skip and ctx.needs_input_grad[1] and ctx.has_bias and \
                ctx.needs_input_grad[2] and _state.wgrads is not None and not torch.is_grad_enabled() and \
                _wgrad_act_direct(w, b, x, dy, y, ctx.slope, ctx.stride, ctx.pad):
            # head conv of the discriminator in the D step: only its parameter gradients are wanted, and the kernel applies the
            # activation's backward while it reads dy -- no lrelu-backward pass over the 382 MB gradient in the serial chain
            return None, None, None, None, None, None, None, None
        g = dy if ctx.slope is None else _LReluBwd.apply(dy, y, ctx.slope)
        dx = _ConvDgrad.apply(g, w, tuple(x.shape), ctx.stride, ctx.pad) if need_dx else None
        dw = db = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2] and not skip
        if ctx.needs_input_grad[1] and not skip and _state.wgrads is not None and not torch.is_grad_enabled():
            dw, db = wgrad_for_params(w, b, x, g, ctx.stride, ctx.pad, want_b)
        elif ctx.needs_input_grad[1] and not skip:
            dw, db = _ConvWgrad.apply(x, g, tuple(w.shape), ctx.stride, ctx.pad, want_b)
        elif want_b:
            db = _ColSum.apply(g)
        dres = _passed_through(dy) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        return dx, dw, db, dres, None, None, None, None


class _ConvDgrad(Function):
    """dx = conv_transpose(dy, w): bilinear in (dy, w)."""

    @staticmethod
    def forward(ctx, dy, w, x_shape, stride, pad):
        ctx.stride, ctx.pad, ctx.x_shape = stride, pad, x_shape
        ctx.save_for_backward(dy, w)
        return conv2d_dgrad_raw(dy, w, x_shape, stride, pad)

    @staticmethod
    def backward(ctx, ddx):
        dy, w = ctx.saved_tensors
        skip = _skip_param_grads(w)
        d_dy = _ConvFwd.apply(ddx, w, None, None, ctx.stride, ctx.pad, None, True) if ctx.needs_input_grad[0] else None
        d_w = None
        if ctx.needs_input_grad[1] and not skip and _state.wgrads is not None and not torch.is_grad_enabled():
            d_w, _ = wgrad_for_params(w, None, ddx, dy, ctx.stride, ctx.pad, False)   # same stream/order as every other wgrad of w
        elif ctx.needs_input_grad[1] and not skip:
            d_w, _ = _ConvWgrad.apply(ddx, dy, tuple(w.shape), ctx.stride, ctx.pad, False)
        return d_dy, d_w, None, None, None


class _HeadDgradMasked(Function):
    """dx = conv_transpose(m * dy, w) with m = LeakyReLU'(y) read from the head conv's activation record: bilinear in (dy, w), the mask
    is a constant.  One node where _LReluBwd and _ConvDgrad stood, and neither m * dy nor the second-order m * conv(ddx, w) is ever
    a tensor of its own: the kernels on both sides apply the mask in registers.  `y` rides along for a third-order graph only."""

    @staticmethod
    def forward(ctx, dy, w, y, bits, x_shape, slope):
        ctx.x_shape, ctx.slope = x_shape, slope
        ctx.save_for_backward(dy, w, y, bits)
        return conv2d_dgrad_head_mask_raw(dy, w, x_shape, bits, slope)

    @staticmethod
    def backward(ctx, ddx):
        dy, w, y, bits = ctx.saved_tensors
        skip = _skip_param_grads(w)
        d_dy = _HeadFwdMasked.apply(ddx, w, y, bits, ctx.slope) if ctx.needs_input_grad[0] else None
        d_w = None
        if ctx.needs_input_grad[1] and not skip and torch.is_grad_enabled():
            d_w, _ = _ConvWgrad.apply(ddx, _LReluBwd.apply(dy, y, ctx.slope), tuple(w.shape), 1, 1, False)
        elif ctx.needs_input_grad[1] and not skip and _state.wgrads is not None:
            d_w, _ = wgrad_for_params(w, None, ddx, dy, 1, 1, False, head_bits=(bits, ctx.slope))   # same stream/order as every other wgrad of w
        elif ctx.needs_input_grad[1] and not skip:
            d_w, _ = conv2d_wgrad_raw(ddx, dy, tuple(w.shape), 1, 1, False, head_bits=(bits, ctx.slope))
        return d_dy, d_w, None, None, None, None


class _HeadFwdMasked(Function):
    """d_dy = m * conv(ddx, w): the adjoint of _HeadDgradMasked in dy, the mask applied in the head conv kernel's epilogue."""

    @staticmethod
    def forward(ctx, ddx, w, y, bits, slope):
        ctx.slope = slope
        ctx.save_for_backward(ddx, w, y, bits)
        return conv2d_fwd_head_mask_raw(ddx, w, None, slope, bits=bits)

    @staticmethod
    def backward(ctx, g):
        ddx, w, y, bits = ctx.saved_tensors
        d_ddx = _HeadDgradMasked.apply(g, w, y, bits, tuple(ddx.shape), ctx.slope) if ctx.needs_input_grad[0] else None
        d_w = None
        if ctx.needs_input_grad[1] and not _skip_param_grads(w):
            d_w, _ = _ConvWgrad.apply(ddx, _LReluBwd.apply(g, y, ctx.slope), tuple(w.shape), 1, 1, False)
        return d_ddx, d_w, None, None, None


class _ConvWgrad(Function):
    """(dw, db) = wgrad(x, dy): dw bilinear in (x, dy), db = sum of dy over pixels."""

    @staticmethod
    def forward(ctx, x, dy, w_shape, stride, pad, with_bias):
        ctx.stride, ctx.pad, ctx.w_shape = stride, pad, w_shape
        ctx.save_for_backward(x, dy)
        dw, db = conv2d_wgrad_raw(x, dy, w_shape, stride, pad, with_bias)
        if db is None:
            ctx.mark_non_differentiable()
        return dw, db

    @staticmethod
    def backward(ctx, ddw, ddb):
        x, dy = ctx.saved_tensors
        d_x = d_dy = None
        if ddw is not None:
            ddw = ddw.contiguous()
            if ctx.needs_input_grad[0]:
                d_x = _ConvDgrad.apply(dy, ddw, tuple(x.shape), ctx.stride, ctx.pad)
            if ctx.needs_input_grad[1]:
                d_dy = _ConvFwd.apply(x, ddw, None, None, ctx.stride, ctx.pad, None, True)
        if ddb is not None and ctx.needs_input_grad[1]:
            e = ddb.view(1, -1, 1, 1).expand(dy.shape)
            d_dy = e if d_dy is None else d_dy + e
        return d_x, d_dy, None, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, act_slope=None, residual=None):
    """nn.Conv2d forward with the elementwise tail of its call site fused (bias, LeakyReLU/ReLU,
    residual add).  x: logical NCHW; returns logical NCHW in NHWC memory."""
    return _ConvFwd.apply(x, weight, bias, residual, stride, padding, act_slope)


# --------------------------------------------------------------------------------------------- #
# spectral normalisation of conv weights (csrc/sn.hip; reference base_networks.py:73-131)
# --------------------------------------------------------------------------------------------- #


def _align64(n):
    return (n + 63) // 64 * 64


class SpectralTable:
    """The spectral layers of one network, [(weight_bar, weight_u, weight_v)], as the device table srhip_sn_forward_batched /
    srhip_sn_backward_batched walk.  The table holds the parameters' addresses and, for what a pass writes, offsets into a buffer that
    is allocated per pass: it is built once (again only when a parameter has moved: .to(), dp.ParamArena) and no pass copies anything
    to the device."""

    def __init__(self, layers):
        self.layers = [tuple(l) for l in layers]
        if not self.layers:
            raise ValueError('SpectralTable: no layers')
        self.dims = []
        for wbar, u, v in self.layers:
            cout, k = wbar.shape[0], wbar[0].numel()
            if tuple(u.shape) != (cout,) or tuple(v.shape) != (k,):
                raise ValueError('SpectralTable: weight_u %s / weight_v %s do not fit weight_bar %s' % (tuple(u.shape), tuple(v.shape), tuple(wbar.shape)))
            self.dims.append((cout, k))
        self.max_cout, self.max_k = max(d[0] for d in self.dims), max(d[1] for d in self.dims)
        self._key = self.table = self.last_out = None
        self.offsets, self.pass_elems, self.ws_doubles = [], 0, 0

    def ensure(self):
        key = tuple(t.data_ptr() for l in self.layers for t in l)
        if key == self._key:
            return
        import struct
        lib = _hip.lib()
        if lib.srhip_sn_entry_bytes() != 88:
            raise RuntimeError('SpectralTable: the library\'s layer descriptor is %d bytes, this table writes 88' % lib.srhip_sn_entry_bytes())
        blob, at, dat, self.offsets = bytearray(), 0, 0, []
        for (wbar, u, v), (cout, k) in zip(self.layers, self.dims):
            for t in (wbar, u, v):
                _require_gpu(t, 'spectral_weights')
                if not t.is_contiguous():
                    raise ValueError('spectral_weights: parameters must be contiguous')
            o = {}
            for name, n in (('sigma', 1), ('u', cout), ('v', k), ('s', cout), ('tpart', lib.srhip_sn_tpart_elems(cout, k)), ('weff', cout * k)):
                o[name] = at
                at += _align64(n)
            # SnEntry (csrc/sn.hip), 88 bytes: Q wbar, Q u, Q v | q off_sigma, off_weff, off_u, off_v, off_tpart, off_s (floats from the pass
            # buffer), q off_dpart (doubles from the backward's workspace) | i cout, i k
            blob += struct.pack('<QQQqqqqqqqii', wbar.data_ptr(), u.data_ptr(), v.data_ptr(), o['sigma'], o['weff'], o['u'], o['v'],
                                o['tpart'], o['s'], dat, cout, k)
            dat += lib.srhip_sn_dot_parts(cout, k)
            self.offsets.append(o)
        self.pass_elems, self.ws_doubles = at, dat
        self.table = torch.frombuffer(blob, dtype=torch.uint8).to(self.layers[0][0].device)
        self._key = key

    def forward(self):
        """One power iteration of every layer on the current stream; returns (pass buffer, [effective weights, views of it])."""
        self.ensure()
        wbar0 = self.layers[0][0]
        out = torch.empty(self.pass_elems, device=wbar0.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_sn_forward_batched(_p(self.table), len(self.layers), _p(out), self.max_cout, self.max_k, _stream()),
                   'sn_forward_batched')
        ws = []
        for (wbar, _, _), o in zip(self.layers, self.offsets):
            w = out[o['weff']:o['weff'] + wbar.numel()].view(wbar.shape)
            w._srhip_eff_packed = {}
            ws.append(w)
        self.last_out = out
        return out, ws

    def sigmas(self, out=None):
        """sigma of every layer as the pass that wrote `out` (default: the last pass) computed it."""
        out = self.last_out if out is None else out
        return torch.stack([out[o['sigma']] for o in self.offsets])

    def snapshot(self, out, i):
        """(u, v, sigma) of layer i as the pass that wrote `out` left them."""
        o, (cout, k) = self.offsets[i], self.dims[i]
        return out[o['u']:o['u'] + cout], out[o['v']:o['v'] + k], out[o['sigma']]

    def backward(self, out, grads, slots):
        """slots[i] += projection of grads[i] (None: layer skipped) with the (u, v, sigma) of the pass that wrote `out`."""
        self.ensure()
        n = len(self.layers)
        tab = ctypes.c_void_p * n
        gs = [g.contiguous() if g is not None else None for g in grads]
        for g, s, (wbar, _, _) in zip(gs, slots, self.layers):
            if g is not None:
                _require_gpu(g, 'sn_backward')
                if g.numel() != wbar.numel() or s is None or s.numel() != wbar.numel() or not s.is_contiguous():
                    raise ValueError('sn_backward: gradient / slot do not fit weight_bar %s' % (tuple(wbar.shape),))
        ws = torch.empty(max(self.ws_doubles, 1), device=out.device, dtype=torch.float64)
        _hip.check(_hip.lib().srhip_sn_backward_batched(_p(self.table), n, _p(out), tab(*[g.data_ptr() if g is not None else None for g in gs]),
                                                       tab(*[s.data_ptr() if (s is not None and g is not None) else None for g, s in zip(gs, slots)]),
                                                       _p(ws), self.max_cout, self.max_k, _stream()), 'sn_backward_batched')


class _SpectralWeights(Function):
    """(weight_bar, weight_u, weight_v) of every layer of the table -> the effective weights W = weight_bar / sigma of this pass.
    u and v advance IN PLACE on every call (train, eval, no_grad alike: the reference's SpectralNorm.forward); they are constants of
    the graph (no gradient), sigma depends on weight_bar.  The backward receives the gradients autograd has summed for each W (the
    first-order and the penalty's second-order contributions: the projection is linear) and projects them once, with the u, v and
    sigma THIS pass left in its buffer, straight into weight_bar's arena slot under direct_param_grads()."""

    @staticmethod
    def forward(ctx, table, *params):
        ctx.table = table
        ctx.out, ws = table.forward()
        ctx.set_materialize_grads(False)
        return tuple(ws)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        table, n = ctx.table, len(ctx.table.layers)
        wbars = [l[0] for l in table.layers]
        gs = [g if ctx.needs_input_grad[1 + i] else None for i, g in enumerate(gs)]
        ret = [None] * n
        if any(g is not None for g in gs) and not _skip_param_grads():
            slots = []
            for i, (g, wbar) in enumerate(zip(gs, wbars)):
                slot = _grad_slot(wbar) if g is not None else None
                if g is not None and slot is None:
                    slot = ret[i] = torch.zeros_like(wbar)
                slots.append(slot)
            table.backward(ctx.out, gs, slots)
        return (None,) + tuple(ret) + (None,) * (2 * n)


def spectral_weights(table):
    """The effective weights of one pass, in the table's layer order (one batched call; see _SpectralWeights)."""
    wbars, us, vs = zip(*table.layers)
    return _SpectralWeights.apply(table, *wbars, *us, *vs)


class _SumN(Function):
    """((t0 + t1) + t2) + ... in one pass (srhip_sum_n); every term gets the incoming gradient, as with chained adds."""

    @staticmethod
    def forward(ctx, tokens, *ts):
        _require_gpu(ts[0], 'sum_n')
        ts = [nhwc(t) for t in ts]
        out = torch.empty_like(ts[0], memory_format=CL)
        tab = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        _hip.check(_hip.lib().srhip_sum_n(tab, len(ts), _p(out), out.numel(), _stream()), 'sum_n')
        ctx.n, ctx.tokens = len(ts), tokens
        return out

    @staticmethod
    def backward(ctx, g):
        # a term that is the tagged input of a fused RAB (carry_open) gets no gradient edge: the RAB's data gradient adds g itself
        return (None,) + tuple(None if _carry_stash(tok, g) else g for tok in ctx.tokens)


def sum_tensors(ts):
    """Sum of 2..16 same-shape NCHW tensors in the order given (the generator's bus); falls back to chained adds otherwise."""
    ts = list(ts)
    if (2 <= len(ts) <= 16 and ts[0].is_cuda and ts[0].dim() == 4 and ts[0].numel() % 4 == 0
            and all(t.shape == ts[0].shape and t.dtype == torch.float32 for t in ts)):
        return _SumN.apply(tuple(_carry_commit(t) for t in ts), *ts)
    out = ts[0]
    for t in ts[1:]:
        out = out + t
    return out


class _CatChannels(Function):
    """torch.cat(dim = 1) of NHWC tensors in one pass (srhip_cat_channels); the backward splits the gradient back into dense tensors
    (srhip_split_channels).  Round 6: ATen's channels-last cat of the multi-scale block's three branches (sradsgan.py:340-344) took
    169 us for 72 MB on the one stream the generator's forward runs on."""

    @staticmethod
    def forward(ctx, *ts):
        _require_gpu(ts[0], 'cat_channels')
        ts = [nhwc(t) for t in ts]
        n, _, h, w = ts[0].shape
        chans = [t.shape[1] for t in ts]
        out = empty_nhwc(n, sum(chans), h, w, ts[0])
        tab = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        ctab = (ctypes.c_int * len(ts))(*chans)
        _hip.check(_hip.lib().srhip_cat_channels(tab, ctab, len(ts), _p(out), n * h * w, _stream()), 'cat_channels')
        ctx.chans, ctx.nhw = chans, (n, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        g = nhwc(g)
        n, h, w = ctx.nhw
        outs = [empty_nhwc(n, c, h, w, g) for c in ctx.chans]
        tab = (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
        ctab = (ctypes.c_int * len(outs))(*ctx.chans)
        _hip.check(_hip.lib().srhip_split_channels(_p(g), ctab, len(outs), tab, n * h * w, _stream()), 'split_channels')
        return tuple(outs)


def cat_channels(ts):
    """torch.cat(ts, dim=1) for 2..8 same-size fp32 NCHW tensors whose channel counts are multiples of 4; torch.cat otherwise."""
    ts = list(ts)
    if (2 <= len(ts) <= 8 and ts[0].is_cuda and all(t.dim() == 4 and t.dtype == torch.float32 and t.shape[1] % 4 == 0
                                                       and t.shape[0] == ts[0].shape[0] and t.shape[2:] == ts[0].shape[2:] for t in ts)):
        return _CatChannels.apply(*ts)
    return torch.cat(ts, dim=1)


# --------------------------------------------------------------------------------------------- #
# pixel shuffle (+ LeakyReLU) -- sradsgan.py:381-386
# --------------------------------------------------------------------------------------------- #


class _PixelShuffleAct(Function):
    @staticmethod
    def forward(ctx, x, r, slope):
        _require_gpu(x, 'pixel_shuffle')
        x = nhwc(x)
        n, c, h, w = x.shape
        cout = c // (r * r)
        out = empty_nhwc(n, cout, h * r, w * r, x)
        _hip.check(_hip.lib().srhip_pixel_shuffle_fwd(_p(x), _p(out), n, h, w, cout, r, float(slope or 0.0),
                                                      int(slope is not None), _stream()), 'pixel_shuffle_fwd')
        ctx.r, ctx.slope, ctx.in_shape = r, slope, (n, c, h, w)
        ctx.save_for_backward(out if slope is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        dout = nhwc(dout)
        n, c, h, w = ctx.in_shape
        din = empty_nhwc(n, c, h, w, dout)
        _hip.check(_hip.lib().srhip_pixel_shuffle_bwd(_p(dout), _p(out), _p(din), n, h, w, c // (ctx.r * ctx.r), ctx.r,
                                                      float(ctx.slope or 0.0), int(ctx.slope is not None), _stream()),
                   'pixel_shuffle_bwd')
        return din, None, None


def pixel_shuffle_act(x, r, slope=None):
    return _PixelShuffleAct.apply(x, r, slope)


# --------------------------------------------------------------------------------------------- #
# fused local-attention tail of RAB / ResGroup: CLAM -> SLAM -> conv1x1 (+bias) -> += skip
# (sradsgan.py:254-274, 303-323).  y = s*u and z = m*y are never written to HBM.
# --------------------------------------------------------------------------------------------- #


def _tail_forward(u, skip, fc1_w, fc2_w, w7, wc, bc, pool=None, out_pp=None):
    """returns (out, tensors to save for _tail_backward).  pool: (buffer, section bytes, nseg) from conv2d_fwd_pool_raw -- the
    pooling partials of u left behind by the conv that produced it (else the tail runs its own pooling pass)."""
    n, c, h, w = u.shape
    lib = _hip.lib()
    dev = u.device
    f32 = dict(device=dev, dtype=torch.float32)
    avg, mx, s = torch.empty(n, c, **f32), torch.empty(n, c, **f32), torch.empty(n, c, **f32)
    arg = torch.empty(n, c, device=dev, dtype=torch.int32)
    pooled, m = torch.empty(n * h * w, 2, **f32), torch.empty(n * h * w, **f32)
    argc = torch.empty(n * h * w, device=dev, dtype=torch.int32)
    fc1c, fc2c, w7c = fc1_w.detach().contiguous(), fc2_w.detach().contiguous(), w7.detach().contiguous()
    if pool is not None:
        _hip.check(lib.srhip_attn_tail_fwd_pooled(_p(u), _p(pool[0]), pool[1], pool[2], _p(fc1c), _p(fc2c), _p(w7c), _p(avg), _p(mx), _p(arg),
                                                  _p(s), _p(pooled), _p(argc), _p(m), n, h, w, c, fc1_w.shape[0], _stream()),
                   'attn_tail_fwd_pooled')
    else:
        ws = torch.empty(lib.srhip_attn_tail_workspace(n) // 4, **f32)
        _hip.check(lib.srhip_attn_tail_fwd(_p(u), _p(fc1c), _p(fc2c), _p(w7c), _p(avg), _p(mx), _p(arg), _p(s),
                                           _p(pooled), _p(argc), _p(m), _p(ws), ws.numel() * 4, n, h, w, c,
                                           fc1_w.shape[0], _stream()), 'attn_tail_fwd')
    out = conv2d_fwd_raw(u, wc, bc, 1, 0, None, skip, m, s, out_pp=out_pp)      # out_pp: the block output also as padded planes
    return out, (avg, mx, arg, s, pooled, argc, m)


def _tail_backward(g, u, fc1_w, fc2_w, w7, wc, bc, saved, has_bias, skip_params=False, du_pp=None):
    """g: gradient at the tail's output (NHWC).  Returns (du, dfc1, dfc2, dw7, dwc, dbc).  du_pp: a PP buffer that receives du as
    padded planes INSTEAD of the fp32 tensor (du is then returned as None)."""
    avg, mx, arg, s, pooled, argc, m = saved
    n, c, h, w = u.shape
    lib = _hip.lib()
    f32 = dict(device=u.device, dtype=torch.float32)
    dz = conv2d_dgrad_raw(g, wc, tuple(u.shape), 1, 0)            # gradient at z = m*s*u
    dwc = dbc = None
    if not skip_params:
        dwc, dbc = wgrad_for_params(wc, bc, u, g, 1, 0, has_bias, m, s)             # x operand = z, rebuilt on the fly
    du = torch.empty_like(u, memory_format=CL)
    hid = fc1_w.shape[0]
    g7 = None if skip_params else _grad_slot(w7)
    g1, g2 = (None, None) if skip_params else (_grad_slot(fc1_w), _grad_slot(fc2_w))
    direct = g1 is not None and g2 is not None
    dw7 = g7 if g7 is not None else torch.empty(w7.shape, **f32)
    dfc1 = g1 if direct else torch.empty(fc1_w.shape, **f32)
    dfc2 = g2 if direct else torch.empty(fc2_w.shape, **f32)
    # spatial half (7x7 conv, per-pixel gate), channel half (sigmoid -> shared MLP) and the arg-max fix-up: one call
    ws = torch.empty(lib.srhip_attn_tail_bwd_fused_workspace(n, h, w, hid) // 4, **f32)
    _hip.check(lib.srhip_attn_tail_bwd_pp(_p(dz), _p(u), _p(s), _p(m), _p(pooled), _p(argc), _p(avg), _p(mx), _p(arg),
                                              _p(w7.detach().contiguous()), _p(fc1_w.detach().contiguous()),
                                              _p(fc2_w.detach().contiguous()), _p(du), _p(du_pp.buf) if du_pp is not None else None, _p(dw7),
                                              int(g7 is not None), _p(dfc1), _p(dfc2),
                                              int(direct), _p(ws), ws.numel() * 4, n, h, w, c, hid, _stream()), 'attn_tail_bwd')
    if g7 is not None:
        dw7 = None
    if direct:
        dfc1 = dfc2 = None
    if du_pp is not None:
        du = None                  # the fp32 tensor only holds the main pass's partial result: the planes are the gradient
    return du, dfc1, dfc2, dw7, dwc, dbc


def _tail_eval_ok(u):
    """Inference fast path (srhip_attn_tail_eval): grad mode off, split-bf16 arithmetic, a CUDA tensor."""
    return not torch.is_grad_enabled() and u.is_cuda and get_conv_math() == 'bf16x3'


def _tail_forward_eval(u, skip, fc1_w, fc2_w, w7, wc, bc, pool=None):
    """conv1x1(SLAM(CLAM(u))) + bc + skip with nothing saved: two launches (sradsgan.py:254-274 in eval mode), one when the conv
    that produced u left the pooling partials behind (pool, see _tail_forward)."""
    u, skip = nhwc(u), nhwc(skip)
    n, c, h, w = u.shape
    lib = _hip.lib()
    out = torch.empty_like(u, memory_format=CL)
    if bc is not None:
        bc = _dense16(bc.detach())                # a parameter may be a view at any offset (torch.nn.utils.vector_to_parameters): the kernel reads float4
    if pool is not None:
        _hip.check(lib.srhip_attn_tail_eval_pooled(_p(u), _p(skip), _p(pool[0]), pool[1], pool[2], _p(fc1_w.detach().contiguous()),
                                                   _p(fc2_w.detach().contiguous()), _p(w7.detach().contiguous()), _p(packed_weight(wc, 0)),
                                                   _p(bc), _p(out), n, h, w, c, fc1_w.shape[0], _stream()), 'attn_tail_eval_pooled')
        return out
    ws = torch.empty(lib.srhip_attn_tail_workspace(n) // 4, device=u.device, dtype=torch.float32)
    _hip.check(lib.srhip_attn_tail_eval(_p(u), _p(skip), _p(fc1_w.detach().contiguous()), _p(fc2_w.detach().contiguous()),
                                        _p(w7.detach().contiguous()), _p(packed_weight(wc, 0)), _p(bc), _p(out), _p(ws), ws.numel() * 4,
                                        n, h, w, c, fc1_w.shape[0], _stream()), 'attn_tail_eval')
    return out


class _AttentionTail(Function):
    @staticmethod
    def forward(ctx, u, skip, fc1_w, fc2_w, w7, wc, bc, carry=None, emit_pp=False):
        _require_gpu(u, 'attention_tail')
        u, skip = nhwc(u), nhwc(skip)
        _state.last_out_pp = None
        out_pp = None
        if emit_pp:                                    # the output also as padded planes for the RAB that consumes it (attention_tail)
            n, c, h, wd = u.shape
            out_pp = plane_pool.get(n, c, h, wd, u.device)
        out, saved = _tail_forward(u, skip, fc1_w, fc2_w, w7, wc, bc, out_pp=out_pp)
        _state.last_out_pp = out_pp
        ctx.save_for_backward(u, fc1_w, fc2_w, w7, wc, bc, *saved)
        ctx.has_bias = bc is not None
        ctx.carry = carry              # token of a skip tensor whose gradient is stashed for the group's first RAB (carry_open)
        return out

    @staticmethod
    def backward(ctx, g):
        u, fc1_w, fc2_w, w7, wc, bc, *saved = ctx.saved_tensors
        g = nhwc(g)
        du, dfc1, dfc2, dw7, dwc, dbc = _tail_backward(g, u, fc1_w, fc2_w, w7, wc, bc, saved, ctx.has_bias,
                                                       _skip_param_grads(fc1_w, fc2_w, w7, wc, bc))
        dskip = None if _carry_stash(ctx.carry, g) else _passed_through(g)
        return du, dskip, dfc1, dfc2, dw7, dwc, dbc, None, None


class _RabBlock(Function):
    """Whole residual attention block (sradsgan.py:250-275) as ONE autograd node:
         t = LeakyReLU_0.2(conv1(x)) ; u = conv2(t) ; out = conv1x1(SLAM(CLAM(u))) + x
    Backward chains the fused kernels directly: conv2's dgrad applies conv1's activation mask in its
    epilogue, conv1's dgrad adds the skip gradient in its epilogue -- no lrelu-backward pass, no
    gradient-accumulation adds, 3 saved activations (x, t, u) instead of ~12."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, x_pp=None, emit_pp=False, carry=None, group_first=False):
        _require_gpu(x, 'rab_block')
        x = nhwc(x)
        ctx.carry = carry              # token under which the input's other consumers stash their gradients (carry_open)
        ctx.t_pp = ctx.x_pp = ctx.signs = None
        ctx.planes = False
        ctx.group_first = bool(group_first)   # the first block of a ResGroup: its backward closes the group's weight-gradient launch
        _state.last_out_pp = None
        if rab_planes_ok(x, w1, w2):
            # round 5: t stays in padded split-bf16 planes between the block's own kernels (conv1's epilogue writes them, conv2 reads
            # them without its in-place split, the backward's activation mask and weight gradient read them again).  x_pp: the block
            # input ALSO as planes, left by the previous block's tail (emit_pp): conv1 and its weight gradient read them
            n, _, h, wd = x.shape
            t_pp = plane_pool.get(n, w1.shape[0], h, wd, x.device)
            # conv1's epilogue also leaves the signs of t (1 bit per element): the mask conv2's data gradient applies
            ctx.signs = pp_sign_words(n, h, wd, w1.shape[0], x.device) if (_PP_SIGNS and b1 is not None and any(ctx.needs_input_grad)) else None
            conv2d_fwd_pp_raw(x_pp if x_pp is not None else x, w1, b1, 0.2, out_pp=t_pp, signs=ctx.signs)
            if pool_epilogue_ok(x, w2):
                u, pool = conv2d_fwd_pp_raw(t_pp, w2, b2, pool=True)
            else:
                u, pool = conv2d_fwd_pp_raw(t_pp, w2, b2), None
            out_pp = plane_pool.get(n, x.shape[1], h, wd, x.device) if emit_pp else None
            out, saved = _tail_forward(u, x, fc1_w, fc2_w, w7, wc, bc, pool, out_pp=out_pp)
            _state.last_out_pp = out_pp
            ctx.t_pp, ctx.x_pp = t_pp, x_pp
            ctx.planes = True
            ctx.save_for_backward(x, u, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, *saved)
            ctx.has_b = (b1 is not None, b2 is not None, bc is not None)
            return out
        t = conv2d_fwd_raw(x, w1, b1, 1, 1, 0.2)
        if pool_epilogue_ok(t, w2):                      # conv2 leaves the CLAM pooling partials of u behind (its epilogue, when the patch walk takes it)
            u, pool = conv2d_fwd_pool_raw(t, w2, b2)
        else:
            u, pool = conv2d_fwd_raw(t, w2, b2, 1, 1), None
        out, saved = _tail_forward(u, x, fc1_w, fc2_w, w7, wc, bc, pool)
        ctx.save_for_backward(x, t, u, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, *saved)
        ctx.has_b = (b1 is not None, b2 is not None, bc is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.t_pp is not None:
            return _RabBlock._backward_planes(ctx, g)
        if getattr(ctx, 'planes', False):
            # the pooled plane buffers (t, x, sign words) went back to the pool with the first backward: there is nothing to run a
            # second one on (retain_graph) -- say so instead of unpacking saved_tensors in the fp32 path's order
            raise RuntimeError('_RabBlock: backward called twice on the padded-plane path (its plane buffers are released by the first '
                               'backward); run the forward again')
        x, t, u, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, *saved = ctx.saved_tensors
        g = nhwc(g)
        skip = _skip_param_grads(w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc)      # one node, one decision: a listed parameter prunes the block's
        du, dfc1, dfc2, dw7, dwc, dbc = _tail_backward(g, u, fc1_w, fc2_w, w7, wc, bc, saved, ctx.has_b[2], skip)
        dt = conv2d_dgrad_raw(du, w2, tuple(t.shape), 1, 1, None, t, 0.2)          # * LeakyReLU'(t)
        dw2 = db2 = dw1 = db1 = None
        if not skip:
            dw2, db2 = wgrad_for_params(w2, b2, t, du, 1, 1, ctx.has_b[1])
        dx = conv2d_dgrad_raw(dt, w1, tuple(x.shape), 1, 1, g, extra=_carry_take(ctx.carry)) if ctx.needs_input_grad[0] else None   # + skip gradient (+ the input's stashed gradients)
        if not skip:
            dw1, db1 = wgrad_for_params(w1, b1, x, dt, 1, 1, ctx.has_b[0])
        return dx, dw1, db1, dw2, db2, dfc1, dfc2, dw7, dwc, dbc, None, None, None, None

    @staticmethod
    def _backward_planes(ctx, g):
        """The backward with t and dt as padded planes: conv2's dgrad reads the mask from t's hi plane and writes dt as planes, conv1's
        dgrad reads them without its split, both weight gradients run on the flat 8-wave kernel (the 64-channel operands x / du are
        converted on the weight-gradient stream)."""
        x, u, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, *saved = ctx.saved_tensors
        t_pp, ctx.t_pp = ctx.t_pp, None
        x_pp, ctx.x_pp = ctx.x_pp, None
        g = nhwc(g)
        skip = _skip_param_grads(w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc)      # one node, one decision: a listed parameter prunes the block's
        n, _, h, wd = x.shape
        # the tail's backward leaves du as fp32 (the gradient of the block's residual stream) AND as padded planes: conv2's data and
        # weight gradient read the planes (no in-kernel split, no conversion pass)
        du_pp = plane_pool.get(n, u.shape[1], h, wd, x.device)
        du, dfc1, dfc2, dw7, dwc, dbc = _tail_backward(g, u, fc1_w, fc2_w, w7, wc, bc, saved, ctx.has_b[2], skip, du_pp)
        dt_pp = plane_pool.get(n, w1.shape[0], h, wd, x.device)
        signs, ctx.signs = ctx.signs, None
        conv2d_dgrad_pp_raw(du_pp, w2, actmask=t_pp if signs is None else None, slope=0.2, out_pp=dt_pp, signs=signs)   # * LeakyReLU'(t), planes out
        dw2 = db2 = dw1 = db1 = None
        main = torch.cuda.current_stream()
        t_done = dt_done = False
        # (request order: conv1's data gradient first, weight gradients held back for a slot behind it, did not move the step: DESIGN.md, profiles/r06_step_ab.txt)
        if not skip:
            t_done = wgrad_pp_for_params(w2, b2, t_pp, du_pp, ctx.has_b[1], release=(t_pp, du_pp))
            if not t_done:                                # autograd wants the gradients returned: the fp32 path on converted operands
                dw2, db2 = wgrad_for_params(w2, b2, pp_to_f32(t_pp), pp_to_f32(du_pp), 1, 1, ctx.has_b[1])
        dx = conv2d_dgrad_pp_raw(dt_pp, w1, residual=g, extra=_carry_take(ctx.carry)) if ctx.needs_input_grad[0] else None   # + skip gradient (+ the input's stashed gradients)
        if not skip:
            dt_done = wgrad_pp_for_params(w1, b1, x_pp if x_pp is not None else x, dt_pp, ctx.has_b[0],
                                          release=(dt_pp,) if x_pp is None else (dt_pp, x_pp))
            if not dt_done:
                dw1, db1 = wgrad_for_params(w1, b1, x, pp_to_f32(dt_pp), 1, 1, ctx.has_b[0])
        if not t_done:
            plane_pool.put(t_pp, (main,))
            plane_pool.put(du_pp, (main,))
        if not dt_done:
            plane_pool.put(dt_pp, (main,))
            if x_pp is not None:
                plane_pool.put(x_pp, (main,))
        if ctx.group_first:
            flush_pending_pp()                            # a launch never straddles ResGroups: what the exchange's group-boundary flush finds is the same with and without it
        return dx, dw1, db1, dw2, db2, dfc1, dfc2, dw7, dwc, dbc, None, None, None, None


def rab_block(x, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, emit_pp=False, group_first=False):
    if _tail_eval_ok(x):                                 # inference: three conv-sized launches + the pooling partials per block
        _require_gpu(x, 'rab_block')
        x = nhwc(x)
        if rab_planes_ok(x, w1, w2):
            n, _, h, wd = x.shape
            t_pp = plane_pool.get(n, w1.shape[0], h, wd, x.device)
            conv2d_fwd_pp_raw(x, w1, b1, 0.2, out_pp=t_pp)
            if pool_epilogue_ok(x, w2):
                u, pool = conv2d_fwd_pp_raw(t_pp, w2, b2, pool=True)
            else:
                u, pool = conv2d_fwd_pp_raw(t_pp, w2, b2), None
            plane_pool.put(t_pp, (torch.cuda.current_stream(),))
            return _tail_forward_eval(u, x, fc1_w, fc2_w, w7, wc, bc, pool)
        t = conv2d_fwd_raw(x, w1, b1, 1, 1, 0.2)
        if pool_epilogue_ok(t, w2):
            u, pool = conv2d_fwd_pool_raw(t, w2, b2)
        else:
            u, pool = conv2d_fwd_raw(t, w2, b2, 1, 1), None
        return _tail_forward_eval(u, x, fc1_w, fc2_w, w7, wc, bc, pool)
    # emit_pp (the caller knows that another RAB consumes the output): the tail's 1x1 conv leaves the output also as padded planes; they
    # travel as an attribute of the output tensor (with its version counter: an in-place change of the tensor voids them)
    x_pp = None
    tag = getattr(x, '_srhip_pp', None) if _X_PP else None
    if tag is not None and tag[1] == x._version and tag[0].shape == tuple(x.shape):
        x_pp = tag[0]
    out = _RabBlock.apply(x, w1, b1, w2, b2, fc1_w, fc2_w, w7, wc, bc, x_pp, bool(emit_pp and _X_PP), getattr(x, '_srhip_carry', None) if _CARRY else None,
                          bool(group_first))
    pp, _state.last_out_pp = getattr(_state, 'last_out_pp', None), None
    if pp is not None:
        out._srhip_pp = (pp, out._version)
    return out


def attention_tail_supported(u, fc1_w, w7, wc):
    return (u.is_cuda and u.shape[1] == 64 and fc1_w.shape[0] <= 16 and tuple(w7.shape) == (1, 2, 7, 7)
            and tuple(wc.shape[:2]) == (64, 64))


def attention_tail(u, skip, fc1_w, fc2_w, w7, wc, bc, emit_pp=False):
    """conv1x1(SLAM(CLAM(u))) + bc + skip  for la_mode 'CA-SA', pool 'Avg|Max', addconv, C = 64.  emit_pp (the caller knows that a
    fused RAB consumes the output: a ResGroup followed by a ResGroup): the 1x1 conv leaves the output also as padded planes, which
    travel as an attribute of the output tensor like rab_block's -- the next group's first RAB and its weight gradient read them
    instead of running a conversion pass."""
    if _tail_eval_ok(u):
        _require_gpu(u, 'attention_tail')
        return _tail_forward_eval(u, skip, fc1_w, fc2_w, w7, wc, bc)
    emit = bool(emit_pp and _X_PP and get_conv_math() == 'bf16x3' and u.is_cuda)
    out = _AttentionTail.apply(u, skip, fc1_w, fc2_w, w7, wc, bc, _carry_commit(skip), emit)
    pp, _state.last_out_pp = getattr(_state, 'last_out_pp', None), None
    if pp is not None:
        out._srhip_pp = (pp, out._version)
    return out


# --------------------------------------------------------------------------------------------- #
# the tail's ablations (la_mode x pool_mode x addconv, sradsgan.py:215-324): csrc/attn_variants.hip computes the gates s [n,64] and
# m [n,hw] from u without materialising a gated activation, and the variant closes on the 1x1 conv with m and s as its row and channel
# scales ('-' modes with addconv), on the gated cat + the 128 -> 64 conv ('CA|SA'), or on one gate-and-add pass.  One autograd node
# per tail: it saves u and the small statistics; its backward is srhip_attn_var_bwd and the existing 1x1 conv gradients.  With grad
# mode off the same forward kernels run and nothing is saved, so an eval forward and a training forward have the same bits.
# --------------------------------------------------------------------------------------------- #

TAIL_ORDERS = {'CA-SA': 0, 'SA-CA': 1, 'CA': 2, 'SA': 3, 'CA|SA': 4}           # SRHIP_ATTN_* of include/sradsgan_hip.h
_VARIANT_SAVED = ('avg', 'mx', 'arg', 's', 'pooled', 'argc', 'm')


def attention_variant_supported(u, la_mode, fc1_w, w7):
    """The fused route of a non-default tail: C = 64, hidden <= 16, a 7x7 spatial kernel.  fc1_w / w7: None for a variant without
    that gate.  Otherwise the tail is the composition of the srhip_cbam_* primitives below."""
    return (la_mode in TAIL_ORDERS and u.is_cuda and u.dtype == torch.float32 and u.shape[1] == 64
            and (fc1_w is None or fc1_w.shape[0] <= 16) and (w7 is None or tuple(w7.shape[2:]) == (7, 7)))


def _det(p):
    return p.detach().contiguous() if p is not None else None


def attention_variant_gates(u, la_mode, pool_mode, fc1_w, fc2_w, w7):
    """(s [n,64] or None, m [n*hw] or None, the statistics as a dict) of srhip_attn_var_fwd for a dense NHWC u."""
    n, c, h, w = u.shape
    lib = _hip.lib()
    f32, i32 = dict(device=u.device, dtype=torch.float32), dict(device=u.device, dtype=torch.int32)
    rows = _pool_rows(pool_mode, 'attention_variant')
    has_c, has_s = 'CA' in la_mode, 'SA' in la_mode
    t = dict.fromkeys(_VARIANT_SAVED + ('ws',))
    if has_c:
        t['s'] = torch.empty(n, c, **f32)
        t['ws'] = torch.empty(max(lib.srhip_attn_var_workspace(n) // 4, 1), **f32)
        if 0 in rows:
            t['avg'] = torch.empty(n, c, **f32)
        if 1 in rows:
            t['mx'], t['arg'] = torch.empty(n, c, **f32), torch.empty(n, c, **i32)
    if has_s:
        t['pooled'], t['m'] = torch.empty(n * h * w, len(rows), **f32), torch.empty(n * h * w, **f32)
        if 1 in rows:
            t['argc'] = torch.empty(n * h * w, **i32)
    _hip.check(lib.srhip_attn_var_fwd(_p(u), _p(_det(fc1_w)), _p(_det(fc2_w)), _p(_det(w7)), _p(t['avg']), _p(t['mx']), _p(t['arg']),
                                      _p(t['s']), _p(t['pooled']), _p(t['argc']), _p(t['m']), _p(t['ws']),
                                      t['ws'].numel() * 4 if has_c else 0, n, h, w, c, fc1_w.shape[0] if has_c else 0,
                                      TAIL_ORDERS[la_mode], sum(1 << r for r in rows), _stream()), 'attn_var_fwd')
    return t['s'], t['m'], t


def _variant_cat(u, s, m):
    n, c, h, w = u.shape
    cat = empty_nhwc(n, 2 * c, h, w, u)
    _hip.check(_hip.lib().srhip_attn_var_close(_p(u), _p(s), _p(m), None, _p(cat), n, h * w, c, TAIL_ORDERS['CA|SA'], 1, _stream()),
               'attn_var_close')
    return cat


def _variant_forward(u, skip, la_mode, pool_mode, fc1_w, fc2_w, w7, wc, bc):
    """(tail(u) + skip, the statistics) for dense NHWC u, skip.  wc / bc: the closing 1x1 conv of the variants that have one ('-' modes
    with addconv: 64 -> 64; 'CA|SA': 128 -> 64), else None."""
    n, c, h, w = u.shape
    s, m, t = attention_variant_gates(u, la_mode, pool_mode, fc1_w, fc2_w, w7)
    if '-' in la_mode and wc is not None:
        return conv2d_fwd_raw(u, wc, bc, 1, 0, None, skip, m, s), t          # z = m s u is rebuilt inside the conv, as in _tail_forward
    if la_mode == 'CA|SA':
        return conv2d_fwd_raw(_variant_cat(u, s, m), wc, bc, 1, 0, None, skip), t
    out = torch.empty_like(u, memory_format=CL)
    _hip.check(_hip.lib().srhip_attn_var_close(_p(u), _p(s), _p(m), _p(skip), _p(out), n, h * w, c, TAIL_ORDERS[la_mode], 0, _stream()),
               'attn_var_close')
    return out, t


class _VariantTail(Function):
    @staticmethod
    def forward(ctx, u, skip, fc1_w, fc2_w, w7, wc, bc, la_mode, pool_mode):
        u, skip = nhwc(u), nhwc(skip)
        out, t = _variant_forward(u, skip, la_mode, pool_mode, fc1_w, fc2_w, w7, wc, bc)
        ctx.la_mode, ctx.pool_mode = la_mode, pool_mode
        ctx.save_for_backward(u, fc1_w, fc2_w, w7, wc, bc, *[t[k] for k in _VARIANT_SAVED])
        return out

    @staticmethod
    def backward(ctx, g):
        u, fc1_w, fc2_w, w7, wc, bc, avg, mx, arg, s, pooled, argc, m = ctx.saved_tensors
        g = nhwc(g)
        mode = ctx.la_mode
        n, c, h, w = u.shape
        lib = _hip.lib()
        f32 = dict(device=u.device, dtype=torch.float32)
        skip_params = _skip_param_grads(fc1_w, fc2_w, w7, wc, bc)
        dwc = dbc = None
        if mode == 'CA|SA':
            cat = _variant_cat(u, s, m)                               # the conv's x operand, rebuilt: one pass instead of a saved tensor
            dz = conv2d_dgrad_raw(g, wc, tuple(cat.shape), 1, 0)
            if not skip_params:
                dwc, dbc = wgrad_for_params(wc, bc, cat, g, 1, 0, bc is not None)
        elif '-' in mode and wc is not None:
            dz = conv2d_dgrad_raw(g, wc, tuple(u.shape), 1, 0)
            if not skip_params:
                dwc, dbc = wgrad_for_params(wc, bc, u, g, 1, 0, bc is not None, m, s)       # x operand = z, rebuilt on the fly
        else:
            dz = g
        has_c, has_s = s is not None, m is not None
        hid = fc1_w.shape[0] if has_c else 0
        g7 = _grad_slot(w7) if has_s and not skip_params else None
        g1, g2 = (_grad_slot(fc1_w), _grad_slot(fc2_w)) if has_c and not skip_params else (None, None)
        direct = g1 is not None and g2 is not None
        dw7 = g7 if g7 is not None else (torch.empty(w7.shape, **f32) if has_s else None)
        dfc1 = g1 if direct else (torch.empty(fc1_w.shape, **f32) if has_c else None)
        dfc2 = g2 if direct else (torch.empty(fc2_w.shape, **f32) if has_c else None)
        du = torch.empty_like(u, memory_format=CL)
        ws = torch.empty(lib.srhip_attn_var_bwd_workspace(n, h, w, hid) // 4, **f32)
        _hip.check(lib.srhip_attn_var_bwd(_p(dz), _p(u), _p(s), _p(m), _p(avg), _p(mx), _p(arg), _p(pooled), _p(argc), _p(_det(w7)),
                                          _p(_det(fc1_w)), _p(_det(fc2_w)), _p(du), _p(dw7), int(g7 is not None), _p(dfc1), _p(dfc2),
                                          int(direct), _p(ws), ws.numel() * 4, n, h, w, c, hid, TAIL_ORDERS[mode],
                                          sum(1 << r for r in _pool_rows(ctx.pool_mode, 'attention_variant')), _stream()), 'attn_var_bwd')
        if g7 is not None or skip_params:
            dw7 = None
        if direct or skip_params:
            dfc1 = dfc2 = None
        return du, _passed_through(g), dfc1, dfc2, dw7, dwc, dbc, None, None


def attention_variant(u, skip, la_mode, pool_mode, fc1_w, fc2_w, w7, wc, bc):
    """tail(u) + skip for any la_mode in TAIL_ORDERS (attention_variant_supported): one autograd node, or nothing saved with grad
    mode off."""
    _require_gpu(u, 'attention_variant')
    if not torch.is_grad_enabled():
        return _variant_forward(nhwc(u), nhwc(skip), la_mode, pool_mode, fc1_w, fc2_w, w7, wc, bc)[0]
    return _VariantTail.apply(u, skip, fc1_w, fc2_w, w7, wc, bc, la_mode, pool_mode)


# --------------------------------------------------------------------------------------------- #
# channel / spatial attention outside the fused RAB tail: the discriminator's ChannelAttention(256) /
# SpatialAttention (base_networks.py:366-457, sradsgan.py:495-496) and the stand-alone CLAM / SLAM modules.
# Built from the srhip_cbam_* primitives, whose backward passes are again primitives: every Function below is
# differentiable as often as autograd asks (the gradient penalty differentiates the discriminator twice).
# --------------------------------------------------------------------------------------------- #


def _nhwc_dims(x):
    n, c, h, w = x.shape
    return n, h * w, c


class _PoolHW(Function):
    """[n,c,h,w] -> t [n,2,c] = (mean, max) over pixels; the first arg-max pixel is remembered."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, 'cbam_pool_hw')
        x = nhwc(x)
        n, hw, c = _nhwc_dims(x)
        t = torch.empty(n, 2, c, device=x.device, dtype=torch.float32)
        arg = torch.empty(n, c, device=x.device, dtype=torch.int32)
        _hip.check(_hip.lib().srhip_cbam_pool_hw(_p(x), _p(t), _p(arg), 0, n, hw, c, _stream()), 'cbam_pool_hw')
        ctx.arg, ctx.shape = arg, tuple(x.shape)
        return t

    @staticmethod
    def backward(ctx, gt):
        return _UnpoolHW.apply(gt, ctx.arg, ctx.shape)


class _UnpoolHW(Function):
    """t [n,2,c] -> [n,c,h,w]: t0 / hw everywhere + t1 at the remembered arg-max pixel (adjoint of the pooling)."""

    @staticmethod
    def forward(ctx, t, arg, shape):
        t = t.contiguous()
        n, c, h, w = shape
        out = torch.empty(shape, device=t.device, dtype=torch.float32, memory_format=CL)     # (not empty().contiguous(CL): that is a copy kernel)
        _hip.check(_hip.lib().srhip_cbam_unpool_hw(_p(t), _p(arg), _p(out), n, h * w, c, _stream()), 'cbam_unpool_hw')
        ctx.arg = arg
        return out

    @staticmethod
    def backward(ctx, g):
        return _RepoolHW.apply(g, ctx.arg), None, None


class _RepoolHW(Function):
    """pooling at a GIVEN arg-max (linear in x)."""

    @staticmethod
    def forward(ctx, x, arg):
        x = nhwc(x)
        n, hw, c = _nhwc_dims(x)
        t = torch.empty(n, 2, c, device=x.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_cbam_pool_hw(_p(x), _p(t), _p(arg), 1, n, hw, c, _stream()), 'cbam_pool_hw')
        ctx.arg, ctx.shape = arg, tuple(x.shape)
        return t

    @staticmethod
    def backward(ctx, gt):
        return _UnpoolHW.apply(gt, ctx.arg, ctx.shape), None


class _PoolC(Function):
    """[n,c,h,w] -> t [n,2,h,w] (NHWC memory [n][hw][2]) = (mean, max) over channels; first arg-max channel remembered."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, 'cbam_pool_c')
        x = nhwc(x)
        n, c, h, w = x.shape
        t = empty_nhwc(n, 2, h, w, x)
        argc = torch.empty(n, h * w, device=x.device, dtype=torch.int32)
        _hip.check(_hip.lib().srhip_cbam_pool_c(_p(x), _p(t), _p(argc), 0, n, h * w, c, _stream()), 'cbam_pool_c')
        ctx.argc, ctx.shape = argc, tuple(x.shape)
        return t

    @staticmethod
    def backward(ctx, gt):
        return _UnpoolC.apply(gt, ctx.argc, ctx.shape)


class _UnpoolC(Function):
    @staticmethod
    def forward(ctx, t, argc, shape):
        t = nhwc(t)
        n, c, h, w = shape
        out = torch.empty(shape, device=t.device, dtype=torch.float32, memory_format=CL)     # (not empty().contiguous(CL): that is a copy kernel)
        _hip.check(_hip.lib().srhip_cbam_unpool_c(_p(t), _p(argc), _p(out), n, h * w, c, _stream()), 'cbam_unpool_c')
        ctx.argc = argc
        return out

    @staticmethod
    def backward(ctx, g):
        return _RepoolC.apply(g, ctx.argc), None, None


class _RepoolC(Function):
    @staticmethod
    def forward(ctx, x, argc):
        x = nhwc(x)
        n, c, h, w = x.shape
        t = empty_nhwc(n, 2, h, w, x)
        _hip.check(_hip.lib().srhip_cbam_pool_c(_p(x), _p(t), _p(argc), 1, n, h * w, c, _stream()), 'cbam_pool_c')
        ctx.argc, ctx.shape = argc, tuple(x.shape)
        return t

    @staticmethod
    def backward(ctx, gt):
        return _UnpoolC.apply(gt, ctx.argc, ctx.shape), None


class _Scale(Function):
    """x * s with s broadcast over pixels (mode 0, s [n,c]) or over channels (mode 1, s [n,hw]); bilinear."""

    @staticmethod
    def forward(ctx, x, s, mode):
        _require_gpu(x, 'cbam_scale')
        xc, sc = nhwc(x), s.contiguous()
        n, hw, c = _nhwc_dims(xc)
        out = torch.empty_like(xc, memory_format=CL)
        _hip.check(_hip.lib().srhip_cbam_scale(_p(xc), _p(sc), _p(out), n, hw, c, mode, _stream()), 'cbam_scale')
        ctx.mode = mode
        ctx.save_for_backward(x, s)
        return out

    @staticmethod
    def backward(ctx, g):
        x, s = ctx.saved_tensors
        dx = _Scale.apply(g, s, ctx.mode) if ctx.needs_input_grad[0] else None
        ds = _Dot.apply(g, x, ctx.mode).view(s.shape) if ctx.needs_input_grad[1] else None
        return dx, ds, None


class _Dot(Function):
    """sum over pixels (mode 0 -> [n,c]) or over channels (mode 1 -> [n,hw]) of a * b; bilinear."""

    @staticmethod
    def forward(ctx, a, b, mode):
        _require_gpu(a, 'cbam_dot')
        ac, bc = nhwc(a), nhwc(b)
        n, hw, c = _nhwc_dims(ac)
        out = torch.empty((n, c) if mode == 0 else (n, hw), device=a.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_cbam_dot(_p(ac), _p(bc), _p(out), n, hw, c, mode, _stream()), 'cbam_dot')
        ctx.mode = mode
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = _Scale.apply(b, g, ctx.mode) if ctx.needs_input_grad[0] else None
        db = _Scale.apply(a, g, ctx.mode) if ctx.needs_input_grad[1] else None
        return da, db, None


class _Sigmoid(Function):
    """pair == 0: elementwise; pair != 0: x [n,2,c] -> sigmoid(x[:,0] + x[:,1]) (the two MLP branches, base_networks.py:401)."""

    @staticmethod
    def forward(ctx, x, pair):
        _require_gpu(x, 'sigmoid')
        xc = x.contiguous()
        c = xc.shape[-1] if pair else 1
        y = torch.empty((xc.shape[0], c) if pair else tuple(xc.shape), device=x.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_sigmoid_fwd(_p(xc), _p(y), y.numel(), c, int(pair), _stream()), 'sigmoid_fwd')
        ctx.pair, ctx.xshape = pair, tuple(x.shape)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return _SigmoidBwd.apply(g, y, ctx.pair, ctx.xshape), None


class _SigmoidBwd(Function):
    @staticmethod
    def forward(ctx, g, y, pair, xshape):
        gc = g.contiguous()
        dx = torch.empty(xshape, device=g.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_sigmoid_bwd(_p(gc), _p(y), _p(dx), y.numel(), y.shape[-1] if pair else 1, int(pair), _stream()),
                   'sigmoid_bwd')
        ctx.pair = pair
        ctx.save_for_backward(g, y)
        return dx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gg):
        g, y = ctx.saved_tensors
        ggc, gc = gg.contiguous(), g.contiguous()
        dg = torch.empty_like(gc) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        _hip.check(_hip.lib().srhip_sigmoid_bwd_bwd(_p(ggc), _p(gc), _p(y), _p(dg), _p(dy), y.numel(),
                                                    y.shape[-1] if ctx.pair else 1, int(ctx.pair), _stream()), 'sigmoid_bwd_bwd')
        return dg, dy, None, None


POOL_MODES = ('Avg', 'Max', 'Avg|Max')


def _pool_rows(pool_mode, what):
    """indices into the (mean, max) pair of the pooling primitives that `pool_mode` keeps, Avg first like the reference's cat"""
    if pool_mode not in POOL_MODES:
        raise ValueError("%s: pool_mode must be one of %s, got %r" % (what, ', '.join(map(repr, POOL_MODES)), pool_mode))
    return [i for i, name in enumerate(('Avg', 'Max')) if name in pool_mode.split('|')]


def clam(x, fc1_w, fc2_w, pool_mode='Avg|Max'):
    """sradsgan.py:117-127 / base_networks.py:387-403: sigmoid(sum over the pools of MLP(pool x)) * x; the shared bias-free MLP is
    the reference's two 1x1 convs, applied to the stacked pooled rows in one pass.  A single pool takes its row of the (mean, max)
    pair: the other row's gradient is zero, so the pooling's adjoint scatters only what the pool saw."""
    rows_kept = _pool_rows(pool_mode, 'clam')
    n, c = x.shape[0], x.shape[1]
    k = len(rows_kept)
    t = _PoolHW.apply(x)                                                  # [n,2,c]
    if k == 1:
        t = t[:, rows_kept[0]].contiguous()                               # [n,c]
    rows = t.view(k * n, 1, 1, c).permute(0, 3, 1, 2)                     # logical [kn,c,1,1], NHWC memory: a free view
    hid = conv2d(rows, fc1_w, None, 1, 0, act_slope=0.0)                  # ReLU fused
    logits = conv2d(hid, fc2_w, None, 1, 0)                               # [kn,c,1,1]
    s = _Sigmoid.apply(logits.permute(0, 2, 3, 1).reshape(n, k, c) if k == 2 else logits.reshape(n, c), k == 2)   # [n,c]
    return _Scale.apply(x, s, 0)


def slam(x, w7, pool_mode='Avg|Max'):
    """sradsgan.py:141-151 / base_networks.py:440-457: sigmoid(conv kxk(the pooled maps, Avg first)) * x; w7 is [1,1,k,k] for a
    single pool, as in the reference's checkpoints."""
    rows_kept = _pool_rows(pool_mode, 'slam')
    n, c, h, w = x.shape
    pooled = _PoolC.apply(x)                                              # [n,2,h,w]
    if len(rows_kept) == 1:
        pooled = pooled[:, rows_kept[0]:rows_kept[0] + 1]
    logit = conv2d(pooled, w7, None, 1, w7.shape[-1] // 2)                # [n,1,h,w]
    m = _Sigmoid.apply(logit.reshape(n, h * w), False)
    return _Scale.apply(x, m, 1)


def _ws(nbytes, like):
    return torch.empty((max(int(nbytes), 4) + 3) // 4, device=like.device, dtype=torch.float32)


def _gamma_slot(gamma):
    """(buffer, accumulate flag) for a scalar attention gamma: its arena slot in direct_param_grads() mode."""
    g = _grad_slot(gamma)
    if g is not None:
        return g, 1
    return torch.empty(1, device=gamma.device, dtype=torch.float32), 0


class _Cgam(Function):
    """Channel global attention, sradsgan.py:202-212 (srhip_cgam_fwd / srhip_cgam_bwd)."""

    @staticmethod
    def forward(ctx, x, gamma):
        _require_gpu(x, 'cgam')
        x = nhwc(x)
        n, c, h, w = x.shape
        lib = _hip.lib()
        y = torch.empty_like(x, memory_format=CL)
        att = torch.empty(n, c, c, device=x.device, dtype=torch.float32)
        ws = _ws(lib.srhip_cgam_workspace(n, h * w), x)
        gam = gamma.detach().reshape(1).contiguous()
        _hip.check(lib.srhip_cgam_fwd(_p(x), _p(gam), _p(y), _p(att), _p(ws), ws.numel() * 4, n, h * w, c, _stream()),
                   'cgam_fwd')
        ctx.save_for_backward(x, att, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, att, gamma = ctx.saved_tensors
        dy = nhwc(dy)
        n, c, h, w = x.shape
        lib = _hip.lib()
        dx = torch.empty_like(x, memory_format=CL)
        skip = _skip_param_grads(gamma) or not ctx.needs_input_grad[1]
        dgam, acc = (None, 0) if skip else _gamma_slot(gamma)
        ws = _ws(lib.srhip_cgam_workspace(n, h * w), x)
        gam = gamma.detach().reshape(1).contiguous()
        _hip.check(lib.srhip_cgam_bwd(_p(dy), _p(x), _p(att), _p(gam), _p(dx), _p(dgam), acc, _p(ws), ws.numel() * 4,
                                      n, h * w, c, _stream()), 'cgam_bwd')
        return dx, (None if (skip or acc) else dgam.view(gamma.shape))


def cgam(x, gamma):
    """sradsgan.py:202-212; softmax(rowmax(E)-E) == softmax(-E) (shift invariance)."""
    return _Cgam.apply(x, gamma)


class _SgamCore(Function):
    """Position global attention on projected q, k, v (sradsgan.py:165-175): flash-style, no N x N tensor
    (srhip_sgam_flash_fwd / srhip_sgam_flash_bwd).  Saves q, k, v, o = softmax(qk^T) v and the per-query
    log-sum-exp."""

    @staticmethod
    def forward(ctx, x, q, k, v, gamma):
        _require_gpu(x, 'sgam')
        x, q, k, v = nhwc(x), nhwc(q), nhwc(k), nhwc(v)
        n, c, h, w = x.shape
        lib = _hip.lib()
        y = torch.empty_like(x, memory_format=CL)
        o = torch.empty_like(x, memory_format=CL)
        lse = torch.empty(n, h * w, device=x.device, dtype=torch.float32)
        gam = gamma.detach().reshape(1).contiguous()
        _hip.check(lib.srhip_sgam_flash_fwd(_p(q), _p(k), _p(v), _p(x), _p(gam), _p(y), _p(o), _p(lse), n, h * w,
                                            q.shape[1], c, _stream()), 'sgam_flash_fwd')
        ctx.save_for_backward(q, k, v, o, lse, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        q, k, v, o, lse, gamma = ctx.saved_tensors
        dy = nhwc(dy)
        n, c, h, w = v.shape
        lib = _hip.lib()
        dq, dk = torch.empty_like(q, memory_format=CL), torch.empty_like(k, memory_format=CL)
        dv = torch.empty_like(v, memory_format=CL)
        skip = _skip_param_grads(gamma) or not ctx.needs_input_grad[4]
        dgam, acc = (None, 0) if skip else _gamma_slot(gamma)
        ws = _ws(lib.srhip_sgam_flash_bwd_workspace(n, h * w), v)
        gam = gamma.detach().reshape(1).contiguous()
        _hip.check(lib.srhip_sgam_flash_bwd(_p(dy), _p(q), _p(k), _p(v), _p(o), _p(lse), _p(gam), _p(dq), _p(dk), _p(dv),
                                            _p(dgam), acc, _p(ws), ws.numel() * 4, n, h * w, q.shape[1], c, _stream()),
                   'sgam_flash_bwd')
        return _passed_through(dy), dq, dk, dv, (None if (skip or acc) else dgam.view(gamma.shape))


def sgam(x, q, k, v, gamma):
    """sradsgan.py:165-175 with q, k, v already projected by the 1x1 convs (:157-159)."""
    return _SgamCore.apply(x, q, k, v, gamma)


def _bn_reference_bwd(dy, x, y, gamma, eps, slope):
    """First-order backward of train-mode BN(+LeakyReLU) written with differentiable torch ops; only
    used to differentiate it once more (gradient penalty, sradsgan.py:621,639)."""
    n = x.numel() // x.shape[1]
    dz = dy if slope is None else dy * torch.where(y > 0, 1.0, float(slope))
    mean = x.mean((0, 2, 3), keepdim=True)
    var = x.var((0, 2, 3), unbiased=False, keepdim=True)
    invstd = torch.rsqrt(var + eps)
    xhat = (x - mean) * invstd
    dbeta = dz.sum((0, 2, 3))
    dgamma = (dz * xhat).sum((0, 2, 3))
    dx = (gamma.view(1, -1, 1, 1) * invstd) * (dz - dbeta.view(1, -1, 1, 1) / n - xhat * dgamma.view(1, -1, 1, 1) / n)
    return dx, dgamma, dbeta


_BN_BWD_X = os.environ.get('SRHIP_BN_BWD_X', '1') == '1'      # A/B knob: 0 = the BatchNorm backward reads y for the LeakyReLU mask (rounds 1-4)
_BN_FOLD = os.environ.get('SRHIP_BN_FOLD', '1') == '1'        # A/B knob: 0 = autograd sums a BatchNorm input's two gradients in the penalty's double backward


@contextlib.contextmanager
def bn_fold_second_order():
    """Around ONE backward through a gradient penalty's double-backward graph (sradsgan.py:621-639, 886): a BatchNorm input x receives two
    gradients there -- from the first-order backward's node (d penalty / d x through the batch statistics and the normalised value) and,
    later, from the forward node.  Inside this context the first is held back (not handed to autograd) and the forward node's backward
    adds it in its apply pass (srhip_bn_train_bwd_acc_xa, in place): one pass over three tensors less per BatchNorm layer.  The second-
    order nodes of a layer run before its forward node (their results feed it through the layers behind); a held-back gradient that
    no forward node has taken when the backward ends is an error, not a silent loss."""
    if not _BN_FOLD:
        yield
        return
    prev, _state.bn_fold = getattr(_state, 'bn_fold', None), {}
    ok = False
    try:
        yield
        ok = True
    finally:
        left, _state.bn_fold = _state.bn_fold, prev
        if ok and left:
            raise RuntimeError('bn_fold_second_order: %d BatchNorm input gradient(s) of the double backward were never taken by a forward node' % len(left))


class _BNTrainBwd(Function):
    @staticmethod
    def forward(ctx, dy, x, y, gamma, mean, invstd, eps, slope, acc_gamma=None, acc_beta=None, beta=None, addend=None):
        # addend (bn_fold_second_order): x's other gradient, added in the apply pass, in place (dx IS that buffer afterwards)
        # acc_gamma / acc_beta: the parameters' gradient slots (direct_param_grads mode): the kernel adds into them itself
        # (srhip_bn_train_bwd_acc) instead of two add launches per BatchNorm backward
        # NB: save the tensors autograd handed us (not layout-converted copies), or the second-order
        # graph through x / dy would be cut
        dyc, xc, yc = nhwc(dy), nhwc(x), nhwc(y)
        n, c, h, w = x.shape
        rows = n * h * w
        lib = _hip.lib()
        fold = addend is not None and beta is not None and slope is not None and _BN_BWD_X and addend.is_contiguous(memory_format=CL)
        dx = addend if fold else torch.empty_like(xc, memory_format=CL)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = torch.empty(lib.srhip_bn_workspace(rows, c) // 4, device=x.device, dtype=torch.float32)
        if fold:
            _hip.check(lib.srhip_bn_train_bwd_acc_xa(_p(dyc), _p(xc), _p(gamma.detach().contiguous()), _p(beta.detach().contiguous()), _p(mean),
                                                     _p(invstd), _p(addend), _p(dx), _p(dgamma), _p(dbeta), _p(acc_gamma), _p(acc_beta), _p(ws),
                                                     ws.numel() * 4, rows, c, float(slope), 1, _stream()), 'bn_train_bwd_xa')
        elif beta is not None and slope is not None and _BN_BWD_X:
            # the LeakyReLU mask from the recomputed pre-activation instead of a read of y (srhip_bn_train_bwd_acc_x): the same bits
            _hip.check(lib.srhip_bn_train_bwd_acc_x(_p(dyc), _p(xc), _p(gamma.detach().contiguous()), _p(beta.detach().contiguous()), _p(mean),
                                                    _p(invstd), _p(dx), _p(dgamma), _p(dbeta), _p(acc_gamma), _p(acc_beta), _p(ws),
                                                    ws.numel() * 4, rows, c, float(slope), 1, _stream()), 'bn_train_bwd_x')
        else:
            _hip.check(lib.srhip_bn_train_bwd_acc(_p(dyc), _p(xc), _p(yc), _p(gamma.detach().contiguous()), _p(mean), _p(invstd),
                                                  _p(dx), _p(dgamma), _p(dbeta), _p(acc_gamma), _p(acc_beta), _p(ws), ws.numel() * 4,
                                                  rows, c, float(slope or 0.0), int(slope is not None), _stream()), 'bn_train_bwd')
        if addend is not None and not fold:
            dx.add_(addend)
        ctx.eps, ctx.slope = eps, slope
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(dy, x, y, gamma, mean, invstd, beta)
        return dx, dgamma, dbeta

    @staticmethod
    def backward(ctx, ddx, ddgamma, ddbeta):
        dy, x, y, gamma, mean, invstd, beta = ctx.saved_tensors
        if ddx is None and ddgamma is None and ddbeta is None:
            return (None,) * 12
        if ddx is not None and ddgamma is None and ddbeta is None and not torch.is_grad_enabled():
            # the gradient-penalty case: one fused second-order pass (3 launches instead of ~40 ATen ops)
            uc, dyc, xc, yc = nhwc(ddx), nhwc(dy), nhwc(x), nhwc(y)
            n, c, h, w = x.shape
            rows = n * h * w
            lib = _hip.lib()
            g_dy, g_x = torch.empty_like(xc, memory_format=CL), torch.empty_like(xc, memory_format=CL)
            g_gamma = torch.empty_like(gamma)
            ws = torch.empty(lib.srhip_bn_bwd2_workspace(rows, c) // 4, device=x.device, dtype=torch.float32)
            slot = None if _skip_param_grads(gamma) else _grad_slot(gamma)   # direct_param_grads(): straight into the arena, by the kernel
            if beta is not None and ctx.slope is not None and _BN_BWD_X:
                _hip.check(lib.srhip_bn_train_bwd_bwd_acc_x(_p(uc), _p(dyc), _p(xc), _p(gamma.detach().contiguous()), _p(beta.detach().contiguous()),
                                                            _p(mean), _p(invstd), _p(g_dy), _p(g_x), _p(g_gamma), _p(slot), _p(ws),
                                                            ws.numel() * 4, rows, c, float(ctx.slope), 1, _stream()), 'bn_train_bwd_bwd_x')
            else:
                _hip.check(lib.srhip_bn_train_bwd_bwd_acc(_p(uc), _p(dyc), _p(xc), _p(yc), _p(gamma.detach().contiguous()),
                                                          _p(mean), _p(invstd), _p(g_dy), _p(g_x), _p(g_gamma), _p(slot), _p(ws),
                                                          ws.numel() * 4, rows, c, float(ctx.slope or 0.0),
                                                          int(ctx.slope is not None), _stream()), 'bn_train_bwd_bwd')
            if slot is not None:
                g_gamma = None
            fold = getattr(_state, 'bn_fold', None)
            if fold is not None and ctx.needs_input_grad[1] and (x.data_ptr(), tuple(x.shape)) not in fold:
                fold[(x.data_ptr(), tuple(x.shape))] = g_x     # (bn_fold_second_order) the forward node of this layer adds it to its own
                g_x = None
            return g_dy, g_x, None, g_gamma, None, None, None, None, None, None, None, None
        with torch.enable_grad():
            dy_, x_, g_ = (t.detach().requires_grad_(True) for t in (dy, x, gamma))
            outs = _bn_reference_bwd(dy_, x_, y, g_, ctx.eps, ctx.slope)
            pairs = [(o, d) for o, d in zip(outs, (ddx, ddgamma, ddbeta)) if d is not None]
            gdy, gx, gg = torch.autograd.grad([o for o, _ in pairs], [dy_, x_, g_], [d for _, d in pairs],
                                              allow_unused=True)
        return gdy, gx, None, gg, None, None, None, None, None, None, None, None


class _BNTrainFwd(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, slope):
        _require_gpu(x, 'batch_norm')
        xc = nhwc(x)
        n, c, h, w = x.shape
        rows = n * h * w
        lib = _hip.lib()
        y = torch.empty_like(xc, memory_format=CL)
        mean, invstd = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = torch.empty(lib.srhip_bn_workspace(rows, c) // 4, device=x.device, dtype=torch.float32)
        _hip.check(lib.srhip_bn_train_fwd(_p(xc), _p(gamma.detach().contiguous()), _p(beta.detach().contiguous()),
                                          _p(running_mean), _p(running_var), _p(y), _p(mean), _p(invstd), _p(ws),
                                          ws.numel() * 4, rows, c, float(eps), float(momentum), float(slope or 0.0),
                                          int(slope is not None), _stream()), 'bn_train_fwd')
        ctx.eps, ctx.slope = eps, slope
        ctx.save_for_backward(x, y, gamma, mean, invstd, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, invstd, beta = ctx.saved_tensors
        fold = getattr(_state, 'bn_fold', None)
        held = fold.pop((x.data_ptr(), tuple(x.shape)), None) if (fold and not torch.is_grad_enabled()) else None
        if not torch.is_grad_enabled() and not _skip_param_grads(gamma, beta):
            # direct_param_grads(): add into the arena slots here, on the stream this node runs on, instead of handing the
            # gradients to autograd -- its AccumulateGrad nodes run on the stream the parameter was FIRST used on in this
            # iteration (the main stream, D(gen_hr)), which would make the main stream wait for the D stream's backward
            gg, gb = _grad_slot(gamma), _grad_slot(beta)
            if gg is not None and gb is not None:
                dx, _, _ = _BNTrainBwd.apply(dy, x, y, gamma, mean, invstd, ctx.eps, ctx.slope, gg, gb, beta, held)
                return dx, None, None, None, None, None, None, None
        dx, dgamma, dbeta = _BNTrainBwd.apply(dy, x, y, gamma, mean, invstd, ctx.eps, ctx.slope, None, None, beta, held)
        return dx, dgamma, dbeta, None, None, None, None, None


def batch_norm_act(x, bn, slope=None):
    """Train-mode BatchNorm2d + LeakyReLU (sradsgan.py:478-479) on the fused HIP kernels; updates the
    running statistics like nn.BatchNorm2d (momentum 0.1, unbiased running_var).  Twice differentiable."""
    if not bn.training:
        # eval(): running statistics, a per-channel affine (SRGAN's generator at validation time; the SRADSGAN
        # discriminator is never put in eval()).  Inference only: srhip_bn_eval_fwd has no backward.
        _require_gpu(x, 'batch_norm')
        if torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad):
            raise NotImplementedError('batch_norm_act: eval()-mode BatchNorm is built for inference only (wrap the call in '
                                      'torch.no_grad()); training through frozen statistics is not on the SRADSGAN path')
        xc = nhwc(x)
        n, c, h, w = xc.shape
        y = torch.empty_like(xc, memory_format=CL)
        _hip.check(_hip.lib().srhip_bn_eval_fwd(_p(xc), _p(bn.weight.detach().contiguous()), _p(bn.bias.detach().contiguous()),
                                                _p(bn.running_mean), _p(bn.running_var), _p(y), n * h * w, c, float(bn.eps),
                                                float(slope or 0.0), int(slope is not None), _stream()), 'bn_eval_fwd')
        return y
    y = _BNTrainFwd.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, slope)
    with torch.no_grad():
        bn.num_batches_tracked += 1
    stash = getattr(bn, '_stat_stash', None)
    if stash is not None and y.grad_fn is not None:
        # (batch mean, invstd, count) of this call, so the caller can replay the running-statistics update
        # of a forward pass it does not recompute (TrainStep: D(fake) == D(gen_hr))
        x_, y_, g_, mean, invstd, b_ = y.grad_fn.saved_tensors
        stash.append((bn, mean, invstd, x.numel() // x.shape[1]))
    return y


def replay_bn_update(stash):
    """Applies nn.BatchNorm2d's running-statistics update once more for every stashed (bn, mean, invstd, n)."""
    if not stash:
        return
    with torch.no_grad():
        if len({(bn.momentum, bn.eps) for bn, _, _, _ in stash}) == 1 and len(stash) > 1:
            # one launch per arithmetic step for all layers (the same element-wise operations as the per-layer form below)
            bn0 = stash[0][0]
            m, eps = bn0.momentum, bn0.eps
            var = torch._foreach_pow([t[2] for t in stash], -2)
            torch._foreach_sub_(var, eps)
            torch._foreach_mul_(var, [n / max(n - 1, 1) for _, _, _, n in stash])
            rm, rv = [t[0].running_mean for t in stash], [t[0].running_var for t in stash]
            torch._foreach_mul_(rm, 1 - m)
            torch._foreach_add_(rm, [t[1] for t in stash], alpha=m)
            torch._foreach_mul_(rv, 1 - m)
            torch._foreach_add_(rv, var, alpha=m)
            torch._foreach_add_([t[0].num_batches_tracked for t in stash], 1)
            return
        for bn, mean, invstd, n in stash:
            var = invstd.pow(-2) - bn.eps
            bn.running_mean.mul_(1 - bn.momentum).add_(mean, alpha=bn.momentum)
            bn.running_var.mul_(1 - bn.momentum).add_(var * (n / max(n - 1, 1)), alpha=bn.momentum)
            bn.num_batches_tracked += 1


# --------------------------------------------------------------------------------------------- #
# per-sample normalisations of the patch discriminator (gn.hip): instance norm and the reference's GroupNorm, + LeakyReLU
# --------------------------------------------------------------------------------------------- #


def _gn_reference_bwd(dy, x, gamma, beta, groups, eps, unbiased, slope):
    """First-order backward of group_norm_act written with differentiable torch ops; only used to differentiate it once more with
    cotangents the fused second-order pass does not take (like _bn_reference_bwd).  The LeakyReLU mask is a constant."""
    n, c, h, w = x.shape
    cpg = c // groups
    m = cpg * h * w
    k = m / (m - 1.0) if unbiased else 1.0

    def E(t):
        return t.reshape(n, groups, -1).mean(-1).repeat_interleave(cpg, 1).view(n, c, 1, 1)

    mean = E(x)
    invstd = torch.rsqrt(k * E((x - mean) ** 2) + eps)
    xhat = (x - mean) * invstd
    ga = gamma.view(1, c, 1, 1) if gamma is not None else 1.0
    dz = dy
    if slope is not None:
        with torch.no_grad():
            z = xhat * ga + (beta.view(1, c, 1, 1) if beta is not None else 0.0)
            mask = torch.where(z > 0, 1.0, float(slope))
        dz = dy * mask
    a = dz * ga
    dx = invstd * (a - E(a) - k * xhat * E(a * xhat))
    if gamma is None:
        return dx, None, None
    return dx, (dz * xhat).sum((0, 2, 3)).view_as(gamma), dz.sum((0, 2, 3)).view_as(gamma)


def _gn_dims(x, groups):
    n, c, h, w = x.shape
    return n, h * w, c, groups


def _gn_ws(lib, n, p, c, like):
    return torch.empty(lib.srhip_gn_workspace(n, p, c) // 4, device=like.device, dtype=torch.float32)


def _flat(t):
    return None if t is None else t.detach().reshape(-1)


class _GNBwd(Function):
    @staticmethod
    def forward(ctx, dy, x, gamma, beta, mean, invstd, groups, eps, unbiased, slope, acc_gamma=None, acc_beta=None):
        # acc_gamma / acc_beta: the parameters' gradient slots (direct_param_grads mode), added into by the kernel itself
        # NB: save the tensors autograd handed us (not layout-converted copies), or the second-order graph through x / dy would be cut
        dyc, xc = nhwc(dy), nhwc(x)
        n, p, c, _ = _gn_dims(x, groups)
        lib = _hip.lib()
        dx = torch.empty_like(xc, memory_format=CL)
        dgamma, dbeta = (torch.empty_like(gamma), torch.empty_like(gamma)) if gamma is not None else (None, None)
        ws = _gn_ws(lib, n, p, c, x)
        _hip.check(lib.srhip_gn_bwd(_p(dyc), _p(xc), _p(_flat(gamma)), _p(_flat(beta)), _p(mean), _p(invstd), None, _p(dx), _p(dgamma),
                                    _p(dbeta), _p(acc_gamma), _p(acc_beta), _p(ws), ws.numel() * 4, n, p, c, groups, int(unbiased),
                                    float(slope or 0.0), int(slope is not None), _stream()), 'gn_bwd')
        ctx.cfg = (groups, eps, unbiased, slope)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(dy, x, gamma, beta, mean, invstd)
        return dx, dgamma, dbeta

    @staticmethod
    def backward(ctx, ddx, ddgamma, ddbeta):
        dy, x, gamma, beta, mean, invstd = ctx.saved_tensors
        groups, eps, unbiased, slope = ctx.cfg
        if ddx is None and ddgamma is None and ddbeta is None:
            return (None,) * 12
        if ddx is not None and ddgamma is None and ddbeta is None and not torch.is_grad_enabled():
            # the gradient-penalty case: one fused second-order pass
            uc, dyc, xc = nhwc(ddx), nhwc(dy), nhwc(x)
            n, p, c, _ = _gn_dims(x, groups)
            lib = _hip.lib()
            g_dy, g_x = torch.empty_like(xc, memory_format=CL), torch.empty_like(xc, memory_format=CL)
            g_gamma = torch.empty_like(gamma) if gamma is not None else None
            ws = _gn_ws(lib, n, p, c, x)
            slot = None if (gamma is None or _skip_param_grads(gamma)) else _grad_slot(gamma)   # direct_param_grads(): straight into the arena
            _hip.check(lib.srhip_gn_bwd_bwd(_p(uc), _p(dyc), _p(xc), _p(_flat(gamma)), _p(_flat(beta)), _p(mean), _p(invstd), _p(g_dy), _p(g_x),
                                            _p(g_gamma), _p(slot), _p(ws), ws.numel() * 4, n, p, c, groups, int(unbiased),
                                            float(slope or 0.0), int(slope is not None), _stream()), 'gn_bwd_bwd')
            if slot is not None:
                g_gamma = None
            return (g_dy, g_x, g_gamma) + (None,) * 9
        with torch.enable_grad():
            dy_, x_ = dy.detach().requires_grad_(True), x.detach().requires_grad_(True)
            g_ = gamma.detach().requires_grad_(True) if gamma is not None else None
            outs = _gn_reference_bwd(dy_, x_, g_, beta, groups, eps, unbiased, slope)
            pairs = [(o, d) for o, d in zip(outs, (ddx, ddgamma, ddbeta)) if d is not None and o is not None]
            ins = [dy_, x_] + ([g_] if g_ is not None else [])
            got = torch.autograd.grad([o for o, _ in pairs], ins, [d for _, d in pairs], allow_unused=True)
        return (got[0], got[1], got[2] if g_ is not None else None) + (None,) * 9


class _GNFwd(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, unbiased, slope):
        _require_gpu(x, 'group_norm')
        xc = nhwc(x)
        n, p, c, _ = _gn_dims(x, groups)
        lib = _hip.lib()
        y = torch.empty_like(xc, memory_format=CL)
        mean = torch.empty(n * groups, device=x.device, dtype=torch.float32)
        invstd = torch.empty_like(mean)
        ws = _gn_ws(lib, n, p, c, x)
        _hip.check(lib.srhip_gn_fwd(_p(xc), _p(_flat(gamma)), _p(_flat(beta)), _p(y), _p(mean), _p(invstd), _p(ws), ws.numel() * 4, n, p, c,
                                    groups, int(unbiased), float(eps), float(slope or 0.0), int(slope is not None), _stream()), 'gn_fwd')
        ctx.cfg = (groups, eps, unbiased, slope)
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        groups, eps, unbiased, slope = ctx.cfg
        if gamma is not None and not torch.is_grad_enabled() and not _skip_param_grads(gamma, beta):
            # direct_param_grads(): into the arena slots here, on the stream this node runs on (see _BNTrainFwd.backward)
            gg, gb = _grad_slot(gamma), _grad_slot(beta)
            if gg is not None and gb is not None:
                dx, _, _ = _GNBwd.apply(dy, x, gamma, beta, mean, invstd, groups, eps, unbiased, slope, gg, gb)
                return dx, None, None, None, None, None, None
        dx, dgamma, dbeta = _GNBwd.apply(dy, x, gamma, beta, mean, invstd, groups, eps, unbiased, slope)
        return dx, dgamma, dbeta, None, None, None, None


def group_norm_act(x, groups, weight=None, bias=None, eps=1e-5, unbiased=False, slope=None):
    """Per-sample, per-group normalisation + LeakyReLU on the fused HIP kernels (gn.hip): nn.InstanceNorm2d(C) is groups = C with the
    biased variance and no affine; the reference's GroupNorm (base_networks.py:12-31) is groups = 32 with the UNBIASED variance and
    weight / bias of shape (1, C, 1, 1).  x: any memory format; returns channels-last.  Twice differentiable."""
    if (weight is None) != (bias is None):
        raise ValueError('group_norm_act: weight and bias are given or left out together')
    if weight is not None and (weight.numel() != x.shape[1] or not weight.is_contiguous() or not bias.is_contiguous()):
        raise ValueError('group_norm_act: weight and bias hold one contiguous value per channel')
    return _GNFwd.apply(x, weight, bias, int(groups), float(eps), bool(unbiased), slope)


def max_pool2x2_raw(x):
    _require_gpu(x, 'max_pool2x2')
    x = nhwc(x)
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, h // 2, w // 2, x)
    _hip.check(_hip.lib().srhip_maxpool2x2_fwd(_p(x), _p(y), n, h, w, c, _stream()), 'maxpool2x2_fwd')
    return y


def max_pool3x3s2_raw(x):
    """nn.MaxPool2d(kernel_size=3, stride=2) (AlexNet features[2] / [5]): floor mode, no padding.  Its backward: max_pool3x3s2_bwd_raw."""
    _require_gpu(x, 'max_pool3x3s2')
    x = nhwc(x)
    n, c, h, w = x.shape
    if h < 3 or w < 3:
        raise ValueError('max_pool3x3s2: needs H, W >= 3, got %d x %d' % (h, w))
    y = empty_nhwc(n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1, x)
    _hip.check(_hip.lib().srhip_maxpool3x3s2_fwd(_p(x), _p(y), n, h, w, c, _stream()), 'maxpool3x3s2_fwd')
    return y


def lpips_stem_raw(x, w_hwio, bias, normalize=True, out=None):
    """Scaling layer + AlexNet conv1 + ReLU (srhip_lpips_stem).  x: [M,3,H,W]; w_hwio: the weight as a dense [11,11,3,64] tensor; out: an
    NHWC [M,64,Ho,Wo] tensor (or a batch slice of one) to write into."""
    _require_gpu(x, 'lpips_stem')
    x = nhwc(x)
    m, c, h, w = x.shape
    if c != 3 or tuple(w_hwio.shape) != (11, 11, 3, 64) or not w_hwio.is_contiguous():
        raise ValueError('lpips_stem: needs a 3-channel image and a dense [11, 11, 3, 64] weight')
    if h < 7 or w < 7:
        raise ValueError('lpips_stem: needs H, W >= 7, got %d x %d' % (h, w))
    ho, wo = _out_hw(h, w, 11, 4, 2)
    y = empty_nhwc(m, 64, ho, wo, x) if out is None else out
    if tuple(y.shape) != (m, 64, ho, wo) or not y.is_contiguous(memory_format=CL):
        raise ValueError('lpips_stem: out must be a dense NHWC %s tensor' % ((m, 64, ho, wo),))
    _hip.check(_hip.lib().srhip_lpips_stem(_p(x), _p(w_hwio), _p(bias.detach().contiguous()), _p(y), m, h, w, int(bool(normalize)),
                                           _stream()), 'lpips_stem')
    return y


def lpips_head_raw(f, pairs, w, partial):
    """One tap of the LPIPS head (srhip_lpips_head).  f: [M,C,h,w] features; pairs: int32 [P,2] on the device (indices into M, checked by
    the caller); w: [C]; partial: float64 [P, srhip_lpips_blocks()] that receives the pixel sums."""
    _require_gpu(f, 'lpips_head')
    f = nhwc(f)
    m, c, h, wd = f.shape
    npairs = pairs.shape[0]
    if pairs.dtype != torch.int32 or not pairs.is_cuda or not pairs.is_contiguous() or w.numel() != c:
        raise ValueError('lpips_head: pairs must be a dense int32 [P, 2] device tensor and w must have C elements')
    _hip.check(_hip.lib().srhip_lpips_head(_p(f), _p(pairs), _p(w.detach().contiguous()), _p(partial), m, npairs, h, wd, c, _stream()),
               'lpips_head')
    return partial


def lpips_finish_raw(partial, tap_pixels, out=None):
    """partial: float64 [T,P,blocks]; tap_pixels: h * w of each tap -> float64 [P] = sum over taps of the pixel means."""
    ntaps, npairs = partial.shape[0], partial.shape[1]
    out = torch.empty(npairs, device=partial.device, dtype=torch.float64) if out is None else out
    counts = (ctypes.c_long * ntaps)(*[int(v) for v in tap_pixels])
    _hip.check(_hip.lib().srhip_lpips_finish(_p(partial), counts, ntaps, npairs, _p(out), _stream()), 'lpips_finish')
    return out


def lpips_head_bwd_raw(f, pairs, w, upstream, count):
    """One tap's gradient of the LPIPS head with respect to the pred features, through the tap's ReLU (srhip_lpips_head_bwd).  f:
    [M,C,h,w] features of all images; pairs: int32 [P,2] on the device, (target index, pred index) per pair; w: [C]; upstream: a
    float32 device scalar; count: the number of values the mean runs over (N * h * w) -> [P,C,h,w].  A pixel whose pred features are
    all zero gets zeros (torch autograd yields NaN there)."""
    _require_gpu(f, 'lpips_head_bwd')
    f = nhwc(f)
    m, c, h, wd = f.shape
    npairs = pairs.shape[0]
    if pairs.dtype != torch.int32 or not pairs.is_cuda or not pairs.is_contiguous() or w.numel() != c:
        raise ValueError('lpips_head_bwd: pairs must be a dense int32 [P, 2] device tensor and w must have C elements')
    if upstream.dtype != torch.float32 or not upstream.is_cuda or upstream.numel() != 1:
        raise ValueError('lpips_head_bwd: upstream must be a float32 device scalar')
    df = empty_nhwc(npairs, c, h, wd, f)
    _hip.check(_hip.lib().srhip_lpips_head_bwd(_p(f), _p(pairs), _p(w.detach().contiguous()), _p(upstream), 1.0 / float(count), _p(df), m,
                                               npairs, h, wd, c, _stream()), 'lpips_head_bwd')
    return df


def max_pool3x3s2_bwd_raw(x, dy, relu=False, residual=None):
    """Backward of nn.MaxPool2d(3, 2) in gather form (srhip_maxpool3x3s2_bwd): dx = gather(dy) [* (x > 0)] [+ residual], x the pool's
    input.  The first maximum of a window in scan order takes its gradient, as in ATen."""
    _require_gpu(x, 'max_pool3x3s2_bwd')
    _require_gpu(dy, 'max_pool3x3s2_bwd')
    x, dy = nhwc(x), nhwc(dy)
    n, c, h, w = x.shape
    if h < 3 or w < 3 or tuple(dy.shape) != (n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1):
        raise ValueError('max_pool3x3s2_bwd: dy %s is not the pooled shape of x %s' % (tuple(dy.shape), tuple(x.shape)))
    if residual is not None:
        _require_gpu(residual, 'max_pool3x3s2_bwd')
        residual = nhwc(residual)
        if residual.shape != x.shape:
            raise ValueError('max_pool3x3s2_bwd: residual %s must have the shape of x %s' % (tuple(residual.shape), tuple(x.shape)))
    dx = empty_nhwc(n, c, h, w, x)
    _hip.check(_hip.lib().srhip_maxpool3x3s2_bwd(_p(x), _p(dy), _p(residual), _p(dx), n, h, w, c, int(bool(relu)), _stream()),
               'maxpool3x3s2_bwd')
    return dx


def lpips_stem_bwd_raw(g, w_hwio, image_hw, normalize=True):
    """Data gradient of the LPIPS stem back to the image, scaling layer included (srhip_lpips_stem_bwd).  g: [M,64,Ho,Wo], the gradient
    at the stem conv's output with the ReLU mask applied; w_hwio: the dense [11,11,3,64] weight; image_hw: (H, W) -> [M,3,H,W]."""
    _require_gpu(g, 'lpips_stem_bwd')
    g = nhwc(g)
    h, w = image_hw
    if tuple(w_hwio.shape) != (11, 11, 3, 64) or not w_hwio.is_contiguous():
        raise ValueError('lpips_stem_bwd: needs a dense [11, 11, 3, 64] weight')
    if h < 7 or w < 7 or tuple(g.shape[1:]) != (64,) + _out_hw(h, w, 11, 4, 2):
        raise ValueError('lpips_stem_bwd: g %s is not the stem output of a %d x %d image' % (tuple(g.shape), h, w))
    m = g.shape[0]
    dx = empty_nhwc(m, 3, h, w, g)
    _hip.check(_hip.lib().srhip_lpips_stem_bwd(_p(g), _p(w_hwio), _p(dx), m, h, w, int(bool(normalize)), _stream()), 'lpips_stem_bwd')
    return dx


_POOL_IDX = os.environ.get('SRHIP_POOL_IDX', '1') == '1'       # A/B knob: 0 = the max-pool backward re-reads the pool's input


def max_pool2x2_idx_raw(x):
    """(y, rec): the pool and its 2-byte records per 4 outputs (arg-max position + "maximum > 0"), which max_pool2x2_bwd_idx_raw reads
    instead of x."""
    _require_gpu(x, 'max_pool2x2')
    x = nhwc(x)
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, h // 2, w // 2, x)
    rec = torch.empty(n * (h // 2) * (w // 2) * (c // 4), device=x.device, dtype=torch.int16)
    _hip.check(_hip.lib().srhip_maxpool2x2_fwd_idx(_p(x), _p(y), _p(rec), n, h, w, c, _stream()), 'maxpool2x2_fwd_idx')
    return y, rec


def max_pool2x2_bwd_idx_raw(dy, rec, x_shape, relu_input):
    dy = nhwc(dy)
    n, c, h, w = x_shape
    dx = torch.empty(n, h, w, c, device=dy.device, dtype=torch.float32).permute(0, 3, 1, 2)
    _hip.check(_hip.lib().srhip_maxpool2x2_bwd_idx(_p(dy), _p(rec), _p(dx), n, h, w, c, int(relu_input), _stream()), 'maxpool2x2_bwd_idx')
    return dx


def max_pool2x2_bwd_raw(dy, x, relu_input):
    dy, x = nhwc(dy), nhwc(x)
    n, c, h, w = x.shape
    dx = torch.empty_like(x, memory_format=CL)
    _hip.check(_hip.lib().srhip_maxpool2x2_bwd(_p(dy), _p(x), _p(dx), n, h, w, c, int(relu_input), _stream()),
               'maxpool2x2_bwd')
    return dx


class _MaxPool2x2(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return max_pool2x2_raw(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return max_pool2x2_bwd_raw(dy, x, False)


def max_pool2x2(x):
    if x.shape[1] % 4 == 0 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0:
        return _MaxPool2x2.apply(x)
    raise NotImplementedError('max_pool2x2: the HIP kernel takes C %% 4 == 0 and even H, W (VGG on 216 x 216 tiles); got %s -- '
                              'there is no ATen fallback' % (tuple(x.shape),))


class _VggFeatures(Function):
    """vgg19.features[:12] with frozen weights (sradsgan.py:88-99, 836-838) as ONE autograd node whose
    backward is the data-gradient chain only: every ReLU backward rides in the epilogue of the dgrad
    (or in the max-pool backward) that produces its input gradient -- no separate mask passes."""

    @staticmethod
    def forward(ctx, x, *wb):
        ws, bs = wb[0::2], wb[1::2]
        x = nhwc(x)
        y1 = conv2d_fwd_raw(x, ws[0], bs[0], 1, 1, 0.0)
        y2 = conv2d_fwd_raw(y1, ws[1], bs[1], 1, 1, 0.0)
        idx = _POOL_IDX and ctx.needs_input_grad[0]      # a backward will follow: the pools leave 2-byte records instead of keeping y2 / y4
        p1, r1 = max_pool2x2_idx_raw(y2) if idx else (max_pool2x2_raw(y2), None)
        y3 = conv2d_fwd_raw(p1, ws[2], bs[2], 1, 1, 0.0)
        y4 = conv2d_fwd_raw(y3, ws[3], bs[3], 1, 1, 0.0)
        p2, r2 = max_pool2x2_idx_raw(y4) if idx else (max_pool2x2_raw(y4), None)
        y5 = conv2d_fwd_raw(p2, ws[4], bs[4], 1, 1, 0.0)
        if idx:
            ctx.shapes = (tuple(y2.shape), tuple(y4.shape))
            ctx.save_for_backward(y1, r1, p1, y3, r2, p2, y5, *ws)
        else:
            ctx.shapes = None
            ctx.save_for_backward(y1, y2, p1, y3, y4, p2, y5, *ws)
        ctx.x_shape = tuple(x.shape)
        return y5

    @staticmethod
    def backward(ctx, g):
        y1, y2, p1, y3, y4, p2, y5, w1, w2, w3, w4, w5 = ctx.saved_tensors
        g = lrelu_bwd_raw(g, y5, 0.0)                                            # ReLU after conv3_1 (54x54, small)
        g = conv2d_dgrad_raw(g, w5, tuple(p2.shape), 1, 1)
        g = max_pool2x2_bwd_idx_raw(g, y4, ctx.shapes[1], True) if ctx.shapes else max_pool2x2_bwd_raw(g, y4, True)   # pool2 + ReLU(conv2_2) (y4 = its records)
        g = conv2d_dgrad_raw(g, w4, tuple(y3.shape), 1, 1, None, y3, 0.0)         # + ReLU(conv2_1)
        g = conv2d_dgrad_raw(g, w3, tuple(p1.shape), 1, 1)
        g = max_pool2x2_bwd_idx_raw(g, y2, ctx.shapes[0], True) if ctx.shapes else max_pool2x2_bwd_raw(g, y2, True)   # pool1 + ReLU(conv1_2) (y2 = its records)
        g = conv2d_dgrad_raw(g, w2, tuple(y1.shape), 1, 1, None, y1, 0.0)         # + ReLU(conv1_1)
        g = conv2d_dgrad_raw(g, w1, ctx.x_shape, 1, 1)
        return (g,) + (None,) * 10


def vgg_features(x, weights_and_biases):
    return _VggFeatures.apply(x, *weights_and_biases)


class _L1Mean(Function):
    @staticmethod
    def forward(ctx, a, b):
        _require_gpu(a, 'l1_mean')
        a, b = _dense16(a), _dense16(b)
        if a.shape != b.shape:
            raise ValueError('l1_mean: shapes differ: %s vs %s' % (tuple(a.shape), tuple(b.shape)))
        lib = _hip.lib()
        out = torch.empty((), device=a.device, dtype=torch.float32)
        ws = _ws(lib.srhip_reduce_workspace(), a)
        _hip.check(lib.srhip_l1_mean_fwd(_p(a), _p(b), _p(out), _p(ws), ws.numel() * 4, a.numel(), _stream()), 'l1_mean_fwd')
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad
        da = torch.empty_like(a, memory_format=CL) if a.dim() == 4 else torch.empty_like(a)
        db = (torch.empty_like(a, memory_format=CL) if a.dim() == 4 else torch.empty_like(a)) if need_b else None
        _hip.check(_hip.lib().srhip_l1_mean_bwd(_p(a), _p(b), _p(gout.contiguous()), _p(da), _p(db), a.numel(), _stream()),
                   'l1_mean_bwd')
        return (da if need_a else None), db


def l1_mean(a, b):
    """nn.L1Loss() (sradsgan.py:686,834,838)."""
    return _L1Mean.apply(a, b)


class _Mean(Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, 'mean')
        xc = x.contiguous()
        lib = _hip.lib()
        out = torch.empty((), device=x.device, dtype=torch.float32)
        ws = _ws(lib.srhip_reduce_workspace(), x)
        _hip.check(lib.srhip_mean_fwd(_p(xc), _p(out), _p(ws), ws.numel() * 4, xc.numel(), _stream()), 'mean_fwd')
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, gout):
        dx = torch.empty(ctx.shape, device=gout.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_mean_bwd(_p(gout.contiguous()), _p(dx), dx.numel(), _stream()), 'mean_bwd')
        return dx


def mean(x):
    """The critic means of GANLoss('wgan-gp') (sradsgan.py:61-66)."""
    return _Mean.apply(x)


class _GpPenalty(Function):
    @staticmethod
    def forward(ctx, grads):
        _require_gpu(grads, 'gp_penalty')
        g = nhwc(grads)
        n, c, h, w = g.shape
        lib = _hip.lib()
        out = torch.empty((), device=g.device, dtype=torch.float32)
        ws = _ws(lib.srhip_reduce_workspace(), g)
        _hip.check(lib.srhip_gp_norm_penalty_fwd(_p(g), _p(out), _p(ws), ws.numel() * 4, n * h * w, c, _stream()),
                   'gp_norm_penalty_fwd')
        ctx.save_for_backward(g)
        return out

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        n, c, h, w = g.shape
        dg = torch.empty_like(g, memory_format=CL)
        _hip.check(_hip.lib().srhip_gp_norm_penalty_bwd(_p(g), _p(gout.contiguous()), _p(dg), n * h * w, c, _stream()),
                   'gp_norm_penalty_bwd')
        return dg


GP_NORMS = {'L2': 0, 'L1': 1, 'Linf': 2}         # SRHIP_GP_NORM_* (--grad_penalty_Lp_norm)
GP_PENALTIES = {'LS': 0, 'hinge': 1}             # SRHIP_GP_PENALTY_* (--penalty_type)


class _GpPenaltyKinds(Function):
    """srhip_gp_penalty_{fwd,bwd}: any (norm, penalty) pair; the kinds travel by value (nothing synchronises with the host)."""

    @staticmethod
    def forward(ctx, grads, norm_kind, penalty_kind):
        _require_gpu(grads, 'gp_penalty')
        g = nhwc(grads)
        n, c, h, w = g.shape
        lib = _hip.lib()
        out = torch.empty((), device=g.device, dtype=torch.float32)
        ws = _ws(lib.srhip_reduce_workspace(), g)
        _hip.check(lib.srhip_gp_penalty_fwd(_p(g), _p(out), _p(ws), ws.numel() * 4, n * h * w, c, norm_kind, penalty_kind, _stream()),
                   'gp_penalty_fwd')
        ctx.save_for_backward(g)
        ctx.kinds = (norm_kind, penalty_kind)
        return out

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        n, c, h, w = g.shape
        dg = torch.empty_like(g, memory_format=CL)
        _hip.check(_hip.lib().srhip_gp_penalty_bwd(_p(g), _p(gout.contiguous()), _p(dg), n * h * w, c, ctx.kinds[0], ctx.kinds[1],
                                                   _stream()), 'gp_penalty_bwd')
        return dg, None, None


def gp_penalty(grads, norm='L2', penalty='LS'):
    """sradsgan.py:624-637: `norm` ('L2' | 'L1' | 'Linf') over the channel dim (per pixel), `penalty` ('LS': (norm - 1)^2 | 'hinge':
    relu(norm - 1)), mean.  The defaults take srhip_gp_norm_penalty_*, every other pair srhip_gp_penalty_*."""
    if norm not in GP_NORMS or penalty not in GP_PENALTIES:
        raise ValueError('gp_penalty: norm must be one of %s and penalty one of %s, got %r / %r'
                         % (sorted(GP_NORMS), sorted(GP_PENALTIES), norm, penalty))
    if norm == 'L2' and penalty == 'LS':
        return _GpPenalty.apply(grads)
    return _GpPenaltyKinds.apply(grads, GP_NORMS[norm], GP_PENALTIES[penalty])


class _MseMean(Function):
    @staticmethod
    def forward(ctx, a, b):
        _require_gpu(a, 'mse_mean')
        a, b = _dense16(a), _dense16(b)
        if a.shape != b.shape:
            raise ValueError('mse_mean: shapes differ: %s vs %s' % (tuple(a.shape), tuple(b.shape)))
        lib = _hip.lib()
        out = torch.empty((), device=a.device, dtype=torch.float32)
        ws = _ws(lib.srhip_reduce_workspace(), a)
        _hip.check(lib.srhip_mse_mean_fwd(_p(a), _p(b), _p(out), _p(ws), ws.numel() * 4, a.numel(), _stream()), 'mse_mean_fwd')
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad
        da = torch.empty_like(a, memory_format=CL) if a.dim() == 4 else torch.empty_like(a)
        db = (torch.empty_like(a, memory_format=CL) if a.dim() == 4 else torch.empty_like(a)) if need_b else None
        _hip.check(_hip.lib().srhip_mse_mean_bwd(_p(a), _p(b), _p(gout.contiguous()), _p(da), _p(db), a.numel(), _stream()),
                   'mse_mean_bwd')
        return (da if need_a else None), db


def mse_mean(a, b):
    """nn.MSELoss() (DSSR's loss_Lp_norm='L2', model/dssr.py:266-269)."""
    return _MseMean.apply(a, b)


# --------------------------------------------------------------------------------------------- #
# DSSR (model/dssr.py:69-177): average-pool channel attention + residual, and the upsampler fold
# --------------------------------------------------------------------------------------------- #


class _ConvPool(Function):
    """y = conv3x3(x, w) + b (stride 1, pad 1, 64 output channels) that also leaves the channel pooling partials of y behind
    (srhip_conv2d_fwd_pool).  Returns (y, pool buffer, segments per image); only y is differentiable."""

    @staticmethod
    def forward(ctx, x, w, b):
        y, (pool, sec, nseg) = conv2d_fwd_pool_raw(x, w, b)
        ctx.save_for_backward(x, w, b)
        ctx.mark_non_differentiable(pool)
        return y, pool, nseg

    @staticmethod
    def backward(ctx, dy, _dpool, _dnseg):
        x, w, b = ctx.saved_tensors
        skip = _skip_param_grads(w)
        dx = _ConvDgrad.apply(dy, w, tuple(x.shape), 1, 1) if ctx.needs_input_grad[0] else None
        dw = db = None
        want_b = b is not None and ctx.needs_input_grad[2] and not skip
        if ctx.needs_input_grad[1] and not skip and _state.wgrads is not None and not torch.is_grad_enabled():
            dw, db = wgrad_for_params(w, b, x, dy, 1, 1, want_b)
        elif ctx.needs_input_grad[1] and not skip:
            dw, db = _ConvWgrad.apply(x, dy, tuple(w.shape), 1, 1, want_b)
        elif want_b:
            db = _ColSum.apply(dy)
        return dx, dw, db


def conv2d_pool(x, weight, bias=None):
    """conv2d(x, weight, bias, 1, 1) plus the channel sums of its output as (pool buffer, segments per image) when the conv's
    epilogue can produce them (pool_epilogue_ok), else (y, None)."""
    if pool_epilogue_ok(x, weight):
        y, pool, nseg = _ConvPool.apply(x, weight, bias)
        return y, (pool, nseg)
    return conv2d(x, weight, bias, 1, 1), None


class _CaResidual(Function):
    """out = sigmoid(fc2 relu(fc1 mean_hw u + b1) + b2) * u + x: dssr.py:69-82 (CA with the average pool only, no biases) and the
    `out += x` of WAB (:103); with the biases, RCAN's CALayer and the `res += x` of its RCAB (drcan.py:94-135).  Three launches
    forward (pooling pass unless the conv that produced u left its sums, MLP, scale + add), four backward (g * u partials, per-image
    MLP backward, MLP weight and bias gradients, du); deterministic.  Without biases the bias-free entry points run, unchanged."""

    @staticmethod
    def forward(ctx, u, x, fc1_w, fc2_w, pool=None, fc1_b=None, fc2_b=None):
        _require_gpu(u, 'ca_residual')
        u, x = nhwc(u), nhwc(x)
        n, c, h, w = u.shape
        if c != 64 or x.shape != u.shape:
            raise ValueError('ca_residual: u and x must be [n, 64, h, w] of one shape, got %s / %s' % (tuple(u.shape), tuple(x.shape)))
        lib = _hip.lib()
        f32 = dict(device=u.device, dtype=torch.float32)
        hid = fc1_w.shape[0]
        biased = fc1_b is not None or fc2_b is not None
        if biased and ((fc1_b is not None and fc1_b.numel() != hid) or (fc2_b is not None and fc2_b.numel() != c)):
            raise ValueError('ca_residual: fc1_b must have %d and fc2_b %d elements' % (hid, c))
        if pool is None:
            nseg = lib.srhip_ca_segments()
            psum = torch.empty(n * nseg * c, **f32)
            _hip.check(lib.srhip_ca_pool_sum(_p(u), _p(psum), n, h * w, c, _stream()), 'ca_pool_sum')
        else:
            psum, nseg = pool                        # the sum section leads the conv epilogue's [sum | max | arg] buffer
        avg, s, hidden = torch.empty(n, c, **f32), torch.empty(n, c, **f32), torch.empty(n, hid, **f32)
        fc1c, fc2c = fc1_w.detach().contiguous(), fc2_w.detach().contiguous()
        if biased:
            b1c = fc1_b.detach().contiguous() if fc1_b is not None else None
            b2c = fc2_b.detach().contiguous() if fc2_b is not None else None
            _hip.check(lib.srhip_ca_mlp_fwd_bias(_p(psum), nseg, _p(fc1c), _p(b1c), _p(fc2c),
                                                 _p(b2c), _p(avg), _p(hidden), _p(s), n, h * w, c, hid,
                                                 _stream()), 'ca_mlp_fwd_bias')
        else:
            _hip.check(lib.srhip_ca_mlp_fwd(_p(psum), nseg, _p(fc1c), _p(fc2c), _p(avg), _p(hidden), _p(s), n, h * w, c, hid,
                                            _stream()), 'ca_mlp_fwd')
        out = torch.empty_like(u, memory_format=CL)
        _hip.check(lib.srhip_ca_scale_res(_p(u), _p(s), _p(x), _p(out), n, h * w, c, _stream()), 'ca_scale_res')
        ctx.save_for_backward(u, fc1c, fc2c, avg, hidden, s)
        ctx.biased = (fc1_b is not None, fc2_b is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        u, fc1c, fc2c, avg, hidden, s = ctx.saved_tensors
        g = nhwc(g)
        n, c, h, w = u.shape
        lib = _hip.lib()
        f32 = dict(device=u.device, dtype=torch.float32)
        part = torch.empty(n * lib.srhip_ca_segments() * c, **f32)
        _hip.check(lib.srhip_ca_bwd_partial(_p(g), _p(u), _p(part), n, h * w, c, _stream()), 'ca_bwd_partial')
        dmean = torch.empty(n, c, **f32)
        dfc1, dfc2 = torch.empty(fc1c.shape, **f32), torch.empty(fc2c.shape, **f32)
        ws = _ws(lib.srhip_ca_mlp_bwd_workspace(n, fc1c.shape[0]), u)
        need = ctx.needs_input_grad
        has1, has2 = ctx.biased
        db1 = torch.empty(fc1c.shape[0], **f32) if has1 and need[5] else None
        db2 = torch.empty(c, **f32) if has2 and need[6] else None
        if has1 or has2:
            _hip.check(lib.srhip_ca_mlp_bwd_bias(_p(part), _p(avg), _p(hidden), _p(s), _p(fc1c), _p(fc2c), _p(dmean), _p(dfc1),
                                                 _p(db1), _p(dfc2), _p(db2),
                                                 _p(ws), ws.numel() * 4, n, h * w, c, fc1c.shape[0], _stream()), 'ca_mlp_bwd_bias')
        else:
            _hip.check(lib.srhip_ca_mlp_bwd(_p(part), _p(avg), _p(hidden), _p(s), _p(fc1c), _p(fc2c), _p(dmean), _p(dfc1), _p(dfc2),
                                            _p(ws), ws.numel() * 4, n, h * w, c, fc1c.shape[0], _stream()), 'ca_mlp_bwd')
        du = torch.empty_like(u, memory_format=CL)
        _hip.check(lib.srhip_ca_bwd_du(_p(g), _p(s), _p(dmean), _p(du), n, h * w, c, _stream()), 'ca_bwd_du')
        return (du if need[0] else None, _passed_through(g) if need[1] else None, dfc1 if need[2] else None,
                dfc2 if need[3] else None, None, db1, db2)


def ca_residual(u, x, fc1_w, fc2_w, pool=None, fc1_b=None, fc2_b=None):
    """sigmoid(fc2(relu(fc1(avgpool u) + fc1_b)) + fc2_b) * u + x (dssr.py:69-82, 103; with the biases drcan.py:94-135) for 64-channel
    u.  pool: (buffer, segments per image) from conv2d_pool, whose leading section holds the channel sums of u; None runs a pooling
    pass.  fc1_b [hidden] / fc2_b [64]: the 1x1 convs' biases, optional; without them the arithmetic is DSSR's, bit for bit."""
    return _CaResidual.apply(u, x, fc1_w, fc2_w, pool, fc1_b, fc2_b)


class _AddBcastScaled(Function):
    """out = a + scale * b, b of batch 1 broadcast over a's batch: UP(S) + G * UP(0) of the DSSR upsampler fold."""

    @staticmethod
    def forward(ctx, a, b, scale):
        _require_gpu(a, 'add_bcast_scaled')
        a, b = nhwc(a), nhwc(b)
        if b.shape[0] != 1 or b.shape[1:] != a.shape[1:]:
            raise ValueError('add_bcast_scaled: b must have the shape of a with batch 1, got %s / %s' % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty_like(a, memory_format=CL)
        _hip.check(_hip.lib().srhip_add_bcast_scaled(_p(a), _p(b), float(scale), _p(out), a.shape[0], b.numel(), _stream()),
                   'add_bcast_scaled')
        ctx.scale, ctx.n = float(scale), a.shape[0]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = nhwc(g)
        db = None
        if ctx.needs_input_grad[1]:
            db = empty_nhwc(1, *g.shape[1:], like=g)
            _hip.check(_hip.lib().srhip_batch_sum_scaled(_p(g), ctx.scale, _p(db), ctx.n, db.numel(), _stream()), 'batch_sum_scaled')
        return g, db, None


def add_bcast_scaled(a, b, scale):
    """a + scale * b with b [1, C, H, W] broadcast over a's batch (NHWC, C*H*W % 4 == 0)."""
    return _AddBcastScaled.apply(a, b, scale)


# --------------------------------------------------------------------------------------------- #
# NDSRGAN (model/ndsrgan.py:57-211): concat-free dense blocks, scaled residuals with running trunk sums, nearest upsampling,
# SmoothL1
# --------------------------------------------------------------------------------------------- #


DENSE_NF, DENSE_NC, DENSE_W = 64, 32, 192          # block channels, growth per CL, width of a dense-block buffer (64 + 4 * 32)
RES_SCALE = 0.2                                    # `x * 0.2` of the residuals and running sums
LRELU_SLOPE = 0.2                                  # nn.LeakyReLU(0.2) of the CLs


def _rowld(t):
    """(t, row stride) for a logical NCHW tensor whose memory is NHWC pixel rows of stride ld >= C (a channel slice of a wider NHWC
    buffer, or dense channels-last); anything else is made dense channels-last first."""
    n, c, h, w = t.shape
    st = t.stride()
    ld = st[3]
    if (st[1] == 1 and ld >= c and ld % 4 == 0 and st[2] == w * ld and (n == 1 or st[0] == h * w * ld)
            and t.data_ptr() % 16 == 0):
        return t, ld
    return nhwc(t), c


def _dense_buffer(n, h, w, like):
    return empty_nhwc(n, DENSE_W, h, w, like)


def conv2d_fwd_ld(x, ldx, w, b, y, ldy, n, h, wd, slope=None):
    """stride-1 'same' conv reading cin channels of rows of stride ldx and writing cout channels into rows of stride ldy (bias,
    optional fused LeakyReLU): a CL of a dense block reads a channel prefix of its buffer and writes its own slice of it."""
    cout, cin, kh, kw = w.shape
    flags = (EPI_BIAS if b is not None else 0) | (EPI_LRELU if slope is not None else 0)
    bias = b.detach().contiguous() if b is not None else None
    _hip.check(_hip.lib().srhip_conv2d_fwd(_p(x), _p(packed_weight(w, 0)), _p(bias), None, None, None, _p(y), n, h, wd, cin, cout, kh,
                                           kw, 1, kh // 2, ldx, ldy, 0, float(slope or 0.0), flags, _stream()), 'conv2d_fwd (strided)')


def conv2d_dgrad_ld(dy, ldy, w, dx, ldx, n, h, wd, accumulate):
    """dx (rows of stride ldx, cin channels) = / += conv_transpose(dy, w) for a stride-1 'same' conv, dy rows of stride ldy."""
    cout, cin, kh, kw = w.shape
    _hip.check(_hip.lib().srhip_conv2d_dgrad(_p(dy), _p(packed_weight(w, 1)), _p(dx), None, None, 0.0, n, h, wd, cin, cout, kh, kw, 1,
                                             kh // 2, ldy, ldx, cin, int(accumulate), _stream()), 'conv2d_dgrad (strided)')


def conv2d_wgrad_ld(x, ldx, dy, ldy, w_shape, n, h, wd, with_bias=True):
    """(dw, db) of a stride-1 'same' conv from x (cin channels of rows of stride ldx) and dy (rows of stride ldy)."""
    cout, cin, kh, kw = w_shape
    lib = _hip.lib()
    nbytes = lib.srhip_conv2d_wgrad_workspace(n, h, wd, cin, cout, kh, kw, 1, kh // 2)
    ws = torch.empty((max(nbytes, 4) + 3) // 4, device=x.device, dtype=torch.float32)
    dw = torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if with_bias else None
    _hip.check(lib.srhip_conv2d_wgrad(_p(x), _p(dy), _p(dw), _p(db), None, None, 0, _p(ws), ws.numel() * 4, n, h, wd, cin, cout, kh, kw,
                                      1, kh // 2, ldx, ldy, _stream()), 'conv2d_wgrad (strided)')
    return dw, db


def scaled_res_raw(r, ldr, c, ldc, s, lds, alpha, beta, y, ldy, z, ldz, rows, ch=DENSE_NF):
    """y = r + alpha * c, z = s + beta * y on raw rows (srhip_scaled_res_fwd); any of c, y, z may be None (see the header)."""
    _hip.check(_hip.lib().srhip_scaled_res_fwd(_p(r), ldr, _p(c), ldc, _p(s), lds, float(alpha), float(beta), _p(y), ldy, _p(z), ldz,
                                               rows, ch, _stream()), 'scaled_res_fwd')


def scaled_res_bwd_raw(dz, ldz, e, lde, ka, kb, kc, dc, ldc, dr, ldr, width, rows, ch=DENSE_NF):
    """dc = ka dz; dr[0:ch] = kb dz + kc e, dr[ch:width] = 0 (srhip_scaled_res_bwd)."""
    _hip.check(_hip.lib().srhip_scaled_res_bwd(_p(dz), ldz, _p(e), lde, float(ka), float(kb), float(kc), _p(dc), ldc, _p(dr), ldr,
                                               width, rows, ch, _stream()), 'scaled_res_bwd')


def lrelu_bwd_strided_raw(dy, ldg, y, ldy, dx, ldx, slope, rows, ch):
    _hip.check(_hip.lib().srhip_lrelu_bwd_strided(_p(dy), ldg, _p(y), ldy, _p(dx), ldx, float(slope), rows, ch, _stream()),
               'lrelu_bwd_strided')


def _dense_fwd(buf, wb, n, h, w, slope):
    """The four CLs of a dense block inside its buffer (channels 0:64 hold the block input), then conv5 over all 192 channels.
    Returns conv5's output (dense, bias included)."""
    for j in range(4):
        off = DENSE_NF + DENSE_NC * j
        conv2d_fwd_ld(buf, DENSE_W, wb[2 * j], wb[2 * j + 1], buf[:, off:], DENSE_W, n, h, w, slope)
    c5 = empty_nhwc(n, DENSE_NF, h, w, buf)
    conv2d_fwd_ld(buf, DENSE_W, wb[8], wb[9], c5, DENSE_NF, n, h, w)
    return c5


def _dense_bwd(buf, wb, dz, ldz, e, lde, ka, kb, kc, n, h, w, slope, grads):
    """Backward of one dense block whose result is r + alpha conv5(buf) (or a running sum of it): dz the gradient at the result, ka /
    kb the factors it reaches conv5 / the block input with, e (optional) one more gradient of the block input added with factor kc.
    Appends the 10 parameter gradients (CL weights / biases in order, conv5's last) to `grads`; returns the gradient buffer, whose
    channels 0:64 are the block input's gradient."""
    rows = n * h * w
    dbuf = _dense_buffer(n, h, w, buf)
    dc5 = empty_nhwc(n, DENSE_NF, h, w, buf)
    scaled_res_bwd_raw(dz, ldz, e, lde, ka, kb, kc, dc5, DENSE_NF, dbuf, DENSE_W, DENSE_W, rows)
    g = [None] * 10
    g[8], g[9] = conv2d_wgrad_ld(buf, DENSE_W, dc5, DENSE_NF, tuple(wb[8].shape), n, h, w)
    conv2d_dgrad_ld(dc5, DENSE_NF, wb[8], dbuf, DENSE_W, n, h, w, accumulate=True)
    for j in range(3, -1, -1):
        off = DENSE_NF + DENSE_NC * j
        gs = dbuf[:, off:]
        # every consumer of CL j's output (later CLs, conv5) has added its share: apply the LeakyReLU backward in place
        lrelu_bwd_strided_raw(gs, DENSE_W, buf[:, off:], DENSE_W, gs, DENSE_W, slope, rows, DENSE_NC)
        g[2 * j], g[2 * j + 1] = conv2d_wgrad_ld(buf, DENSE_W, gs, DENSE_W, tuple(wb[2 * j].shape), n, h, w)
        conv2d_dgrad_ld(gs, DENSE_W, wb[2 * j], dbuf, DENSE_W, n, h, w, accumulate=True)
    grads.extend(g)
    return dbuf


class _DenseStats:
    fills = 0              # block inputs copied into a new dense buffer by _adopt_or_fill (the generator's forward makes none)


dense_stats = _DenseStats()


def _adopt_or_fill(x, ldx, n, h, w):
    """The dense buffer whose channels 0:64 hold x: x's own buffer when the op that produced x wrote it there (its `_srhip_dense_buf`
    tag), else a new buffer that x is copied into (one pass, counted in dense_stats.fills)."""
    buf = getattr(x, '_srhip_dense_buf', None)
    if buf is not None and ldx == DENSE_W and buf.data_ptr() == x.data_ptr() and buf.shape[0] == n and tuple(buf.shape[2:]) == (h, w):
        return buf
    dense_stats.fills += 1
    buf = _dense_buffer(n, h, w, x)
    scaled_res_raw(x, ldx, None, 0, None, 0, 0.0, 0.0, buf, DENSE_W, None, 0, n * h * w)
    return buf


def _result_tensor(x, chain):
    """output of a block: channels 0:64 of the NEXT block's dense buffer (chain), tagged so that block adopts the buffer; or dense."""
    n, _, h, w = x.shape
    if not chain:
        return empty_nhwc(n, DENSE_NF, h, w, x), DENSE_NF
    nxt = _dense_buffer(n, h, w, x)
    out = nxt[:, :DENSE_NF]
    out._srhip_dense_buf = nxt
    return out, DENSE_W


class _DenseBlock(Function):
    """DenseBlock (ndsrgan.py:60-76) on its own: x + 0.2 * conv5(cat(x, CL1, ..., CL4)), the concatenation never formed."""

    @staticmethod
    def forward(ctx, x, *wb):
        _require_gpu(x, 'dense_block')
        x, ldx = _rowld(x)
        n, _, h, w = x.shape
        buf = _adopt_or_fill(x, ldx, n, h, w)
        c5 = _dense_fwd(buf, wb, n, h, w, LRELU_SLOPE)
        y = empty_nhwc(n, DENSE_NF, h, w, x)
        scaled_res_raw(buf, DENSE_W, c5, DENSE_NF, None, 0, RES_SCALE, 0.0, y, DENSE_NF, None, 0, n * h * w)
        ctx.save_for_backward(buf, *wb)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        buf, *wb = ctx.saved_tensors
        dy, ld = _rowld(dy)
        n, _, h, w = dy.shape
        grads = []
        dbuf = _dense_bwd(buf, wb, dy, ld, None, 0, RES_SCALE, 1.0, 0.0, n, h, w, LRELU_SLOPE, grads)
        return (dbuf[:, :DENSE_NF],) + tuple(grads)


def dense_block(x, weights_and_biases):
    """ndsrgan.py:60-76 for nf = 64, nc = 32: weights_and_biases = [w1, b1, ..., w4, b4, w5, b5] (CLs, then the 192 -> 64 conv)."""
    return _DenseBlock.apply(x, *weights_and_biases)


class _DcrdbStep(Function):
    """One step of DRRDBnet (ndsrgan.py:94-158): S = x + 0.2 * DCRDB(x) with DCRDB (:78-92) = three dense blocks on running sums
    t1 = x + .2 o1, t2 = t1 + .2 o2, t3 = t2 + .2 o3 (the reference's left-to-right sums, same fp32 operations), o4 = conv(t3),
    DCRDB(x) = o4 * .2 + x.  Each t_i lands in channels 0:64 of the next dense block's buffer, and S in the next step's when
    `chain`.  Backward: per dense block one srhip_scaled_res_bwd pass (conv5's gradient and the buffer's initial gradient), conv5's
    wgrad and accumulating dgrad, then per CL (last first) the strided LeakyReLU backward in place, wgrad and accumulating dgrad
    into the buffer's channel prefix."""

    @staticmethod
    def forward(ctx, x, chain, *params):
        _require_gpu(x, 'dcrdb')
        x, ldx = _rowld(x)
        n, _, h, w = x.shape
        rows = n * h * w
        a = b = RES_SCALE
        bufs = [_adopt_or_fill(x, ldx, n, h, w)]
        t3 = None
        for k in range(3):
            buf = bufs[k]
            c5 = _dense_fwd(buf, params[10 * k:10 * k + 10], n, h, w, LRELU_SLOPE)
            if k < 2:
                nxt = _dense_buffer(n, h, w, x)
                scaled_res_raw(buf, DENSE_W, c5, DENSE_NF, buf, DENSE_W, a, b, None, 0, nxt, DENSE_W, rows)
                bufs.append(nxt)
            else:
                t3 = empty_nhwc(n, DENSE_NF, h, w, x)
                scaled_res_raw(buf, DENSE_W, c5, DENSE_NF, buf, DENSE_W, a, b, None, 0, t3, DENSE_NF, rows)
        c4 = empty_nhwc(n, DENSE_NF, h, w, x)
        conv2d_fwd_ld(t3, DENSE_NF, params[30], params[31], c4, DENSE_NF, n, h, w)
        out, ldo = _result_tensor(x, chain)
        scaled_res_raw(x, ldx, c4, DENSE_NF, x, ldx, a, b, None, 0, out, ldo, rows)
        ctx.save_for_backward(t3, *bufs, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dS):
        t3, b1, b2, b3, *params = ctx.saved_tensors
        dS, lds = _rowld(dS)
        n, _, h, w = dS.shape
        a = b = RES_SCALE
        ka, kb = a * b, 1.0 + b
        dc4 = empty_nhwc(n, DENSE_NF, h, w, dS)
        scaled_res_bwd_raw(dS, lds, None, 0, ka, 0.0, 0.0, dc4, DENSE_NF, None, 0, DENSE_NF, n * h * w)
        gw4, gb4 = conv2d_wgrad_ld(t3, DENSE_NF, dc4, DENSE_NF, tuple(params[30].shape), n, h, w)
        dz = empty_nhwc(n, DENSE_NF, h, w, dS)
        conv2d_dgrad_ld(dc4, DENSE_NF, params[30], dz, DENSE_NF, n, h, w, accumulate=False)
        ldz = DENSE_NF
        per_block = [None, None, None]
        for k, buf in ((2, b3), (1, b2), (0, b1)):
            grads = []
            # the step's input x reaches S directly and through DCRDB's own residual: (1 + .2) dS, folded into block 1's pass
            e, lde = (dS, lds) if k == 0 else (None, 0)
            dbuf = _dense_bwd(buf, params[10 * k:10 * k + 10], dz, ldz, e, lde, ka, kb, kb, n, h, w, LRELU_SLOPE, grads)
            per_block[k] = grads
            dz, ldz = dbuf[:, :DENSE_NF], DENSE_W
        return (dz, None) + tuple(per_block[0] + per_block[1] + per_block[2]) + (gw4, gb4)


def dcrdb_step(x, params, chain=False):
    """x + 0.2 * DCRDB(x) (one term of ndsrgan.py:121-158's running sum).  params: the 32 DCRDB tensors in state_dict order
    (RDB1..3 each [CL weights / biases, conv5 weight, bias], then conv).  chain: the result is written into the next step's dense
    buffer (the caller feeds it to another dcrdb_step)."""
    return _DcrdbStep.apply(x, bool(chain), *params)


class _ConvIntoDense(Function):
    """conv 3x3 + bias (stride 1, 'same', 64 output channels) written into channels 0:64 of a new dense-block buffer: the generator's
    conv1 (ndsrgan.py:164-167), whose output is the first DCRDB's input.  Returns that channel slice, tagged for adoption."""

    @staticmethod
    def forward(ctx, x, w, b):
        _require_gpu(x, 'conv2d_into_dense')
        if w.shape[0] != DENSE_NF or tuple(w.shape[2:]) != (3, 3):
            raise ValueError('conv2d_into_dense: a 3x3 conv to 64 channels, got weight %s' % (tuple(w.shape),))
        x, ldx = _rowld(x)
        n, _, h, wd = x.shape
        out, ldo = _result_tensor(x, True)
        conv2d_fwd_ld(x, ldx, w, b, out, ldo, n, h, wd)
        ctx.save_for_backward(x, w, b)
        ctx.ldx = ldx
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dy, ldy = _rowld(dy)
        n, cin, h, wd = x.shape
        dx = None
        if ctx.needs_input_grad[0]:
            dx = empty_nhwc(n, cin, h, wd, dy)
            conv2d_dgrad_ld(dy, ldy, w, dx, cin, n, h, wd, accumulate=False)
        dw, db = conv2d_wgrad_ld(x, ctx.ldx, dy, ldy, tuple(w.shape), n, h, wd, with_bias=b is not None)
        return dx, dw, db


def conv2d_into_dense(x, weight, bias):
    return _ConvIntoDense.apply(x, weight, bias)


class _ConvResidualStrided(Function):
    """conv 3x3 (x) + bias + r, r read through its own row stride: the generator's `out + conv2(trunk)` (ndsrgan.py:203) with `out`
    the channel slice of the first dense buffer that conv1 wrote (no copy of it).  Output dense."""

    @staticmethod
    def forward(ctx, x, w, b, r):
        _require_gpu(x, 'conv2d_residual_strided')
        x, ldx = _rowld(x)
        r, ldr = _rowld(r)
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        y = empty_nhwc(n, cout, h, wd, x)
        bias = b.detach().contiguous()
        _hip.check(_hip.lib().srhip_conv2d_fwd(_p(x), _p(packed_weight(w, 0)), _p(bias), _p(r), None, None, _p(y), n, h, wd, cin, cout,
                                               3, 3, 1, 1, ldx, cout, ldr, 0.0, EPI_BIAS | EPI_RESIDUAL, _stream()),
                   'conv2d_fwd (strided residual)')
        ctx.save_for_backward(x, w, b)
        ctx.ldx = ldx
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dy = nhwc(dy)
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = empty_nhwc(n, cin, h, wd, dy)
            conv2d_dgrad_ld(dy, cout, w, dx, cin, n, h, wd, accumulate=False)
        dw, db = conv2d_wgrad_ld(x, ctx.ldx, dy, cout, tuple(w.shape), n, h, wd)
        return dx, dw, db, dy


def conv2d_residual_strided(x, weight, bias, residual):
    return _ConvResidualStrided.apply(x, weight, bias, residual)


class _UpsampleNearest(Function):
    """nn.UpsamplingNearest2d(scale_factor = r), r in {2, 3} (ndsrgan.py:175-181), NHWC."""

    @staticmethod
    def forward(ctx, x, r):
        _require_gpu(x, 'upsample_nearest')
        x = nhwc(x)
        n, c, h, w = x.shape
        y = empty_nhwc(n, c, h * r, w * r, x)
        _hip.check(_hip.lib().srhip_upsample_nearest_fwd(_p(x), _p(y), n, h, w, c, r, _stream()), 'upsample_nearest_fwd')
        ctx.r, ctx.shape = r, (n, c, h, w)
        return y

    @staticmethod
    def backward(ctx, g):
        return _UpsampleNearestBwd.apply(g, ctx.r, ctx.shape), None


class _UpsampleNearestBwd(Function):
    @staticmethod
    def forward(ctx, g, r, shape):
        g = nhwc(g)
        n, c, h, w = shape
        dx = empty_nhwc(n, c, h, w, g)
        _hip.check(_hip.lib().srhip_upsample_nearest_bwd(_p(g), _p(dx), n, h, w, c, r, _stream()), 'upsample_nearest_bwd')
        ctx.r = r
        return dx

    @staticmethod
    def backward(ctx, gg):
        return _UpsampleNearest.apply(gg, ctx.r), None, None


def upsample_nearest(x, r):
    return _UpsampleNearest.apply(x, int(r))


class _SmoothL1Mean(Function):
    @staticmethod
    def forward(ctx, a, b, target):
        _require_gpu(a, 'smooth_l1_mean')
        a = _dense16(a)
        if b is not None:
            b = _dense16(b)
            if a.shape != b.shape:
                raise ValueError('smooth_l1_mean: shapes differ: %s vs %s' % (tuple(a.shape), tuple(b.shape)))
        lib = _hip.lib()
        out = torch.empty((), device=a.device, dtype=torch.float32)
        ws = _ws(lib.srhip_reduce_workspace(), a)
        _hip.check(lib.srhip_smooth_l1_mean_fwd(_p(a), _p(b), float(target), _p(out), _p(ws), ws.numel() * 4, a.numel(), _stream()),
                   'smooth_l1_mean_fwd')
        ctx.save_for_backward(a, b)
        ctx.target = float(target)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        need_b = b is not None and ctx.needs_input_grad[1]
        like = (lambda: torch.empty_like(a, memory_format=CL)) if a.dim() == 4 else (lambda: torch.empty_like(a))
        da = like()
        db = like() if need_b else None
        _hip.check(_hip.lib().srhip_smooth_l1_mean_bwd(_p(a), _p(b), ctx.target, _p(gout.contiguous()), _p(da), _p(db), a.numel(),
                                                       _stream()), 'smooth_l1_mean_bwd')
        return (da if ctx.needs_input_grad[0] else None), db, None


def smooth_l1_mean(a, target):
    """nn.SmoothL1Loss() (beta = 1, mean) of a against a tensor or a scalar target (D's valid = 1 / fake = 0 patches: no ones
    tensor)."""
    if torch.is_tensor(target):
        return _SmoothL1Mean.apply(a, target, 0.0)
    return _SmoothL1Mean.apply(a, None, float(target))


# --------------------------------------------------------------------------------------------- #
# AMSSRN's new arithmetic (SRADSGAN/model/amssrn.py:167-217): dilated 3x3 convolutions (csrc/conv_dilated.hip) and PReLU with a
# device-resident slope (csrc/prelu.hip)
# --------------------------------------------------------------------------------------------- #


DIL_MAX = 3                                        # dilations 1..3 (ASPP's d1, d2, d3)


def _dil_check(w_shape, dilation):
    cout, cin, kh, kw = w_shape
    if (kh, kw) != (3, 3) or not 1 <= dilation <= DIL_MAX or cin % 4 or cout % 4:
        raise NotImplementedError('dilated conv: 3x3, dilation 1..%d, channels %% 4 == 0 (got %s, dilation %d)'
                                  % (DIL_MAX, tuple(w_shape), dilation))
    return cout, cin


def _dil_workspace(kind, n, h, wd, cin, cout, dilation, like):
    nbytes = _hip.lib().srhip_conv2d_dil_workspace(kind, n, h, wd, cin, cout, dilation)
    return torch.empty(max((nbytes + 3) // 4, 4), device=like.device, dtype=torch.float32)


def conv2d_dil_fwd_raw(x, ldx, w, b, y, ldy, n, h, wd, dilation, slope=None):
    """y (rows of stride ldy) = act(conv(x, w, dilation) + b) for a stride-1 3x3 conv with pad = dilation; x: rows of stride ldx."""
    _require_gpu(x, 'conv2d_fwd_dil')
    cout, cin = _dil_check(w.shape, dilation)
    flags = (EPI_BIAS if b is not None else 0) | (EPI_LRELU if slope is not None else 0)
    bias = b.detach().contiguous() if b is not None else None
    ws = _dil_workspace(1, n, h, wd, cin, cout, dilation, x)
    _hip.check(_hip.lib().srhip_conv2d_fwd_dil(_p(x), _p(packed_weight(w, 0)), _p(bias), None, _p(y), _p(ws), ws.numel() * 4, n, h, wd,
                                               cin, cout, dilation, ldx, ldy, float(slope or 0.0), flags, _stream()), 'conv2d_fwd_dil')


def conv2d_dil_dgrad_raw(dy, ldy, w, dx, ldx, n, h, wd, dilation, accumulate=False):
    """dx (rows of stride ldx) = / += conv_transpose(dy, w, dilation); dy: rows of stride ldy."""
    _require_gpu(dy, 'conv2d_dgrad_dil')
    cout, cin = _dil_check(w.shape, dilation)
    ws = _dil_workspace(2, n, h, wd, cin, cout, dilation, dy)
    _hip.check(_hip.lib().srhip_conv2d_dgrad_dil(_p(dy), _p(packed_weight(w, 1)), _p(dx), _p(ws), ws.numel() * 4, n, h, wd, cin, cout,
                                                 dilation, ldy, ldx, int(accumulate), _stream()), 'conv2d_dgrad_dil')


def conv2d_dil_wgrad_raw(x, ldx, dy, ldy, w_shape, n, h, wd, dilation, with_bias=True, out=None):
    """(dw [OIHW], db or None) of a dilated 3x3 conv from x and dy (rows of strides ldx / ldy); out=(dw, db): accumulate into them."""
    _require_gpu(x, 'conv2d_wgrad_dil')
    cout, cin = _dil_check(w_shape, dilation)
    ws = _dil_workspace(3, n, h, wd, cin, cout, dilation, x)
    if out is None:
        dw = torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
        db = torch.empty(cout, device=x.device, dtype=torch.float32) if with_bias else None
        acc = 0
    else:
        if not _hip.lib().srhip_conv2d_wgrad_can_accumulate(cin, cout, 3, 3):
            raise NotImplementedError('conv2d_wgrad_dil: accumulating weight gradients need Cin %% 16 == 0 and Cout %% 4 == 0 '
                                      '(srhip_conv2d_wgrad_can_accumulate), got %d -> %d' % (cin, cout))
        (dw, db), acc = out, 1
    _hip.check(_hip.lib().srhip_conv2d_wgrad_dil(_p(x), _p(dy), _p(dw), _p(db), acc, _p(ws), ws.numel() * 4, n, h, wd, cin, cout, dilation,
                                                 ldx, ldy, _stream()), 'conv2d_wgrad_dil')
    return dw, db


class _ConvDil(Function):
    """y = conv(x, w, dilation) + b, stride 1, pad = dilation (first-order: the generator-only AMSSRN step needs no double backward)."""

    @staticmethod
    def forward(ctx, x, w, b, dilation):
        _require_gpu(x, 'conv2d_dil')
        x = nhwc(x)
        n, cin, h, wd = x.shape
        if w.shape[1] != cin:
            raise ValueError('conv2d_dil: weight expects %d input channels, got %d' % (w.shape[1], cin))
        cout = w.shape[0]
        y = empty_nhwc(n, cout, h, wd, x)
        conv2d_dil_fwd_raw(x, cin, w, b, y, cout, n, h, wd, dilation)
        ctx.dilation, ctx.has_bias = dilation, b is not None
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = nhwc(dy)
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = empty_nhwc(n, cin, h, wd, dy)
            conv2d_dil_dgrad_raw(dy, cout, w, dx, cin, n, h, wd, ctx.dilation)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = conv2d_dil_wgrad_raw(x, cin, dy, cout, tuple(w.shape), n, h, wd, ctx.dilation, ctx.has_bias and ctx.needs_input_grad[2])
            if not ctx.needs_input_grad[1]:
                dw = None
        return dx, dw, db, None


def conv2d_dil(x, weight, bias=None, dilation=1):
    """nn.Conv2d(k = 3, padding = dilation, dilation = dilation) forward on the HIP path.  x: logical NCHW; returns NHWC memory."""
    return _ConvDil.apply(x, weight, bias, int(dilation))


def prelu_fwd_raw(z, ldz, y, ldy, slope, rows, ch):
    """y = z > 0 ? z : a z over `rows` pixel rows of ch channels (own row strides); slope: the 1-element device tensor a."""
    _require_gpu(z, 'prelu_fwd')
    _hip.check(_hip.lib().srhip_prelu_fwd(_p(z), ldz, _p(y), ldy, _p(slope.detach()), rows, ch, _stream()), 'prelu_fwd')


def prelu_bwd_raw(g, ldg, z, ldz, dz, lddz, slope, partials, rows, ch):
    """dz = z > 0 ? g : a g; writes srhip_prelu_parts() slope-gradient partials into `partials` (reduce with prelu_slope_reduce_raw)."""
    _require_gpu(g, 'prelu_bwd')
    _hip.check(_hip.lib().srhip_prelu_bwd(_p(g), ldg, _p(z), ldz, _p(dz), lddz, _p(slope.detach()), _p(partials), rows, ch, _stream()),
               'prelu_bwd')


def prelu_slope_reduce_raw(partials, da, accumulate=False):
    """da (=|+=) the fixed-order sum of every partial in `partials`."""
    _hip.check(_hip.lib().srhip_prelu_slope_reduce(_p(partials), partials.numel(), _p(da), int(accumulate), _stream()), 'prelu_slope_reduce')


class _PReLU(Function):
    @staticmethod
    def forward(ctx, z, slope):
        _require_gpu(z, 'prelu')
        if slope.numel() != 1:
            raise NotImplementedError('prelu: one slope per module (nn.PReLU()), got %d' % slope.numel())
        z = nhwc(z)
        n, c, h, w = z.shape
        y = torch.empty_like(z, memory_format=CL)
        prelu_fwd_raw(z, c, y, c, slope, n * h * w, c)
        ctx.save_for_backward(z, slope)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, slope = ctx.saved_tensors
        g = nhwc(g)
        n, c, h, w = z.shape
        dz = torch.empty_like(z, memory_format=CL)
        partials = torch.empty(_hip.lib().srhip_prelu_parts(), device=z.device, dtype=torch.float32)
        prelu_bwd_raw(g, c, z, c, dz, c, slope, partials, n * h * w, c)
        da = torch.empty_like(slope)
        prelu_slope_reduce_raw(partials, da)
        return dz, da


def prelu(z, slope):
    """nn.PReLU() (one slope) on the HIP path; the slope stays on the device."""
    return _PReLU.apply(z, slope)


class _NonLocalQuad(Function):
    """y = softmax(theta^T phi) g on each image quadrant (amssrn.py:103-165), 8 inter channels, NHWC [n, 8, h, w] operands."""

    @staticmethod
    def forward(ctx, th, ph, g):
        _require_gpu(th, 'nl_quad')
        th, ph, g = nhwc(th), nhwc(ph), nhwc(g)
        n, c, h, w = th.shape
        if c != 8 or ph.shape != th.shape or g.shape != th.shape:
            raise NotImplementedError('nl_quad: theta, phi, g of 8 channels and one shape, got %s' % (tuple(th.shape),))
        y = torch.empty_like(th, memory_format=CL)
        ml = torch.empty(n * h * w * 2, device=th.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_nl_quad_fwd(_p(th), _p(ph), _p(g), _p(y), _p(ml), n, h, w, _stream()), 'nl_quad_fwd')
        ctx.save_for_backward(th, ph, g, y, ml)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        th, ph, g, y, ml = ctx.saved_tensors
        dy = nhwc(dy)
        n, _, h, w = th.shape
        dd = torch.empty(n * h * w, device=th.device, dtype=torch.float32)
        dth, dph, dg = (torch.empty_like(th, memory_format=CL) for _ in range(3))
        _hip.check(_hip.lib().srhip_nl_quad_bwd(_p(th), _p(ph), _p(g), _p(y), _p(ml), _p(dy), _p(dd), _p(dth), _p(dph), _p(dg), n, h, w,
                                                _stream()), 'nl_quad_bwd')
        return dth, dph, dg


def nonlocal_quadrants(theta, phi, g):
    return _NonLocalQuad.apply(theta, phi, g)


class _GammaResidual(Function):
    """out = a + gamma * b with gamma a 1-element device tensor (amssrn.py:327-328)."""

    @staticmethod
    def forward(ctx, a, b, gamma):
        _require_gpu(a, 'gamma_res')
        a, b = nhwc(a), nhwc(b)
        out = torch.empty_like(a, memory_format=CL)
        _hip.check(_hip.lib().srhip_gamma_res_fwd(_p(a), _p(b), _p(gamma.detach()), _p(out), a.numel(), _stream()), 'gamma_res_fwd')
        ctx.save_for_backward(b, gamma)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        b, gamma = ctx.saved_tensors
        g = nhwc(g)
        lib = _hip.lib()
        db = torch.empty_like(b, memory_format=CL) if ctx.needs_input_grad[1] else None
        partials = torch.empty(lib.srhip_gamma_parts(), device=g.device, dtype=torch.float32)
        _hip.check(lib.srhip_gamma_res_bwd(_p(g), _p(b), _p(gamma.detach()), _p(db), _p(partials), g.numel(), _stream()), 'gamma_res_bwd')
        dgamma = torch.empty_like(gamma)
        prelu_slope_reduce_raw(partials, dgamma)
        return g, db, dgamma


def gamma_residual(a, b, gamma):
    return _GammaResidual.apply(a, b, gamma)


def channel_attention_bias_prelu(x, w1, b1, slope, w2, b2):
    """CALayer (amssrn.py:167-183) for any C % 4 == 0: x * sigmoid(conv_du(avgpool x)), conv_du = 1x1 (+bias), PReLU, 1x1 (+bias).
    Pooling (srhip_cbam_pool_hw, mean half), the two 1x1 convs on [n, C, 1, 1], PReLU, sigmoid and the per-channel scale all run on
    HIP kernels, each differentiable."""
    n, c = x.shape[:2]
    mean = _PoolHW.apply(x)[:, 0].reshape(n, c, 1, 1)
    z = conv2d(mean, w1, b1)
    u = conv2d(prelu(z, slope), w2, b2)
    s = _Sigmoid.apply(nhwc(u), 0)
    return _Scale.apply(x, s.reshape(n, c), 0)


# --------------------------------------------------------------------------------------------- #
# HAT (model/hat.py): nn.Linear on 1x1 conv routes, LayerNorm, GELU, window attention (SA / OCA), the HAB combine with CAB's
# channel attention (csrc/hat.hip).  Tokens are the NHWC rows of logical [n, C, h, w] channels_last tensors.
# --------------------------------------------------------------------------------------------- #


HAT_SA, HAT_OCA = 0, 1
HAT_WIDE_DIMS = (144, 180)          # the published widths (csrc/hat_wide.hip: srhip_hatw_*); 96 is the reference's (srhip_hat_*)


def _hat_family(c, what):
    """False: the reference's family (C = 96, srhip_hat_*); True: the published one (C = 144 / 180, srhip_hatw_*)."""
    if c == 96:
        return False
    if c in HAT_WIDE_DIMS:
        return True
    raise ValueError('%s: %d channels belong to neither HAT family (96; %s)' % (what, c, ' / '.join(map(str, HAT_WIDE_DIMS))))


class _Linear(Function):
    """y = x W^T + b [+ residual] over the channels of every pixel: the 1x1 conv route with W [out, in] read as [out, in, 1, 1]."""

    @staticmethod
    def forward(ctx, x, w, b, residual):
        y = conv2d_fwd_raw(x, w, b, 1, 0, None, residual)
        ctx.save_for_backward(nhwc(x), w)
        ctx.has_b, ctx.has_res = b is not None, residual is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = nhwc(dy)
        dx = conv2d_dgrad_raw(dy, w, tuple(x.shape), 1, 0) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, db = conv2d_wgrad_raw(x, dy, _wshape(w), 1, 0, ctx.has_b)
            dw = dw.view(w.shape)
        return dx, dw, db, (dy if ctx.has_res and ctx.needs_input_grad[3] else None)


def linear(x, weight, bias=None, residual=None):
    """nn.Linear(in, out) applied to the channel vector of every pixel of x [n, in, h, w] (NHWC memory) -> [n, out, h, w]."""
    return _Linear.apply(x, weight, bias, residual)


def _hat_tokens(x, c, what):
    _require_gpu(x, what)
    x = nhwc(x)
    if x.dim() != 4 or x.shape[1] != c:
        raise ValueError('%s: expected [n, %d, h, w], got %s' % (what, c, tuple(x.shape)))
    return x


class _LayerNorm(Function):
    """nn.LayerNorm(C) over the channels of every pixel (eps 1e-5), C = 96 or a published width."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        c = weight.numel()
        wide = _hat_family(c, 'layer_norm')
        x = _hat_tokens(x, c, 'layer_norm')
        tokens = x.numel() // c
        y = torch.empty_like(x, memory_format=CL)
        stats = torch.empty(2, tokens, device=x.device, dtype=torch.float32)
        if wide:
            _hip.check(_hip.lib().srhip_hatw_ln_fwd(_p(x), _p(weight.detach().contiguous()), _p(bias.detach().contiguous()), _p(y),
                                                    _p(stats[0]), _p(stats[1]), tokens, c, _stream()), 'hatw_ln_fwd')
        else:
            _hip.check(_hip.lib().srhip_hat_ln_fwd(_p(x), _p(weight.detach().contiguous()), _p(bias.detach().contiguous()), _p(y),
                                                   _p(stats[0]), _p(stats[1]), tokens, _stream()), 'hat_ln_fwd')
        ctx.save_for_backward(x, weight, stats)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, stats = ctx.saved_tensors
        dy = nhwc(dy)
        c = weight.numel()
        tokens = x.numel() // c
        lib = _hip.lib()
        dx = torch.empty_like(x, memory_format=CL)
        dg = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        db = torch.empty_like(weight) if ctx.needs_input_grad[2] else None
        if c != 96:
            part = torch.empty(lib.srhip_hatw_ln_parts(tokens) * 2 * c, device=x.device, dtype=torch.float32)
            _hip.check(lib.srhip_hatw_ln_bwd(_p(dy), _p(x), _p(weight.detach().contiguous()), _p(stats[0]), _p(stats[1]), None, _p(dx),
                                             _p(part), _p(dg), _p(db), tokens, c, _stream()), 'hatw_ln_bwd')
            return dx, dg, db
        part = torch.empty(lib.srhip_hat_ln_parts(tokens) * 192, device=x.device, dtype=torch.float32)
        _hip.check(lib.srhip_hat_ln_bwd(_p(dy), _p(x), _p(weight.detach().contiguous()), _p(stats[0]), _p(stats[1]), None, _p(dx),
                                        _p(part), _p(dg), _p(db), tokens, _stream()), 'hat_ln_bwd')
        return dx, dg, db


def layer_norm(x, weight, bias):
    return _LayerNorm.apply(x, weight, bias)


class _Gelu(Function):
    """nn.GELU() (erf form)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, 'gelu')
        x = nhwc(x)
        y = torch.empty_like(x, memory_format=CL)
        _hip.check(_hip.lib().srhip_hat_gelu_fwd(_p(x), _p(y), x.numel(), _stream()), 'hat_gelu_fwd')
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dy = nhwc(dy)
        dx = torch.empty_like(x, memory_format=CL)
        _hip.check(_hip.lib().srhip_hat_gelu_bwd(_p(dy), _p(x), _p(dx), x.numel(), _stream()), 'hat_gelu_bwd')
        return dx


def gelu(x):
    return _Gelu.apply(x)


class _WindowAttention(Function):
    """softmax(q k^T D^-0.5 + table[rpi] [+ mask]) v per window and head, from the qkv Linear's output [n, 3C, h, w]; the output
    [n, C, h, w] sits at the pixels' own positions (the reference's roll / partition / unfold / reverse are addressing).  The table's
    second dimension is the head count; C = 96 goes to srhip_hat_attn_*, the published widths to srhip_hatw_attn_*."""

    @staticmethod
    def forward(ctx, qkv, table, kind, ws, shift):
        _require_gpu(qkv, 'window_attention')
        if qkv.dim() != 4 or qkv.shape[1] % 3:
            raise ValueError('window_attention: expected [n, 3C, h, w], got %s' % (tuple(qkv.shape),))
        c, heads = qkv.shape[1] // 3, table.shape[1]
        wide = _hat_family(c, 'window_attention')
        qkv = _hat_tokens(qkv, 3 * c, 'window_attention')
        n, _, h, w = qkv.shape
        tab = table.detach().contiguous()
        if wide:
            out = empty_nhwc(n, c, h, w, qkv)
            lse = torch.empty(n * h * w * heads, device=qkv.device, dtype=torch.float32)
            _hip.check(_hip.lib().srhip_hatw_attn_fwd(_p(qkv), _p(tab), _p(out), _p(lse), kind, n, h, w, c, heads, ws, shift,
                                                      _stream()), 'hatw_attn_fwd')
            ctx.save_for_backward(qkv, tab, out, lse)
            ctx.cfg = (kind, ws, shift)
            return out
        out = empty_nhwc(n, 96, h, w, qkv)
        lse = torch.empty(n * h * w * 6, device=qkv.device, dtype=torch.float32)
        _hip.check(_hip.lib().srhip_hat_attn_fwd(_p(qkv), _p(tab), _p(out), _p(lse), kind, n, h, w, ws, shift, _stream()),
                   'hat_attn_fwd')
        ctx.save_for_backward(qkv, tab, out, lse)
        ctx.cfg = (kind, ws, shift)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        qkv, tab, out, lse = ctx.saved_tensors
        kind, ws, shift = ctx.cfg
        dout = nhwc(dout)
        n, _, h, w = qkv.shape
        lib = _hip.lib()
        dqkv = torch.empty_like(qkv, memory_format=CL)
        dtab = torch.empty_like(tab)
        c, heads = qkv.shape[1] // 3, tab.shape[1]
        if c != 96:
            nbytes = lib.srhip_hatw_attn_bwd_workspace(kind, n, h, w, c, heads, ws)
            wsp = torch.empty((nbytes + 3) // 4, device=qkv.device, dtype=torch.float32)
            _hip.check(lib.srhip_hatw_attn_bwd(_p(qkv), _p(tab), _p(out), _p(dout), _p(lse), _p(dqkv), _p(dtab), _p(wsp), nbytes, kind,
                                               n, h, w, c, heads, ws, shift, _stream()), 'hatw_attn_bwd')
            return dqkv, dtab, None, None, None
        nbytes = lib.srhip_hat_attn_bwd_workspace(kind, n, h, w, ws)
        wsp = torch.empty((nbytes + 3) // 4, device=qkv.device, dtype=torch.float32)
        _hip.check(lib.srhip_hat_attn_bwd(_p(qkv), _p(tab), _p(out), _p(dout), _p(lse), _p(dqkv), _p(dtab), _p(wsp), nbytes, kind, n,
                                          h, w, ws, shift, _stream()), 'hat_attn_bwd')
        return dqkv, dtab, None, None, None


def window_attention(qkv, table, kind, window_size, shift=0):
    """kind HAT_SA: (shifted) window self-attention of a HAB; HAT_OCA: OCAB's overlapping cross-attention (shift 0)."""
    return _WindowAttention.apply(qkv, table, kind, window_size, shift)


class _HabCombine(Function):
    """out = (x + kb[b] a) + cs (s[b,c] u), s = sigmoid(w2 relu(w1 mean_hw u + b1) + b2) (CAB's ChannelAttention, hat.py:94-107);
    u None: out = x + kb[b] a.  kb None: 1."""

    @staticmethod
    def forward(ctx, x, a, u, w1, b1, w2, b2, kb, cs):
        x = _hat_tokens(x, x.shape[1], 'hab_combine')
        a = nhwc(a)
        n, c, h, w = x.shape
        lib = _hip.lib()
        out = torch.empty_like(x, memory_format=CL)
        s = mz = None
        if u is not None:
            u = nhwc(u)
            hid = w1.shape[0]
            s = torch.empty(n, c, device=x.device, dtype=torch.float32)
            mz = torch.empty(n, c + hid, device=x.device, dtype=torch.float32)
            if b1 is None or b2 is None:
                raise ValueError('hab_combine: the channel attention has biases (nn.Conv2d default)')
            ca_fwd = lib.srhip_hatw_ca_fwd if c in HAT_WIDE_DIMS else lib.srhip_hat_ca_fwd
            _hip.check(ca_fwd(_p(u), _p(w1.detach().contiguous()), _p(b1.detach().contiguous()), _p(w2.detach().contiguous()),
                              _p(b2.detach().contiguous()), _p(s), _p(mz), n, h * w, c, hid, _stream()), 'hat_ca_fwd')
        _hip.check(lib.srhip_hat_combine_fwd(_p(x), _p(a), _p(kb), _p(u), _p(s), _p(out), float(cs), n, h * w, c, _stream()),
                   'hat_combine_fwd')
        ctx.save_for_backward(u, w1, w2, kb, s, mz)
        ctx.cs, ctx.has_u = float(cs), u is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        u, w1, w2, kb, s, mz = ctx.saved_tensors
        g = nhwc(g)
        n, c, h, w = g.shape
        lib = _hip.lib()
        da = torch.empty_like(g, memory_format=CL)
        if not ctx.has_u:
            _hip.check(lib.srhip_hat_combine_bwd(_p(g), _p(kb), None, None, None, None, None, _p(da), None, None, None, None, None,
                                                 None, 0, ctx.cs, n, h * w, c, 1, _stream()), 'hat_combine_bwd')
            return g, da, None, None, None, None, None, None, None
        hid = w1.shape[0]
        du = torch.empty_like(g, memory_format=CL)
        dw1, db1 = torch.empty_like(w1), torch.empty(hid, device=g.device, dtype=torch.float32)
        dw2, db2 = torch.empty_like(w2), torch.empty(c, device=g.device, dtype=torch.float32)
        nbytes = lib.srhip_hat_combine_bwd_workspace(n, c, hid)
        wsp = torch.empty((nbytes + 3) // 4, device=g.device, dtype=torch.float32)
        combine_bwd = lib.srhip_hatw_combine_bwd if c in HAT_WIDE_DIMS else lib.srhip_hat_combine_bwd
        _hip.check(combine_bwd(_p(g), _p(kb), _p(u), _p(s), _p(mz), _p(w1.detach().contiguous()), _p(w2.detach().contiguous()),
                               _p(da), _p(du), _p(dw1), _p(db1), _p(dw2), _p(db2), _p(wsp), nbytes, ctx.cs, n, h * w, c, hid,
                               _stream()), 'hat_combine_bwd')
        return g, da, du, dw1, db1, dw2, db2, None, None


def hab_combine(x, a, u=None, w1=None, b1=None, w2=None, b2=None, kb=None, conv_scale=0.01):
    """HAB (hat.py:289): x + drop_path(a) + conv_scale * CAB(.) where CAB's output is u * ChannelAttention(u); kb [n] holds the
    drop-path factors floor(keep + U) / keep (None: identity).  With u None: x + drop_path(a) (the MLP branch, hat.py:290)."""
    if kb is not None:
        kb = kb.detach().contiguous().float()
    return _HabCombine.apply(x, a, u, w1, b1, w2, b2, kb, conv_scale)
