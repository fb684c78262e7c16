"""The host layer that decides where a parameter gradient ends up (ops._grad_slot, ops._WgradQueue, direct_param_grads, backward_scope,
no_param_grads), driven with CPU tensors: no kernel runs.  The queue's three launch methods are replaced by recorders, so a test sees
WHICH requests go out together and in what order -- the deterministic half of tests/test_grad_delivery_gpu.py, which checks the values
on the device.

What is pinned:
  * a slot exists only inside a context, for a leaf that requires a gradient and owns a dense fp32 .grad on its own device;
  * grouping: off without a side stream; the g-th request of a key launches exactly those g, in request order; keys never mix (shape,
    bias flag, the plane path's operand formats); a request older than _WGRAD_MAX_AGE goes out alone at the next tick; leaving the
    context launches the stragglers, and raises when some are left;
  * ONE SLOT NEVER APPEARS TWICE IN ONE LAUNCH (the grouped kernels' reduce is a plain read-add-write per problem), and the library
    refuses such a launch;
  * every context restores the module state it changed, nested or left by an exception, and requests pending at an exception are
    never launched."""
import ctypes
import types

import pytest
import torch
from torch.autograd import Function

from tests import grad_delivery_cases as C
from tests.grad_delivery_cases import GROUPED_SHAPE

CL = torch.channels_last


@pytest.fixture
def ops():
    from sradsgan_amd import ops as o
    return o


@pytest.fixture
def rec(ops, monkeypatch):
    """The launches of every queue, as ('multi' | 'planes' | 'single', [jobs]) in launch order; no stream, no kernel."""
    out = []
    monkeypatch.setattr(ops, '_stream', lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(ops._WgradQueue, 'run_fp32', lambda self, jobs: out.append(('multi', list(jobs))))
    monkeypatch.setattr(ops._WgradQueue, 'run_planes', lambda self, jobs: out.append(('planes', list(jobs))))
    monkeypatch.setattr(ops._WgradQueue, 'run', lambda self, jobs, launch, extra=(), by_handle=False: out.append(('single', list(jobs))))
    before = _snapshot(ops)
    yield out
    assert _snapshot(ops) == before, 'a test left the module state changed'


def _snapshot(ops):
    s = ops._state
    return (s.wgrads, s.skip_ids, s.stop_ids, s.skip_param_grads)


SIDE = object()                      # stands for a side stream: the recorders never touch it


def _param(*shape, grad=True):
    p = torch.nn.Parameter(torch.zeros(*shape))
    if grad:
        p.grad = torch.zeros(*shape)
    return p


def _conv(shape=GROUPED_SHAPE, bias=True):
    """(w, b, x, dy) of a 3x3 stride-1 pad-1 conv at `shape` = (n, cin, h, w, cout), parameters with dense zero .grad."""
    n, cin, h, w, cout = shape
    x = torch.zeros(n, cin, h, w).contiguous(memory_format=CL)
    dy = torch.zeros(n, cout, h, w).contiguous(memory_format=CL)
    return _param(cout, cin, 3, 3), (_param(cout) if bias else None), x, dy


def _request(ops, c, want_b=True):
    w, b, x, dy = c
    assert ops.wgrad_for_params(w, b, x, dy, 1, 1, want_b and b is not None) == (None, None)


SMALL = (1, 64, 5, 7, 64)            # accumulating kernel, never grouped
OTHER = (8, 64, 32, 32, 128)         # grouped-eligible, another key than GROUPED_SHAPE


def _slots(launch):
    return [j.gw.data_ptr() for j in launch[1]] + [j.gb.data_ptr() for j in launch[1] if j.gb is not None]


def test_shapes_take_the_routes_the_tests_assume(ops):
    from sradsgan_amd import _hip
    lib = _hip.lib()
    assert ops.get_conv_math() == 'bf16x3'
    for n, cin, h, w, cout in (GROUPED_SHAPE, OTHER):
        assert lib.srhip_conv2d_wgrad_can_accumulate(cin, cout, 3, 3) and lib.srhip_conv2d_wgrad_multi_ok(n, h, w, cin, cout, 3, 3, 1, 1) >= 2
    assert lib.srhip_conv2d_wgrad_multi_ok(*OTHER[:1], OTHER[2], OTHER[3], OTHER[1], OTHER[4], 3, 3, 1, 1) >= 3
    n, cin, h, w, cout = SMALL
    assert lib.srhip_conv2d_wgrad_can_accumulate(cin, cout, 3, 3) and lib.srhip_conv2d_wgrad_multi_ok(n, h, w, cin, cout, 3, 3, 1, 1) == 0


# ---- the table ----------------------------------------------------------------------------------------------------------------- #
def test_every_row_reaches_its_route_and_names_an_existing_reference_and_bar(ops):
    """The eligibility predicates are host-only queries: a row that has left its route fails here already.  Every op the layer owns has
    a row, conv2d one per route, and every reference and bar a row names can be imported."""
    import importlib
    from sradsgan_amd import _hip
    lib = _hip.lib()
    for row in C.ROWS:
        with ops.conv_math(row['math']):
            for pred in row['pred']:
                ok, got = C.predicate_holds(pred, lib, ops)
                assert ok, '%s: predicate %s answers %s' % (row['id'], pred, got)
        for spec in row['ref'].split(' + ') + row['bar'].split(' + '):
            mod, name = spec.split(':')
            assert hasattr(importlib.import_module(mod), name), '%s: %s does not exist' % (row['id'], spec)
    assert {r['op'] for r in C.ROWS} == set(C.OPS)
    conv_routes = {r['id'] for r in C.ROWS if r['op'] == 'conv2d'}
    assert conv_routes == {'conv-accumulate', 'conv-grouped', 'conv-add-3to64', 'conv-add-64to3', 'conv-act-direct', 'conv-head-mask'}
    assert {r['route'] for r in C.ROWS if r['op'] == 'rab_block'} == {'accumulate', 'planes'}
    assert {r.get('la_mode') for r in C.ROWS if r['op'] == 'attention_variant'} == {'CA', 'SA'}
    assert {r.get('affine', True) for r in C.ROWS if r['op'] == 'group_norm_act'} == {True, False}
    for row in C.ROWS:                                   # H != W everywhere, an odd side unless the shape is a tabulated case of the op's reference
        h, w = (row['shape'][2], row['shape'][3])
        assert h != w and (h % 2 or w % 2 or row['build'] in ('tail', 'variant')), row['id']


def test_the_grouped_shape_is_the_smallest_the_library_groups():
    """GROUPED_SHAPE: 2052 pixels.  One pixel row or column less, or one image less, and srhip_conv2d_wgrad_multi_ok declines."""
    from sradsgan_amd import _hip
    ok = _hip.lib().srhip_conv2d_wgrad_multi_ok
    n, cin, h, w, cout = GROUPED_SHAPE
    assert ok(n, h, w, cin, cout, 3, 3, 1, 1) >= 2 and h % 2 and w % 2 and h != w
    assert ok(n, h - 1, w, cin, cout, 3, 3, 1, 1) == 0 and ok(n, h, w - 1, cin, cout, 3, 3, 1, 1) == 0 and ok(n - 1, h, w, cin, cout, 3, 3, 1, 1) == 0
    assert ok(8, 32, 32, cin, cout, 3, 3, 1, 1) >= 2, 'the row of tests/conv_geometry_cases.py the search started from'


# ---- _grad_slot -------------------------------------------------------------------------------------------------------------- #
def test_grad_slot_needs_a_context_a_leaf_and_a_dense_fp32_grad_on_the_parameters_device(ops, rec):
    p = _param(4, 6)
    assert ops._grad_slot(p) is None, 'outside a context'
    with ops.direct_param_grads(None):
        assert ops._grad_slot(p) is p.grad
        assert ops._grad_slot(None) is None
        nonleaf = p * 2.0
        assert not nonleaf.is_leaf and ops._grad_slot(nonleaf) is None, 'a non-leaf tensor'
        frozen = _param(4, 6)
        frozen.requires_grad_(False)
        assert ops._grad_slot(frozen) is None, 'requires_grad=False'
        assert ops._grad_slot(_param(4, 6, grad=False)) is None, 'grad is None'
        strided = _param(4, 6, grad=False)
        strided.grad = torch.zeros(6, 4).t()
        assert not strided.grad.is_contiguous() and ops._grad_slot(strided) is None, 'a non-contiguous grad'
        double = torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.float64))
        double.grad = torch.zeros(4, 6, dtype=torch.float64)
        assert ops._grad_slot(double) is None, 'a grad that is not fp32'
        # torch refuses to ASSIGN a .grad of another dtype or device, so these two stand in for a parameter that got one another way
        g = torch.zeros(4, 6)
        away = types.SimpleNamespace(requires_grad=True, is_leaf=True, grad=g, device=torch.device('cuda:0'))
        assert ops._grad_slot(away) is None, 'a grad on another device than the parameter'
        here = types.SimpleNamespace(requires_grad=True, is_leaf=True, grad=g, device=g.device)
        assert ops._grad_slot(here) is g
        half = types.SimpleNamespace(requires_grad=True, is_leaf=True, grad=g.half(), device=g.device)
        assert ops._grad_slot(half) is None, 'a grad of the wrong dtype'
    assert ops._grad_slot(p) is None


def test_a_missing_slot_sends_the_gradient_back_to_the_caller(ops, rec, monkeypatch):
    """Weight with a slot, bias without (and the reverse): no direct accumulation, the plain kernel's results are returned."""
    calls = []
    monkeypatch.setattr(ops, 'conv2d_wgrad_raw', lambda *a, **k: calls.append((a, k)) or ('dw', 'db'))
    for strip in ('w', 'b'):
        w, b, x, dy = _conv(SMALL)
        (w if strip == 'w' else b).grad = None
        with ops.direct_param_grads(SIDE, 2):
            assert ops.wgrad_for_params(w, b, x, dy, 1, 1, True) == ('dw', 'db')
            assert ops.wgrad_pp_for_params(w, b, x, dy, True) is False
            assert ops._wgrad_act_direct(w, b, x, dy, dy, 0.2, 1, 1) is False
    assert len(calls) == 2 and all('out' not in k for _, k in calls) and rec == []


# ---- grouping and age -------------------------------------------------------------------------------------------------------- #
def test_without_a_side_stream_nothing_waits(ops, rec):
    assert ops._WgradQueue(None, 2).group == 1 and ops._WgradQueue(SIDE, 2).group == 2
    a, b = _conv(), _conv()
    with ops.direct_param_grads(None, 2):
        _request(ops, a)
        assert [k for k, _ in rec] == ['single'] and not ops._state.wgrads.pending
        _request(ops, b)
    assert [(k, len(j)) for k, j in rec] == [('single', 1), ('single', 1)]
    assert rec[0][1][0].gw is a[0].grad and rec[1][1][0].gw is b[0].grad


@pytest.mark.parametrize('g', [2, 3])
def test_the_gth_request_of_a_key_launches_exactly_those_g_in_request_order(ops, rec, g):
    convs = [_conv(OTHER) for _ in range(2 * g)]
    with ops.direct_param_grads(SIDE, g):
        for i, c in enumerate(convs):
            _request(ops, c)
            assert len(rec) == (i + 1) // g, 'request %d' % i
        assert not ops._state.wgrads.pending
    assert [k for k, _ in rec] == ['multi', 'multi']
    for li, (_, jobs) in enumerate(rec):
        assert [j.gw for j in jobs] == [c[0].grad for c in convs[li * g:(li + 1) * g]]
        assert [j.gb for j in jobs] == [c[1].grad for c in convs[li * g:(li + 1) * g]]
        assert all(j.x is c[2] and j.dy is c[3] for j, c in zip(jobs, convs[li * g:(li + 1) * g]))


def test_requests_of_different_keys_never_share_a_launch(ops, rec):
    """Shape, output channels and the bias flag are the key of an fp32 request."""
    a1, a2 = _conv(GROUPED_SHAPE), _conv(GROUPED_SHAPE)
    o1, o2 = _conv(OTHER), _conv(OTHER)
    n1, n2 = _conv(GROUPED_SHAPE, bias=False), _conv(GROUPED_SHAPE, bias=False)
    with ops.direct_param_grads(SIDE, 2):
        for c in (a1, o1, n1):
            _request(ops, c)
        assert rec == [] and len(ops._state.wgrads.pending) == 3
        _request(ops, n2)
        _request(ops, o2)
        _request(ops, a2)
    assert [[j.gw for j in jobs] for _, jobs in rec] == [[n1[0].grad, n2[0].grad], [o1[0].grad, o2[0].grad], [a1[0].grad, a2[0].grad]]
    assert [j.gb for j in rec[0][1]] == [None, None]


def test_a_bias_gradient_that_is_not_wanted_is_another_key(ops, rec):
    a, b = _conv(), _conv()
    with ops.direct_param_grads(SIDE, 2):
        _request(ops, a)
        _request(ops, b, want_b=False)
        assert rec == [], 'a launch has one bias flag: these two must not pair'
    assert sorted(len(j) for _, j in rec) == [1, 1]


def test_plane_requests_group_by_operand_formats(ops, rec):
    n, cin, h, w, cout = SMALL
    pp = lambda c: ops.PP(torch.zeros(1, 2 * c, dtype=torch.bfloat16), n, c, h, w)
    convs = [_conv(SMALL) for _ in range(2 * ops._PP_GROUP)]
    with ops.direct_param_grads(SIDE, 2):
        for i, (wt, b, x, dy) in enumerate(convs):
            xo = pp(cin) if i % 2 else x            # formats alternate: (fp32, planes) and (planes, planes)
            assert ops.wgrad_pp_for_params(wt, b, xo, pp(cout), True) is True
            if i < 2 * ops._PP_GROUP - 2:
                assert rec == []
    assert [k for k, _ in rec] == ['planes', 'planes']
    for li, (_, jobs) in enumerate(rec):
        assert [j.gw for j in jobs] == [c[0].grad for c in convs[li::2]]
        assert len({(isinstance(j.x, ops.PP), isinstance(j.dy, ops.PP)) for j in jobs}) == 1
    rec.clear()
    with ops.direct_param_grads(None, 2):           # no side stream: at once, alone
        wt, b, x, dy = convs[0]
        assert ops.wgrad_pp_for_params(wt, b, x, pp(cout), True) is True
        assert [(k, len(j)) for k, j in rec] == [('planes', 1)]


def test_a_request_older_than_the_age_limit_goes_out_alone_at_the_next_tick(ops, rec):
    first = _conv()
    others = [_conv(SMALL) for _ in range(ops._WGRAD_MAX_AGE + 1)]
    with ops.direct_param_grads(SIDE, 2):
        _request(ops, first)
        for c in others[:-1]:
            _request(ops, c)
        assert [k for k, _ in rec] == ['single'] * ops._WGRAD_MAX_AGE, 'the limit itself is not yet too old'
        _request(ops, others[-1])
        assert rec[-2][0] == 'multi' and [j.gw for j in rec[-2][1]] == [first[0].grad], 'launched alone, before the request that aged it'
        assert rec[-1][1][0].gw is others[-1][0].grad and not ops._state.wgrads.pending
    assert len(rec) == ops._WGRAD_MAX_AGE + 2


def test_leaving_the_context_launches_every_straggler(ops, rec):
    a, o = _conv(GROUPED_SHAPE), _conv(OTHER)
    with ops.direct_param_grads(SIDE, 2):
        _request(ops, a)
        _request(ops, o)
        assert rec == []
    assert [[j.gw for j in jobs] for _, jobs in rec] == [[a[0].grad], [o[0].grad]]


def test_jobs_left_behind_by_the_final_flush_raise(ops, rec, monkeypatch):
    monkeypatch.setattr(ops._WgradQueue, 'flush_all', lambda self: None)
    with pytest.raises(RuntimeError, match='still waiting for a partner'):
        with ops.direct_param_grads(SIDE, 2):
            _request(ops, _conv())
    assert ops._state.wgrads is None and rec == []


# ---- one slot, one launch ---------------------------------------------------------------------------------------------------- #
def _assert_slots_distinct(rec):
    for launch in rec:
        s = _slots(launch)
        assert len(s) == len(set(s)), 'one launch holds a gradient slot twice: its problems race on it'


def test_two_requests_for_one_parameter_never_share_a_launch(ops, rec):
    """A weight used twice in one graph, or one conv in two successive backward calls of one context: the second request sends the
    waiting one out first, so both contributions reach the slot one after the other on the side stream."""
    c = _conv()
    with ops.direct_param_grads(SIDE, 2):
        _request(ops, c)
        _request(ops, c)
    _assert_slots_distinct(rec)
    assert [[j.gw for j in jobs] for _, jobs in rec] == [[c[0].grad], [c[0].grad]], 'both contributions, in request order'


def test_a_repeated_slot_waits_for_the_next_partner(ops, rec):
    c, d = _conv(), _conv()
    with ops.direct_param_grads(SIDE, 2):
        for r in (c, d, c, c, d):
            _request(ops, r)
    _assert_slots_distinct(rec)
    assert [[j.gw for j in jobs] for _, jobs in rec] == [[c[0].grad, d[0].grad], [c[0].grad], [c[0].grad, d[0].grad]]


def test_a_shared_bias_slot_keeps_two_weights_apart(ops, rec):
    c, d = _conv(), _conv()
    d = (d[0], c[1], d[2], d[3])
    with ops.direct_param_grads(SIDE, 2):
        _request(ops, c)
        _request(ops, d)
    _assert_slots_distinct(rec)
    assert sum(len(j) for _, j in rec) == 2


def test_plane_requests_for_one_parameter_never_share_a_launch(ops, rec):
    n, cin, h, w, cout = SMALL
    wt, b, x, dy = _conv(SMALL)
    with ops.direct_param_grads(SIDE, 2):
        for _ in range(ops._PP_GROUP):
            assert ops.wgrad_pp_for_params(wt, b, x, dy, True)
    _assert_slots_distinct(rec)
    assert sum(len(j) for _, j in rec) == ops._PP_GROUP


def test_the_library_refuses_a_grouped_launch_with_a_repeated_destination():
    """srhip_conv2d_wgrad_multi checks its pointer tables before anything touches the device."""
    from sradsgan_amd import _hip
    lib = _hip.lib()
    n, cin, h, w, cout = GROUPED_SHAPE
    tab = ctypes.c_void_p * 2
    ops_ = tab(256, 512)
    args = (1, None, 0, n, h, w, cin, cout, 3, 3, 1, 1, cin, cout, None)
    assert lib.srhip_conv2d_wgrad_multi(2, ops_, ops_, tab(1024, 1024), None, *args) == -1
    assert b'share a destination' in lib.srhip_last_error()
    assert lib.srhip_conv2d_wgrad_multi(2, ops_, ops_, tab(1024, 2048), tab(4096, 4096), *args) == -1
    assert b'share a destination' in lib.srhip_last_error()
    tab3 = ctypes.c_void_p * 3
    assert lib.srhip_conv2d_wgrad_multi(3, tab3(1, 2, 3), tab3(1, 2, 3), tab3(1024, 2048, 1024), None, *args) == -1
    assert b'problems 0 and 2 share a destination' in lib.srhip_last_error()
    assert lib.srhip_conv2d_wgrad_multi(1, ops_, ops_, tab(1024, 2048), None, *args) == -1
    assert b'2..4 problems' in lib.srhip_last_error()


# ---- the accumulate flag ------------------------------------------------------------------------------------------------------- #
def test_a_launch_into_a_slot_asks_the_kernel_to_accumulate(ops, monkeypatch):
    """conv2d_wgrad_raw(out=...) must pass accumulate = 1 (the slot holds earlier contributions), and 0 into a fresh buffer."""
    seen = []

    class Lib:
        def srhip_conv2d_wgrad_workspace(self, *a):
            return 64

        def srhip_conv2d_wgrad(self, *a):
            seen.append(a)
            return 0
    from sradsgan_amd import _hip
    monkeypatch.setattr(_hip, 'lib', lambda: Lib())
    monkeypatch.setattr(ops, '_require_gpu', lambda t, what: None)
    monkeypatch.setattr(ops, '_stream', lambda: ctypes.c_void_p(0))
    w, b, x, dy = _conv(SMALL)
    dw, db = ops.conv2d_wgrad_raw(x, dy, tuple(w.shape), 1, 1, True, out=(w.grad, b.grad))
    assert dw is w.grad and db is b.grad and seen[-1][6] == 1
    assert seen[-1][2].value == w.grad.data_ptr() and seen[-1][3].value == b.grad.data_ptr()
    dw, db = ops.conv2d_wgrad_raw(x, dy, tuple(w.shape), 1, 1, True)
    assert dw is not w.grad and seen[-1][6] == 0


# ---- pruning and state ------------------------------------------------------------------------------------------------------- #
def test_skip_params_match_by_identity_and_stop_at_by_address(ops, rec):
    w, v = _param(4, 6), _param(4, 6)
    x = torch.zeros(3, 5)
    assert not ops._skip_param_grads(w)
    with ops.backward_scope(skip_params=[w], stop_at=(x,)):
        assert ops._skip_param_grads(w) and ops._skip_param_grads(None, w) and ops._skip_param_grads(v, w)
        assert not ops._skip_param_grads(v) and not ops._skip_param_grads(None) and not ops._skip_param_grads()
        assert ops._state.stop_ids == {x.data_ptr()}
        assert x.detach().requires_grad_().data_ptr() in ops._state.stop_ids, 'a detached alias has the address, so it is cut too'
        assert x.clone().data_ptr() not in ops._state.stop_ids
        with ops.no_param_grads():
            assert ops._skip_param_grads(v) and ops._skip_param_grads()
        assert not ops._skip_param_grads(v)
    assert not ops._skip_param_grads(w) and ops._state.stop_ids == frozenset() and ops._state.skip_ids == frozenset()


def test_nested_contexts_restore_what_they_found(ops, rec):
    w, v, x, z = _param(4), _param(4), torch.zeros(3), torch.zeros(3)
    with ops.direct_param_grads(SIDE, 2):
        outer = ops._state.wgrads
        waiting = _conv()
        _request(ops, waiting)
        with ops.backward_scope(skip_params=[w], stop_at=(x,)):
            with ops.backward_scope(skip_params=[v], stop_at=(z,)):
                assert ops._state.skip_ids == {id(v)} and ops._state.stop_ids == {z.data_ptr()}
                with ops.no_param_grads(), ops.no_param_grads():
                    assert ops._state.skip_param_grads is True
                assert ops._state.skip_param_grads is False
                with ops.direct_param_grads(None):
                    assert ops._state.wgrads is not outer and ops._state.wgrads.side is None
                assert ops._state.wgrads is outer and rec == [], 'the inner context flushed its own queue only'
            assert ops._state.skip_ids == {id(w)} and ops._state.stop_ids == {x.data_ptr()}
        assert ops._state.skip_ids == frozenset() and ops._state.stop_ids == frozenset()
        assert list(outer.pending.values())[0][0].gw is waiting[0].grad
    assert ops._state.wgrads is None and len(rec) == 1


class _RequestThenRaise(Function):
    """A backward that asks for a grouped weight gradient (which then waits for a partner) and fails."""

    @staticmethod
    def forward(ctx, t, ops, conv):
        ctx.ops, ctx.conv = ops, conv
        return t * 1.0

    @staticmethod
    def backward(ctx, g):
        _request(ctx.ops, ctx.conv)
        raise ValueError('boom in backward')


def test_an_exception_mid_backward_restores_the_state_and_drops_the_pending_jobs(ops, rec):
    w, x = _param(4), torch.zeros(3)
    t = torch.ones(2, requires_grad=True)
    lost, later = _conv(), _conv()
    with pytest.raises((ValueError, RuntimeError), match='boom in backward'):
        with ops.direct_param_grads(SIDE, 2), ops.backward_scope(skip_params=[w], stop_at=(x,)), ops.no_param_grads():
            assert ops._state.skip_param_grads and ops._state.skip_ids and ops._state.stop_ids and ops._state.wgrads is not None
            _RequestThenRaise.apply(t, ops, lost).sum().backward()
    assert _snapshot(ops) == (None, frozenset(), frozenset(), False)
    assert rec == [], 'the request that was pending at the exception must never be launched'
    with ops.direct_param_grads(SIDE, 2):
        _request(ops, later)
    assert [[j.gw for j in jobs] for _, jobs in rec] == [[later[0].grad]], 'the next context starts from an empty queue'
    for ctx in (lambda: ops.backward_scope(skip_params=[w], stop_at=(x,)), ops.no_param_grads, lambda: ops.direct_param_grads(None)):
        with pytest.raises(KeyError):
            with ctx():
                raise KeyError('left by an exception')
        assert _snapshot(ops) == (None, frozenset(), frozenset(), False)
