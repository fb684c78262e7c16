"""The table of tests/test_grad_delivery_gpu.py: one row per op of sradsgan_amd/ops.py that owns or reaches a parameter gradient under
TrainStep, at the smallest shape on which the row's ROUTE is taken.  Pure Python: importable (and checked, tests/test_grad_delivery_cpu.py)
without a device.

A row:
  id, op     the op of ops.py and the name of the row
  route      how its parameter gradients travel inside ops.direct_param_grads():
               'accumulate'  the accumulating weight-gradient kernel writes into the slot (conv2d_wgrad_raw(out=...))
               'grouped'     the request waits in _WgradQueue.pending for a partner, one srhip_conv2d_wgrad_multi launch serves both
               'add'         the plain kernel into a fresh buffer, then slot.add_(buffer) in program order
               'planes'      ops.wgrad_pp_for_params: the flat kernel on padded planes, in groups of _PP_GROUP
               'kernel-slot' a norm / attention kernel takes the slot as acc_gamma / acc_beta / dgamma / dw7 / dfc and adds into it itself
               'autograd'    the op always returns the gradient: AccumulateGrad adds it to .grad
  shape      (n, cin, h, w, cout) of a conv row, (n, c, h, w) otherwise: odd H != W where the route allows
  pred       the route's eligibility predicates as (name, arguments, comparison, value), evaluated by predicate_holds(): a row that
             cannot reach its route FAILS (on the CPU already), it never takes another route silently
  math       the conv arithmetic the row runs in (ops.conv_math)
  slots      the parameters that use a slot inside a context (their returned gradient is None); every other one goes through autograd
  exact      the parameters whose delivery adds the same fp32 sum once: .grad == fp32(G0 + g_A) bit for bit (the add_ fallback, the norm
             and dgamma slots, the tail's dw7 / dfc accumulate flags -- tests/test_reductions_gpu.py, test_groupnorm_gpu.py,
             test_global_attn_kernels_gpu.py and test_attn_tail_gpu.py hold the kernels' flags to bit equality -- and AccumulateGrad's
             in-place add).  The accumulating and grouped conv kernels fold the prior into their split-K reduce and document no identity.
  ref        the existing fp64 reference the plain run is held to, 'module:function'
  bar        where the bar is imported from, 'module:name' -- no number is restated here
  arith      (conv routes) the arithmetic of the weight-gradient kernel the row lands on, a tests/conv_emulation.py name
  dx         'bits': the data gradient under a context equals the plain run's bit for bit (no op documents another route for it)
  pair       (weight, bias)-like parameter pair of the mixed-slot test
  build      the builder of tests/test_grad_delivery_gpu.py that turns the row into tensors
  seed       (rab rows) the draw whose u = conv2(lrelu(conv1 x)) keeps the tail's arg-max and ReLU decisions clear of a flip: channel, pixel,
             relu margins of attn_tail_ref.margins 8e-4, 5e-4, 0.057 (rab-fp32) and 4e-3, 3e-3, 0.022 (rab-planes), measured in fp32 torch;
             the GPU test asserts attn_tail_ref.assert_margins on the u it meets

GROUPED_SHAPE was found as the issue says: from the ('rowtap', 'multi') row of tests/conv_geometry_cases.py (8 x 64 -> 128 x 32 x 32, 8192
pixels) shrunk while srhip_conv2d_wgrad_multi_ok still answers >= 2.  The answer depends on the pixel count alone at these channels: 2052
pixels is the smallest count served (2048 = 2 x 32 x 32 is not), and 4 x 19 x 27 = 2052 is its smallest factorisation with odd H != W."""

GROUPED_SHAPE = (4, 64, 19, 27, 128)
HEAD_PIXELS = (1, 241, 273)          # 65793 pixels: the head-mask record and srhip_conv2d_wgrad_act need >= 65536; odd H != W
CONV_BAR = 'tests.test_conv_routes_gpu:TAU'
REL_BAR = 'tests.reduction_ref:bound'
ROWS = []
CONTEXTS = (('none', False, 1), ('side-1', True, 1), ('side-2', True, 2))      # (id, side stream, group)


def _conv_pred(shape, k=3, stride=1, pad=1, accumulate=None, multi=None, act=None, head=None):
    n, cin, h, w, cout = shape
    p = []
    if accumulate is not None:
        p.append(('srhip_conv2d_wgrad_can_accumulate', (cin, cout, k, k), '==', int(accumulate)))
    if multi is not None:
        p.append(('srhip_conv2d_wgrad_multi_ok', (n, h, w, cin, cout, k, k, stride, pad)) + multi)
    if act is not None:
        p.append(('srhip_conv2d_wgrad_act_ok', (n, h, w, cin, cout, k, k, stride, pad), '==', int(act)))
    if head is not None:
        p.append(('srhip_conv2d_head_mask_ok', (n, h, w, cin, cout, k, k, stride, pad), '==', int(head)))
    return p


def add(id, op, route, shape, ref, bar, build, slots=(), exact=(), pred=(), math='bf16x3', dx='bits', pair=None, **opt):
    assert route in ('accumulate', 'grouped', 'add', 'planes', 'kernel-slot', 'autograd'), route
    row = dict(id=id, op=op, route=route, shape=tuple(shape), ref=ref, bar=bar, build=build, slots=tuple(slots), exact=tuple(exact), pred=list(pred),
               math=math, dx=dx, pair=pair, **opt)
    ROWS.append(row)
    return row


# ---- conv2d, one row per route ------------------------------------------------------------------------------------------------------------ #
WREF = 'tests.conv_emulation:conv_wgrad'
_S = (2, 64, 7, 9, 64)
add('conv-accumulate', 'conv2d', 'accumulate', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), pair=('w', 'b'), arith='bf16x3', slope=0.2,
    pred=_conv_pred(_S, accumulate=True, multi=('==', 0)))
add('conv-grouped', 'conv2d', 'grouped', GROUPED_SHAPE, WREF, CONV_BAR, 'conv', slots=('w', 'b'), pair=('w', 'b'), arith='bf16x3', slope=None,
    pred=_conv_pred(GROUPED_SHAPE, accumulate=True, multi=('>=', 2)),
    note='under (side, group 2) the single request waits for a partner and leaves with the flush at the end of the context')
_S = (2, 3, 7, 9, 64)
add('conv-add-3to64', 'conv2d', 'add', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), exact=('w', 'b'), pair=('w', 'b'), arith='fp32', slope=0.2,
    pred=_conv_pred(_S, accumulate=False, head=False))
_S = (2, 64, 7, 9, 3)
add('conv-add-64to3', 'conv2d', 'add', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), exact=('w', 'b'), pair=('w', 'b'), arith='fp32', slope=None,
    pred=_conv_pred(_S, accumulate=False))
_S = (HEAD_PIXELS[0], 3, HEAD_PIXELS[1], HEAD_PIXELS[2], 32)
add('conv-act-direct', 'conv2d', 'add', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), arith='fp32', slope=0.2, want_dx=False,
    pred=_conv_pred(_S, accumulate=False, act=True, head=False),
    note='ops._wgrad_act_direct: only the parameter gradients are wanted (x needs none), so there is no data gradient to compare; 32 output channels '
         'keep the row off the head-mask record, which takes every 3 -> 64 conv of this size first.  Not `exact`: srhip_conv2d_wgrad_act applies '
         'the mask while it reads dy, the plain run a pass of its own, and nothing documents the two as bit-identical')
_S = (HEAD_PIXELS[0], 3, HEAD_PIXELS[1], HEAD_PIXELS[2], 64)
add('conv-head-mask', 'conv2d', 'add', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), exact=('w', 'b'), arith='fp32', slope=0.2,
    pred=_conv_pred(_S, accumulate=False, head=True))
_S = (2, 64, 7, 9, 64)
add('conv-pool', 'conv2d_pool', 'accumulate', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), pair=('w', 'b'), arith='bf16x3', slope=None, pool=True,
    pred=_conv_pred(_S, accumulate=True, multi=('==', 0)) + [('pool_epilogue_ok', (64, 64, 3), '==', 1)])
_S = (2, 64, 5, 7, 256)
add('pixel-shuffle-behind-conv', 'pixel_shuffle_act', 'accumulate', _S, WREF, CONV_BAR, 'conv', slots=('w', 'b'), arith='bf16x3', slope=None, shuffle=(2, 0.2),
    pred=_conv_pred(_S, accumulate=True, multi=('==', 0)),
    note='pixel_shuffle_act has no parameter: the row holds the conv in front of it to the gradient the shuffle hands back')
_S = (2, 16, 5, 7, 48)
add('conv-dilated', 'conv2d_dil', 'autograd', _S, WREF, CONV_BAR, 'conv', exact=('w', 'b'), pair=('w', 'b'), arith='bf16x3', slope=None, dilation=2)
_S = (2, 96, 5, 7, 192)
add('linear', 'linear', 'autograd', _S, WREF, CONV_BAR, 'conv', exact=('w', 'b'), pair=('w', 'b'), arith='bf16x3', slope=None, linear=True)

# ---- the fused residual attention block and its tails ----------------------------------------------------------------------------------- #
TAIL_REF = 'tests.attn_tail_ref:e2e_ref'
RAB_PARAMS = ('w1', 'b1', 'w2', 'b2', 'fc1', 'fc2', 'w7', 'wc', 'bc')
add('rab-fp32', 'rab_block', 'accumulate', (2, 64, 9, 11), TAIL_REF + ' + ' + WREF, REL_BAR + ' + ' + CONV_BAR, 'rab', slots=RAB_PARAMS,
    exact=('fc1', 'fc2', 'w7'), math='fp32', cmid=256, pred=[('rab_planes_ok', (2, 64, 9, 11, 256), '==', 0)], arith='fp32', seed=3)
add('rab-planes', 'rab_block', 'planes', (2, 64, 9, 11), TAIL_REF + ' + ' + WREF, REL_BAR + ' + ' + CONV_BAR, 'rab', slots=RAB_PARAMS,
    exact=('fc1', 'fc2', 'w7'), math='bf16x3', cmid=256, pred=[('rab_planes_ok', (2, 64, 9, 11, 256), '==', 1)], arith='bf16x3', seed=5,
    note='under (side, group 2) conv1 and conv2 wait in the plane queue (different shapes, _PP_GROUP partners never come) and leave with the flush.  '
         'Inside a context the two 3x3 weight gradients are held to the emulation on the plane HALVES the block hands to the flat kernel (recorded at the '
         'request); the plain run decodes the planes and runs the row-tap kernel, and is held to the emulation on the decoded operands')
add('attention-tail', 'attention_tail', 'kernel-slot', (3, 64, 10, 12), TAIL_REF, REL_BAR, 'tail', slots=('fc1', 'fc2', 'w7', 'wc', 'bc'),
    exact=('fc1', 'fc2', 'w7'), note='wc / bc: the accumulating weight-gradient kernel with both operand scales; the case and its seed are attn_tail_ref\'s: 3 x 10 x 12 is the '
    'smallest tabulated shape whose n is no power of two (its arg-max margins are asserted there)')
add('variant-clam', 'attention_variant', 'kernel-slot', (3, 64, 10, 12), 'tests.attn_variants_ref:variant_grads', REL_BAR, 'variant',
    slots=('fc1', 'fc2'), exact=('fc1', 'fc2'), la_mode='CA', pool_mode='Avg|Max')
add('variant-slam', 'attention_variant', 'kernel-slot', (3, 64, 10, 12), 'tests.attn_variants_ref:variant_grads', REL_BAR, 'variant',
    slots=('w7',), exact=('w7',), la_mode='SA', pool_mode='Avg|Max')
add('cgam', 'cgam', 'kernel-slot', (2, 64, 3, 5), 'tests.attn_kernels_ref:cgam_eval', 'tests.attn_kernels_ref:bars', 'gam', slots=('gamma',), exact=('gamma',))
add('sgam', 'sgam', 'kernel-slot', (2, 64, 3, 11), 'tests.attn_kernels_ref:sgam_eval', 'tests.attn_kernels_ref:bars', 'gam', slots=('gamma',), exact=('gamma',))

# ---- norms ------------------------------------------------------------------------------------------------------------------------------------ #
add('batch-norm', 'batch_norm_act', 'kernel-slot', (3, 12, 5, 7), 'tests.reduction_ref:bn_bwd_ref', REL_BAR, 'norm', slots=('gamma', 'beta'),
    exact=('gamma', 'beta'), pair=('gamma', 'beta'), slope=0.2)
add('group-norm-affine', 'group_norm_act', 'kernel-slot', (3, 64, 5, 7), 'tests.groupnorm_ref:gn_bwd_ref', REL_BAR, 'norm', slots=('gamma', 'beta'),
    exact=('gamma', 'beta'), pair=('gamma', 'beta'), slope=0.2, groups=32, unbiased=True)
add('group-norm-plain', 'group_norm_act', 'kernel-slot', (3, 64, 5, 7), 'tests.groupnorm_ref:gn_bwd_ref', REL_BAR, 'norm', slope=0.2, groups=64, unbiased=False,
    affine=False, note='no parameter: the row holds the data gradient and shows that a context changes nothing')

# ---- spectral normalisation: the effective weight is no leaf ----------------------------------------------------------------------------------- #
add('spectral', 'spectral_weights', 'kernel-slot', (2, 64, 7, 9, 64), 'tests.test_spectral_gpu:test_projection_against_fp64 + ' + WREF,
    'tests.test_spectral_gpu:_bar + ' + CONV_BAR, 'spectral', slots=('wbar',), exact=('b',), arith='bf16x3',
    note='the projection formula is test_projection_against_fp64\'s.  conv2d on W = weight_bar / sigma: W is no leaf, so its weight gradient goes back to autograd, which hands the sum to '
         '_SpectralWeights.backward; that projects it into weight_bar\'s slot.  The bias travels beside the non-leaf weight: through autograd')

# ---- ops that always return their parameter gradients: the same property must hold through AccumulateGrad ------------------------------------- #
add('layer-norm', 'layer_norm', 'autograd', (2, 96, 3, 5), 'tests.attn_kernels_ref:ln_eval', REL_BAR, 'leaf', exact=('gamma', 'beta'), pair=('gamma', 'beta'))
add('prelu', 'prelu', 'autograd', (2, 12, 5, 7), 'tests.leaf_kernels_ref:prelu_slope_eval', REL_BAR, 'leaf', exact=('slope',))
add('gamma-residual', 'gamma_residual', 'autograd', (2, 12, 5, 7), 'tests.leaf_kernels_ref:gamma_sum_eval', REL_BAR, 'leaf', exact=('gamma',))
add('ca-residual', 'ca_residual', 'autograd', (2, 64, 5, 7), 'tests.leaf_kernels_ref:ca_chain_ref', REL_BAR, 'leaf', exact=('fc1', 'fc2', 'b1', 'b2'),
    pair=('fc1', 'b1'))
add('dense-block', 'dense_block', 'autograd', (2, 64, 5, 7), 'tests.ndsrgan_ref:Dense', REL_BAR, 'dense', math='fp32',
    exact=tuple('%s%d' % (k, i) for i in range(1, 6) for k in 'wb'),
    note='exact-fp32 conv arithmetic, so that the reference\'s own fp32 error is the yardstick (the block\'s kernel test states its bar as a number)')

IDS = [r['id'] for r in ROWS]
BY_ID = {r['id']: r for r in ROWS}
# the ops the issue names, each with at least one row
OPS = ('conv2d', 'conv2d_pool', 'rab_block', 'attention_tail', 'attention_variant', 'cgam', 'sgam', 'batch_norm_act', 'group_norm_act', 'spectral_weights',
       'pixel_shuffle_act', 'linear', 'conv2d_dil', 'layer_norm', 'prelu', 'ca_residual', 'gamma_residual', 'dense_block')


def predicate_holds(pred, lib, ops):
    """One (name, arguments, comparison, value) of a row against the library (host-only queries) and ops' own predicates."""
    name, args, cmp, want = pred
    if name == 'rab_planes_ok':
        n, c, h, w, cm = args
        got = int(ops.get_conv_math() == 'bf16x3' and bool(lib.srhip_conv2d_pp_ok(n, h, w, c, cm)) and bool(lib.srhip_conv2d_pp_ok(n, h, w, cm, c))
                  and bool(lib.srhip_conv2d_wgrad_pp_ok(n, h, w, c, cm) & 4) and bool(lib.srhip_conv2d_wgrad_pp_ok(n, h, w, cm, c) & 4))
    elif name == 'pool_epilogue_ok':
        cin, cout, k = args
        got = int(ops.get_conv_math() == 'bf16x3' and k == 3 and cout == 64 and cin % 32 == 0)
    else:
        got = getattr(lib, name)(*args)
    return {'==': got == want, '>=': got >= want}[cmp], got
