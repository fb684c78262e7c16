"""CPU-side checks of the attention ablations: tests/attn_variants_ref.py's fp64 forward against the oracle's modules and against
attn_tail_ref for the default, the first-index rule on ties, the margins of every GPU case, the state_dict layout of the HIP modules
against the oracle and the reference's record, the oracle against tests/golden/gen_ablation.npz (tools/make_golden_ablation.py), the
trainer's validation of the five switches, and the new entry points' argument checks (no GPU needed: they refuse before any launch)."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import sradsgan_ref as O
from tests import attn_tail_ref as A
from tests import attn_variants_ref as V


def _oracle_tail(t, mode, pool, addconv):
    """A module carrying the oracle's tail for (mode, pool, addconv), fp64, with the case's weights."""
    mod = nn.Module()
    mod.la_mode, mod.addconv = mode, addconv
    O._attention_tail(mod, mode, pool, V.C, addconv)
    O.det_init_(mod, prefix='tail.')
    mod.double()
    with torch.no_grad():
        if 'CA' in mode:
            mod.ca.fc1.weight.copy_(t['fc1'].double().reshape(4, V.C, 1, 1))
            mod.ca.fc2.weight.copy_(t['fc2'].double().reshape(V.C, 4, 1, 1))
        if 'SA' in mode:
            mod.sa.conv1.weight.copy_(V.w7_of(t['w7'], pool).double())
    return mod


@pytest.mark.parametrize('variant', V.VARIANTS, ids=V.variant_id)
def test_forward_closed_forms_agree_with_the_oracle_modules(variant):
    mode, pool, addconv = variant
    t = V.case_inputs('normal', 3, 10, 12)
    mod = _oracle_tail(t, mode, pool, addconv)
    ref = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)
    with torch.no_grad():
        want = O._apply_attention_tail(mod, t['u'].double())
    got = ref['z']
    if hasattr(mod, 'conv'):
        got = torch.einsum('oc,bchw->bohw', mod.conv.weight.detach().reshape(V.C, -1), got) + mod.conv.bias.detach().view(1, V.C, 1, 1)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the backward at the reference's own first arg-maxes against fp64 autograd through the oracle's modules (no ties in this case)
    dz = V.case_dz(t, mode)
    mine = V.variant_grads(dz, t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)
    uu = t['u'].double().requires_grad_()
    if hasattr(mod, 'conv'):
        keep, mod.conv = mod.conv, nn.Identity()              # the gradient is stated at z, in front of the closing conv
        mod.addconv = True
    zz = O._apply_attention_tail(mod, uu)
    named = dict(mod.named_parameters())
    keys = [k for k in ('ca.fc1.weight', 'ca.fc2.weight', 'sa.conv1.weight') if k in named]
    gs = torch.autograd.grad(zz, [uu] + [named[k] for k in keys], dz.double())
    theirs = dict(zip(['du'] + keys, gs))
    pairs = [('du', 'du'), ('dfc1', 'ca.fc1.weight'), ('dfc2', 'ca.fc2.weight'), ('dw7', 'sa.conv1.weight')]
    for a, b in pairs:
        assert (mine[a] is None) == (b not in theirs), a
        if mine[a] is not None:
            d = float((mine[a].reshape(-1) - theirs[b].reshape(-1)).abs().max())
            assert d <= 1e-12 * max(1.0, float(theirs[b].abs().max())), (a, d)
    y64 = V.variant_torch(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool, torch.float64)
    for k in ('avg', 'mx', 's', 'pooled', 'm', 'z'):
        assert (ref[k] is None) == (y64[k] is None), k
        if ref[k] is not None:
            assert float((ref[k] - y64[k]).abs().max()) <= 1e-12, k


@pytest.mark.parametrize('case', [c for c in V.CASES if c[1:] == (3, 10, 12)], ids=V.case_id)
def test_default_variant_is_attn_tail_ref(case):
    t = V.case_inputs(*case)
    ref = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], 'CA-SA', 'Avg|Max')
    old = A.tail_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'])
    for k in ('avg', 'mx', 's', 'pooled', 'm', 'z'):
        assert float((ref[k] - old[k]).abs().max()) <= 1e-12, k
    assert torch.equal(ref['arg'], old['arg']) and torch.equal(ref['argc'], old['argc'])
    # the backward: autograd of the gather formulation against attn_tail_ref's closed forms (the ChanBwd / SpatBwd equations written
    # out), both at the first arg-maxes -- on the tie families too, where torch's own max would be free to pick another index
    mine = V.variant_grads(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], 'CA-SA', 'Avg|Max')
    for k, want in zip(('du', 'dfc1', 'dfc2', 'dw7'), A.tail_bwd_ref(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'])):
        d = float((mine[k] - want).abs().max())
        assert d <= 1e-12 * max(1.0, float(want.abs().max())), (k, d)


def test_ties_go_to_the_first_index():
    """pixel_ties: channel CONST_C is constant (pixel 0 wins) and TIE_C's maximum sits at two pixels (the earlier wins);
    channel_ties: the second channel of a bit-equal pair never wins -- in every configuration that pools the tied tensor."""
    t = V.case_inputs('pixel_ties', *V.TIE_SHAPE)
    p1, p2 = A.tie_pixels(V.TIE_SHAPE[1] * V.TIE_SHAPE[2])
    for mode in ('CA-SA', 'CA', 'CA|SA'):
        for pool in ('Max', 'Avg|Max'):
            arg = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)['arg']
            assert bool((arg[:, A.CONST_C] == 0).all()) and bool((arg[:, A.TIE_C] == p1).all()) and p1 < p2
    t = V.case_inputs('channel_ties', *V.TIE_SHAPE)
    for mode in ('CA-SA', 'SA-CA', 'SA', 'CA|SA'):
        for pool in ('Max', 'Avg|Max'):
            argc = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], mode, pool)['argc']
            won = 0
            for c1, c2 in A.CHANNEL_TIES:
                assert not bool((argc == c2).any())
                won += int((argc == c1).sum())
            assert won > 0                      # the tie is met at all


@pytest.mark.parametrize('pool', ['Max', 'Avg|Max'])
def test_ties_send_the_gradient_to_the_first_index(pool):
    """la_mode 'CA' on pixel_ties: du = s dz + [Avg] davg / hw + [p = arg] dmx, so r = du - s dz is one constant per channel but at the
    arg-max pixel.  At the SECOND tied pixel of TIE_C, and at every pixel > 0 of the constant channel, r is that constant (no dmx
    term); the first tied pixel and pixel 0 carry dmx -- which is not zero here, else the check would see nothing.  channel_ties
    under 'SA': the second channel of a tied pair gets no dpm term anywhere."""
    t = V.case_inputs('pixel_ties', *V.TIE_SHAPE)
    n, c, h, w = t['u'].shape
    p1, p2 = A.tie_pixels(h * w)
    f = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], 'CA', pool)
    du = V.variant_grads(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], 'CA', pool)['du'].reshape(n, c, h * w)
    r = du - f['s'][:, :, None] * t['dz'].double().reshape(n, c, h * w)
    for ch, first in ((A.TIE_C, p1), (A.CONST_C, 0)):
        others = [p for p in range(h * w) if p != first]
        base = r[:, ch, others[0]]
        assert float((r[:, ch, others] - base[:, None]).abs().max()) <= 1e-12            # p2 (and every other loser) carries no dmx
        assert float((r[:, ch, first] - base).abs().min()) > 1e-6                        # the winner does
    t = V.case_inputs('channel_ties', *V.TIE_SHAPE)
    f = V.variant_fwd_ref(t['u'], t['fc1'], t['fc2'], t['w7'], 'SA', pool)
    du = V.variant_grads(t['dz'], t['u'], t['fc1'], t['fc2'], t['w7'], 'SA', pool)['du'].reshape(n, c, h * w)
    r = du - f['m'][:, None, :] * t['dz'].double().reshape(n, c, h * w)                  # [Avg] dpa / 64 + [c = argc] dpm
    for c1, c2 in A.CHANNEL_TIES:
        won = f['argc'] == c1                                                            # pixels where the pair holds the maximum
        assert bool(won.any())
        loser = r[:, c2, :]
        plain = r[:, 0, :] if 0 not in (c1, c2) else r[:, 1, :]                          # a channel that is no arg-max there
        not_arg = won & (f['argc'] != 0)
        assert float((loser - plain)[not_arg].abs().max()) <= 1e-12
        assert float((r[:, c1, :] - plain)[not_arg].abs().min()) > 1e-9


@pytest.mark.parametrize('case', V.CASES, ids=V.case_id)
def test_every_gpu_case_keeps_its_margins(case):
    assert set(V.SEEDS) == set(V.CASES)
    t = V.case_inputs(*case)
    cm, pm, rm = V.case_margins(t)
    print('%s: channel %.3g pixel %.3g relu %.3g' % (V.case_id(case), cm, pm, rm))
    V.assert_margins(t, V.case_id(case))


def test_variant_list_is_the_21_combinations():
    assert len(V.VARIANTS) == len(set(V.VARIANTS)) == 21 and len(V.FORWARDS) == 15


def _layout(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


@pytest.mark.parametrize('variant', V.VARIANTS + [('', 'Avg|Max', True)], ids=V.variant_id)
def test_block_state_dicts_equal_the_oracles(variant):
    """RAB / ResGroup on the HIP path list the oracle's keys and shapes for every variant (a single-pool SLAM's conv1 is
    [1, 1, 7, 7]), and load its state dict strictly."""
    from sradsgan_amd import model as M
    mode, pool, addconv = variant
    for hip, ora in ((M.RAB(64, 64, la_mode=mode, pool_mode=pool, addconv=addconv), O.RAB(64, 64, la_mode=mode, pool_mode=pool, addconv=addconv)),
                     (M.ResGroup(M.RAB, n_blocks=1, rla_mode=mode, bla_mode=mode, pool_mode=pool, addconv=addconv),
                      O.ResGroup(O.RAB, n_blocks=1, rla_mode=mode, bla_mode=mode, pool_mode=pool, addconv=addconv))):
        assert _layout(hip) == _layout(ora)
        hip.load_state_dict(ora.state_dict(), strict=True)
    if 'SA' in mode and pool != 'Avg|Max':
        assert tuple(M.SLAM(7, pool).conv1.weight.shape) == (1, 1, 7, 7)


@pytest.mark.parametrize('ga_mode', ['', 'CA', 'SA', 'CA-SA', 'SA-CA', 'CA|SA'], ids=lambda m: m.replace('|', '+') or 'none')
@pytest.mark.parametrize('addconv', [True, False])
def test_gab_up_state_dicts_equal_the_oracles(ga_mode, addconv):
    from sradsgan_amd import model as M
    for scale in (2, 3):
        assert _layout(M.GAB_UP(ga_mode, addconv, scale)) == _layout(O.GAB_UP(ga_mode, addconv, scale))


@pytest.mark.parametrize('cfg', V.GEN_CONFIGS, ids=V.gen_tag)
def test_generator_layout_and_oracle_against_the_reference_record(cfg, golden):
    """tests/golden/gen_ablation.npz, written from the reference's own GeneratorResNet: the HIP generator and the oracle list its keys
    and shapes; the oracle reproduces its output and every parameter gradient."""
    from sradsgan_amd import model as M
    g, tag = golden('gen_ablation'), V.gen_tag(cfg)
    assert tag in list(g['configs'])
    recorded = list(zip(g[tag + '/keys'].tolist(), [tuple(int(x) for x in s.split(',') if x) for s in g[tag + '/shapes'].tolist()]))
    og = O.GeneratorResNet(O.ResGroup, **V.gen_kwargs(cfg))
    assert _layout(og) == recorded
    assert _layout(M.GeneratorResNet(M.ResGroup, **V.gen_kwargs(cfg))) == recorded
    y, og = V.gen_run(og, cfg)

    def check(name, got, want):
        assert got.shape == want.shape, name
        np.testing.assert_allclose(got, want, rtol=V.GEN_RTOL, atol=V.GEN_ATOL * max(1.0, float(np.abs(want).max())), err_msg=name)
    check('y', O.digest(y), g[tag + '/y'])
    n = 0
    for k, p in og.named_parameters():
        check(k, V.small_digest(p.grad), g[tag + '/grad/' + k])
        n += 1
    assert n == sum(1 for k in g.files if k.startswith(tag + '/grad/'))


def test_trainer_validates_the_ablation_switches():
    from sradsgan_amd import trainer as T
    ns = argparse.Namespace
    assert T.attention_ablation(ns()) == dict(rla_mode='CA-SA', bla_mode='CA-SA', ga_mode='CA-SA', pool_mode='Avg|Max', addconv=True)
    got = T.attention_ablation(ns(rla_mode='SA-CA', bla_mode='', ga_mode='CA|SA', pool_mode='Max', addconv=False))
    assert got == dict(rla_mode='SA-CA', bla_mode='', ga_mode='CA|SA', pool_mode='Max', addconv=False)
    for bad in (dict(rla_mode='SA|CA'), dict(bla_mode='SA|CA'), dict(ga_mode='SA|CA'), dict(pool_mode='Mean'), dict(pool_mode='Max|Avg'),
                dict(addconv=1)):
        with pytest.raises(ValueError):
            T.attention_ablation(ns(**bad))
    for cfg in V.GEN_CONFIGS:
        kw = V.gen_kwargs(cfg)
        assert T.attention_ablation(ns(**{k: kw[k] for k in ('rla_mode', 'bla_mode', 'ga_mode', 'pool_mode', 'addconv')}))


def test_modules_reject_an_unknown_pool_mode():
    from sradsgan_amd import model as M
    for bad in ('Mean', 'Max|Avg', ''):
        with pytest.raises(ValueError):
            M.CLAM(64, pool_mode=bad)
        with pytest.raises(ValueError):
            M.SLAM(7, pool_mode=bad)


def test_new_entry_points_are_declared_and_refuse_bad_arguments():
    """Header and ctypes table agree (tests/test_abi_cpu.py compares all of them); C != 64, hidden > 16, a bad order / pool set and a
    missing output return SRHIP_ERR_ARG with a message, before any launch -- so without a GPU."""
    from sradsgan_amd import _hip
    lib = _hip.lib()
    for name in ('srhip_attn_var_workspace', 'srhip_attn_var_fwd', 'srhip_attn_var_close', 'srhip_attn_var_bwd_workspace', 'srhip_attn_var_bwd'):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert lib.srhip_attn_var_workspace(3) == 3 * 32 * 64 * 3 * 4 and lib.srhip_attn_var_workspace(0) == 0
    one = 16                                   # a non-null, 16-byte aligned stand-in address: nothing may be dereferenced
    fwd = lambda **kw: lib.srhip_attn_var_fwd(*[kw.get(k, one) for k in ('u', 'fc1', 'fc2', 'w7', 'avg', 'mx', 'arg', 's', 'pooled', 'argc', 'm',
                                                                            'ws')], kw.get('ws_bytes', 1 << 30), 2, 3, 5, kw.get('c', 64),
                                              kw.get('hidden', 4), kw.get('order', 0), kw.get('pools', 3), None)
    for bad in (dict(c=32), dict(hidden=17), dict(hidden=0), dict(order=5), dict(order=-1), dict(pools=0), dict(pools=4), dict(u=None),
                dict(s=None), dict(m=None), dict(arg=None), dict(ws_bytes=16), dict(u=8)):
        assert fwd(**bad) == -1 and lib.srhip_last_error(), bad
    close = lambda **kw: lib.srhip_attn_var_close(one, kw.get('s', one), one, kw.get('skip', one), one, 2, 15, kw.get('c', 64),
                                                  kw.get('order', 0), kw.get('cat', 0), None)
    for bad in (dict(c=32), dict(order=7), dict(cat=1), dict(order=4, cat=0), dict(s=None), dict(skip=None)):
        assert close(**bad) == -1 and lib.srhip_last_error(), bad
    assert lib.srhip_attn_var_bwd_workspace(2, 3, 5, 4) == (2 * 32 * 64 + 2 * 2 * 64 + 3 * 2 * 15 + 2 * 2 * 4 * 64) * 4
    bwd = lambda **kw: lib.srhip_attn_var_bwd(*[kw.get(k, one) for k in ('dz', 'u', 's', 'm', 'avg', 'mx', 'arg', 'pooled', 'argc', 'w7', 'fc1',
                                                                            'fc2', 'du', 'dw7')], 0, kw.get('dfc1', one), one, 0, kw.get('ws', one),
                                              kw.get('ws_bytes', 1 << 30), 2, 3, 5, kw.get('c', 64), kw.get('hidden', 4), kw.get('order', 0),
                                              kw.get('pools', 3), None)
    for bad in (dict(c=32), dict(hidden=17), dict(order=5), dict(pools=0), dict(dz=None), dict(du=None), dict(s=None), dict(m=None),
                dict(argc=None), dict(dfc1=None), dict(dw7=None), dict(ws=None), dict(ws_bytes=64)):
        assert bwd(**bad) == -1 and lib.srhip_last_error(), bad
