"""tests/attn_kernels_ref.py without a GPU: its references agree with the ones the older GPU tests carry, every case of its tables
meets the condition that makes it worth running (asserted from the float64 reference's own scores), a correct fp32 implementation --
stock torch on the CPU -- is under every bar the GPU tests will hold, and the refusal lists return the argument (workspace) error with a
message that names the entry, on made-up addresses."""
import os

import pytest
import torch

from tests import attn_kernels_ref as A

F64, F32 = torch.float64, torch.float32


# --------------------------------------------------------------------------------------------- #
# the references against the existing ones
# --------------------------------------------------------------------------------------------- #


def _nchw(t, h, w):
    return t.view(t.shape[0], h, w, -1).permute(0, 3, 1, 2)


def test_cgam_and_sgam_references_agree_with_the_existing_ones():
    from tests.test_attention_gpu import _cgam_ref, _sgam_ref
    h, w = 5, 7
    inp = A.sgam_inputs('random', 2, h * w)
    got = A.sgam_eval(inp, F64)
    leaves = [_nchw(inp[k].double(), h, w).contiguous().requires_grad_() for k in ('x', 'q', 'k', 'v')] + [inp['gamma'].double().requires_grad_()]
    y = _sgam_ref(*leaves)
    y.backward(_nchw(inp['dy'].double(), h, w))
    assert torch.allclose(_nchw(got['y'], h, w), y.detach(), rtol=0, atol=1e-13)
    for name, leaf in zip(('dq', 'dk', 'dv'), leaves[1:4]):
        assert torch.allclose(_nchw(got[name], h, w), leaf.grad, rtol=0, atol=1e-13), name
    assert torch.allclose(got['dgamma'], leaves[4].grad, rtol=1e-12, atol=0)
    emu = A.sgam_split_emulation(inp)
    assert all(0 < A.err(emu[k], got[k]) < 3e-5 for k in ('y', 'o', 'dq', 'dk', 'dv', 'dgamma')) and A.err(emu['lse'], got['lse']) == 0
    inp = A.cgam_inputs(2, h * w, 0.3)
    got = A.cgam_eval(inp, F64)
    x, g = _nchw(inp['x'].double(), h, w).contiguous().requires_grad_(), inp['gamma'].double().requires_grad_()
    y = _cgam_ref(x, g)
    y.backward(_nchw(inp['dy'].double(), h, w))
    assert torch.allclose(_nchw(got['y'], h, w), y.detach(), rtol=0, atol=1e-13)
    assert torch.allclose(_nchw(got['dx'], h, w), x.grad, rtol=0, atol=1e-13)
    assert torch.allclose(got['dgamma'], g.grad, rtol=1e-12, atol=0)


@pytest.mark.parametrize('kind,ws,shift', [(0, 8, 0), (0, 9, 4), (1, 8, 0), (1, 9, 0)])
def test_window_attention_reference_agrees_with_the_existing_one(kind, ws, shift):
    from tests.test_hat_gpu import attn_ref64
    inp = A.hat_attn_inputs(('shared', kind, ws, shift, 2, 2 * ws, 3 * ws, 'random'))
    got = A.hat_attn_eval(inp, F64)
    qkv, table = inp['qkv'].double().permute(0, 3, 1, 2).contiguous().requires_grad_(), inp['table'].double().requires_grad_()
    o = attn_ref64(qkv, table, kind, ws, shift)
    (o * inp['dout'].double().permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(got['out'].permute(0, 3, 1, 2), o.detach())
    assert torch.allclose(got['dqkv'].permute(0, 3, 1, 2), qkv.grad, rtol=0, atol=1e-14)
    assert torch.allclose(got['dtable'], table.grad, rtol=0, atol=1e-12)
    # lse: exp(logit - lse) sums to 1 over the keys of every (pixel, head)
    a, _ = A.hat_attn_terms(inp['qkv'].double(), inp['table'].double(), kind, ws, shift)
    lse_w = torch.logsumexp(a, -1)
    assert torch.allclose(torch.exp(a - lse_w.unsqueeze(-1)).sum(-1), torch.ones_like(lse_w), rtol=0, atol=1e-12)
    # ... and it is placed like `out` (the same un-windowing, which attn_ref64 has just confirmed): a permutation of the windows' rows
    assert got['lse'].shape == (2, 2 * ws, 3 * ws, 6)
    assert torch.equal(got['lse'].reshape(-1).sort()[0], lse_w.reshape(-1).sort()[0])


def test_combine_reference_agrees_with_the_existing_formula():
    inp = A.ca_inputs(3, 18, 96, 3)
    got = A.ca_eval(inp, F64)
    import torch.nn.functional as F
    x6, a6, u6, g6 = (inp[k].double().view(3, 3, 6, 96).permute(0, 3, 1, 2) for k in ('x', 'a', 'u', 'g'))
    w1, w2 = inp['w1'].double().view(3, 96, 1, 1), inp['w2'].double().view(96, 3, 1, 1)
    s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(u6.mean((2, 3), keepdim=True), w1, inp['b1'].double())), w2, inp['b2'].double()))
    y = x6 + inp['kb'].double().view(-1, 1, 1, 1) * a6 + (u6 * s) * 0.01
    assert torch.allclose(got['out'].view(3, 3, 6, 96).permute(0, 3, 1, 2), y, rtol=0, atol=1e-14)
    assert torch.allclose(got['s'], s.view(3, 96), rtol=0, atol=1e-14)


def test_layer_norm_written_out_is_layer_norm():
    for family in A.LN_FAMILIES:
        inp = A.ln_inputs(family, 37)
        a, b = A.ln_eval(inp, F64, True), A.ln_eval(inp, F64, True, stock=False)
        assert all(A.err(b[k], a[k]) < 1e-11 for k in a), family


# --------------------------------------------------------------------------------------------- #
# the conditions of the case tables
# --------------------------------------------------------------------------------------------- #


def test_sgam_case_table_conditions():
    assert set(A.SGAM_HW) == {1, 31, 32, 33, 127, 128, 129, 257}
    n, hw = A.SGAM_BIG
    assert n * hw > 16384 and (n * hw + 15) // 16 > 1024 > 64
    assert (A.SGAM_FAMILY_HW + 31) // 32 == 5 and A.SHARP_KEY // 32 == 4 and A.SHARP_EARLY_KEY // 32 == 1
    s = A.sgam_scores(A.sgam_inputs('sharp', 2, A.SGAM_FAMILY_HW))
    row = s[:, A.SHARP_QUERY]
    rest = row.clone()
    rest[:, A.SHARP_KEY] = float('-inf')
    rest[:, A.SHARP_EARLY_KEY] = float('-inf')
    assert bool((row[:, A.SHARP_KEY] >= rest.amax(-1) + 100).all())
    assert bool((row[:, A.SHARP_EARLY_KEY] > rest.amax(-1)).all()) and bool((row[:, A.SHARP_EARLY_KEY] < row[:, A.SHARP_KEY]).all())
    running = torch.cummax(A.tile_maxima(row), -1)[0]
    assert bool((running[:, 1] > running[:, 0]).all()) and bool((running[:, 4] > running[:, 3]).all())       # rises after the first tile
    up = A.sgam_scores(A.sgam_inputs('ascending', 2, A.SGAM_FAMILY_HW))
    assert bool((up[..., 1:] - up[..., :-1] >= 0.05).all())
    tm = A.tile_maxima(up)
    assert bool((tm[..., 1:] > tm[..., :-1]).all())                                                          # every tile rescales
    down = A.sgam_scores(A.sgam_inputs('descending', 2, A.SGAM_FAMILY_HW))
    assert bool((down[..., :-1] - down[..., 1:] >= 0.05).all())
    tm = A.tile_maxima(down)
    assert bool((tm[..., :1] > tm[..., 1:]).all())                                                           # none after the first does


def test_cgam_case_table_conditions():
    assert {hw for _, hw, sc in A.CGAM_CASES if sc == 0.3} == {1, 15, 16, 17, 127, 128, 129, 257}
    x = A.cgam_inputs(2, 729, 1.0)['x'].double()
    e = x.transpose(1, 2) @ x
    assert float(e.amax()) > 200                                                                              # energies in the hundreds
    att = torch.softmax(e.max(-1, keepdim=True)[0] - e, -1)
    assert float(att.amax(-1).median()) > 0.5                                                                 # a sharp soft-max


def test_hat_case_table_conditions():
    wins = [A.hat_attn_windows(c) for c in A.HAT_ATTN_CASES]
    assert wins[:6] == [75] * 6 and sorted(wins[6:9]) == [64, 65, 128] and wins[9:] == [75] * 3
    assert {(c[1], c[2], c[3]) for c in A.HAT_ATTN_CASES[:6]} == {(0, 8, 0), (0, 8, 4), (1, 8, 0), (0, 9, 0), (0, 9, 4), (1, 9, 0)}
    assert all(c[7] in A.HAT_ATTN_UNCAPPED for c in A.HAT_ATTN_CASES[9:]) and all(c[7] == 'random' for c in A.HAT_ATTN_CASES[:9])
    by = {c[7]: A.hat_attn_inputs(c) for c in A.HAT_ATTN_CASES[9:]}
    logits = {f: A.hat_attn_terms(i['qkv'].double(), i['table'].double(), 0, 8, 0)[0] for f, i in by.items()}
    assert float(logits['x6'].abs().amax()) > 20                                                              # logits of tens
    assert bool((logits['ascending'][..., 1:] - logits['ascending'][..., :-1] >= 0.2).all())
    assert bool((logits['descending'][..., :-1] - logits['descending'][..., 1:] >= 0.2).all())
    assert max(A.LN_TOKENS) > 2048 and (2049 + 3) // 4 > 512 >= (2048 + 3) // 4 and (4099 + 3) // 4 > 2 * 512
    x = A.ln_inputs('constant_token', 323)['x']
    assert float(x[161].var()) == 0.0
    x = A.ln_inputs('mean_1000', 323)['x']
    assert bool((x.double().mean(1) == 1000).all()) and bool((x.max(1)[0] - x.min(1)[0] == 1).all()) and float(x.var(1).min()) > 0.03
    assert max(A.GELU_COUNTS) > 4194304 and max(A.GELU_COUNTS) // 4 == 4096 * 256 + 1
    x = A.gelu_inputs(1028)['x']
    assert float(x[~torch.isnan(x)].min()) == -12 and float(x[~torch.isnan(x)].max()) == 12 and int(torch.isnan(x).sum()) == 1
    assert bool(torch.signbit(x[1028 - 3])) and float(x[1028 - 3]) == 0.0 and float(x[1028 - 4]) == 0.0
    n, hw, c, hid = A.CA_BIG
    per, quads = hw * c // 4, n * hw * c // 4
    assert quads > 4096 * 256 and n * hw * c * 4 < 17 * 2 ** 20
    inp = A.ca_inputs(*A.CA_ZERO_UNIT, zero_unit=True)
    ref = A.ca_eval(inp, F64)
    assert float(ref['mz'][:, 96].abs().max()) == 0.0 and float(ref['dw1'][0].abs().max()) == 0.0 and float(ref['db1'][0]) == 0.0
    assert float(ref['dw1'][1:].abs().max()) > 0
    assert float(A.ca_inputs(3, 7, 4, 1)['kb'][1]) == 0.0


# --------------------------------------------------------------------------------------------- #
# a correct fp32 implementation meets every bar
# --------------------------------------------------------------------------------------------- #


def _under(label, table):
    bad = []
    for name, (b, e32, es) in table.items():
        print('%-44s %-8s fp32 %.3e  split %.3e  bar %.3e' % (label, name, e32, es, b))
        if not e32 <= b:
            bad.append((label, name, e32, b))
    return bad


def test_stock_fp32_meets_the_global_attention_bars():
    bad = []
    for family, n, hw in A.SGAM_CASES:
        if (n, hw) == A.SGAM_BIG:
            n = 2                                      # the same rule on two of its images; the GPU test evaluates all eighteen
        inp = A.sgam_inputs(family, n, hw)
        ref, t32, emu = A.sgam_eval(inp, F64), A.sgam_eval(inp, F32), A.sgam_split_emulation(inp)
        scales = A.sgam_scales(inp)
        zero = [k for k, v in ref.items() if float(v.abs().max()) == 0.0]
        assert zero == (['dq', 'dk'] if hw == 1 else []), (family, hw, zero)
        capped = family == 'random'
        bad += _under('sgam exact %s %dx%d' % (family, n, hw), A.bars(ref, t32, 'sgam', capped, None, scales))
        bad += _under('sgam split %s %dx%d' % (family, n, hw), A.bars(ref, t32, 'sgam', capped, emu, scales))
    for n, hw, scale in A.CGAM_CASES:
        inp = A.cgam_inputs(n, hw, scale)
        ref = A.cgam_eval(inp, F64)
        assert all(float(v.abs().max()) > 0 for v in ref.values())
        bad += _under('cgam %dx%d scale %.1f' % (n, hw, scale), A.bars(ref, A.cgam_eval(inp, F32), 'cgam'))
    assert not bad, bad


def test_stock_fp32_meets_the_hat_bars():
    bad = []
    for case in A.HAT_ATTN_CASES:
        inp = A.hat_attn_inputs(case)
        ref = A.hat_attn_eval(inp, F64)
        assert all(float(v.abs().max()) > 0 for v in ref.values())
        bad += _under('hat attn ' + case[0], A.bars(ref, A.hat_attn_eval(inp, F32), 'hat_attn', case[7] not in A.HAT_ATTN_UNCAPPED))
    for family, tokens in A.LN_CASES:
        inp = A.ln_inputs(family, tokens)
        for dadd in (False, True):
            bad += _under('hat ln %s %d dadd %d' % (family, tokens, dadd), A.bars(A.ln_eval(inp, F64, dadd), A.ln_eval(inp, F32, dadd), 'hat_ln'))
    for count in A.GELU_COUNTS[:2]:
        inp = A.gelu_inputs(count)
        ref, t32 = A.gelu_eval(inp, F64), A.gelu_eval(inp, F32)
        keep = ~torch.isnan(inp['x'])
        assert all(bool(torch.isnan(r[~keep]).all()) and bool(torch.isnan(t[~keep]).all()) for r, t in zip(ref.values(), t32.values()))
        bad += _under('hat gelu %d' % count, A.bars({k: v[keep] for k, v in ref.items()}, {k: v[keep] for k, v in t32.items()}, 'hat_gelu'))
    for c, hid in A.CA_DIMS:
        for n in A.CA_N:
            for hw in A.CA_HW:
                inp = A.ca_inputs(n, hw, c, hid)
                for bias in (True, False):
                    bad += _under('hat combine %dx%dx%d/%d bias %d' % (n, hw, c, hid, bias),
                                  A.bars(A.ca_eval(inp, F64, bias), A.ca_eval(inp, F32, bias), 'hat_combine'))
    assert not bad, bad


# --------------------------------------------------------------------------------------------- #
# argument refusals: the library, no device
# --------------------------------------------------------------------------------------------- #


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


FAKE = {k: 0x100000 + 0x10000 * i for i, k in enumerate('abcdefghijkl')}         # aligned, never dereferenced
FAKE.update(ws=0x4000000, ws_bytes=1 << 24)


def test_every_entry_point_refuses_bad_arguments(lib):
    calls = A.global_attn_refusals(lib, FAKE) + A.hat_refusals(lib, FAKE)
    assert len(calls) > 200
    entries = {label.split(':')[0] for label, _, _ in calls}
    assert entries == {'cgam_fwd', 'cgam_bwd', 'sgam_flash_fwd', 'sgam_flash_bwd', 'hat_ln_fwd', 'hat_ln_bwd', 'hat_gelu_fwd', 'hat_gelu_bwd',
                       'hat_attn_fwd', 'hat_attn_bwd', 'hat_ca_fwd', 'hat_combine_fwd', 'hat_combine_bwd'}
    for label, code, call in calls:
        lib.srhip_cbam_pool_hw(None, None, None, 0, 1, 1, 4, None)               # leaves a message of another entry behind
        entry = label.split(':')[0]
        rc = call()
        msg = lib.srhip_last_error()
        assert rc == code, (label, rc, msg)
        assert msg and entry.encode() in msg, (label, msg)
    assert {code for _, code, _ in calls} == {A.ERR_ARG, A.ERR_WORKSPACE}
    assert [lib.srhip_hat_ln_parts(t) for t in (0, 1, 5, 2048, 2049, 4099)] == [0, 1, 2, 512, 512, 512]
