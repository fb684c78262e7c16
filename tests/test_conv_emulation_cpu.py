"""The fp64 conv emulation (tests/conv_emulation.py) on the CPU: its roundings against torch's / numpy's, the split-bf16
reconstruction, its contractions against torch's conv in double, and a checker that catches one-tap-sized errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_emulation as E


def _awkward(n, seed):
    """fp32 values with every low significand bit in play, signed, across a wide exponent range, plus exact ties."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 12, (n,), generator=g).float())
    ties = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 1 + 2 ** -11, 1 + 3 * 2 ** -11, 2 ** -24, 3 * 2 ** -25,
                         65504.0, 2 ** -14, 2 ** -15 * 1.5, 0.0, -0.0])
    return torch.cat([v, ties])


def test_round_bf16_matches_torch():
    v = _awkward(200000, 1)
    assert torch.equal(E.round_bf16(v), v.to(torch.bfloat16).double())


def test_round_fp16_matches_numpy_with_gradual_underflow():
    v = _awkward(200000, 2)
    v = v[v.abs() < 65504]                                   # (overflow above 65504 is outside this helper)
    ref = torch.from_numpy(v.numpy().astype(np.float16).astype(np.float64))
    assert torch.equal(E.round_fp16(v), ref)
    assert torch.equal(E.round_fp16(v), v.to(torch.float16).double())
    sub = torch.tensor([2 ** -20, -3 * 2 ** -24, 2 ** -15])
    assert (E.round_fp16(sub) != 0).all() and (E.round_fp16(sub, flush_subnormals=True) == 0).all()


def test_split_bf16_reconstructs():
    v = _awkward(200000, 3)
    v = v[v != 0]
    hi, lo = E.split_bf16(v)
    assert torch.equal(hi, E.round_bf16(v))
    assert torch.equal(lo, E.round_bf16((v.double() - hi).float()))
    err = (hi + lo - v.double()).abs() / v.double().abs()
    assert float(err.max()) <= 2.0 ** -16                    # hi + lo holds 16 bits
    # lo is the rounded remainder, never dropped: the split is not bf16 alone
    assert float(((hi - v.double()).abs() / v.double().abs()).max()) > 2.0 ** -10


@pytest.mark.parametrize('stride,pad,dil,k', [(1, 1, 1, 3), (2, 1, 1, 3), (2, 1, 1, 4), (1, 2, 2, 3), (1, 0, 1, 1)])
def test_contractions_match_torch_double(stride, pad, dil, k):
    g = torch.Generator().manual_seed(stride * 100 + k)
    x = torch.randn(2, 5, 11, 9, generator=g).double()
    w = torch.randn(6, 5, k, k, generator=g).double()
    y = F.conv2d(x, w, None, stride, pad, dil)
    ref, absref = E.conv_fwd(x, w, stride, pad, 'fp32', dil)
    assert torch.allclose(ref, y, rtol=1e-12, atol=1e-12)
    assert torch.allclose(absref, F.conv2d(x.abs(), w.abs(), None, stride, pad, dil), rtol=1e-12, atol=1e-12)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    dy = torch.randn(y.shape, generator=g).double()
    F.conv2d(xr, wr, None, stride, pad, dil).backward(dy)
    assert torch.allclose(E.conv_dgrad(dy, w, tuple(x.shape), stride, pad, 'fp32', dil)[0], xr.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(E.conv_wgrad(x, dy, tuple(w.shape), stride, pad, 'fp32', dil)[0], wr.grad, rtol=1e-12, atol=1e-12)


def test_arithmetics_are_what_the_table_says():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 16, 6, 6, generator=g)
    w = torch.randn(8, 16, 3, 3, generator=g)
    ref = {a: E.conv_fwd(x, w, 1, 1, a)[0] for a in E.ARITHS}
    xh, xl = E.split_bf16(x)
    wh, wl = E.split_bf16(w)
    f = lambda a, b: F.conv2d(a, b, None, 1, 1)
    assert torch.allclose(ref['bf16x3'], f(xh, wh) + f(xh, wl) + f(xl, wh), rtol=0, atol=1e-12)
    assert torch.allclose(ref['fp16'], f(x.half().double(), w.half().double()), rtol=0, atol=1e-12)
    assert torch.allclose(ref['bf16'], f(x.bfloat16().double(), w.bfloat16().double()), rtol=0, atol=1e-12)


def test_checker_flags_one_dropped_tap():
    """An output element off by 1/K of its abs reference (one tap of K) fails; fp32-rounded results pass."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 32, 8, 8, generator=g)
    w = torch.randn(16, 32, 3, 3, generator=g)
    ref, absref = E.conv_fwd(x, w, 1, 1, 'fp32')
    tau = 16 * E.U24
    got = ref.float()
    assert E.assert_conv_close(got, ref, absref, tau) < 0.2
    K = 32 * 9
    bad = got.clone()
    bad[1, 5, 3, 4] += float(absref[1, 5, 3, 4]) / K
    with pytest.raises(AssertionError, match=r'image 1, channel 5, pixel \(3, 4\)'):
        E.assert_conv_close(bad, ref, absref, tau)
    # the same conv with its centre tap really dropped in column 0 (a tile-edge fault)
    y_drop = F.conv2d(x.double(), w.double(), None, 1, 1)
    y_drop[:, :, :, 0] -= F.conv2d(x.double(), w.double()[:, :, 1:2, 1:2])[:, :, :, 0]
    assert E.worst(y_drop.float(), ref, absref, tau)[0] > 20


def test_checker_discriminates_neighbouring_arithmetics():
    """The bound of one arithmetic rejects the neighbours' results at the route table's reduction lengths."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 64, 10, 10, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    refs = {a: E.conv_fwd(x, w, 1, 1, a) for a in E.ARITHS}
    tau = 4 * E.U24
    for a, b in [('bf16x3', 'fp32'), ('fp32', 'bf16x3'), ('fp16', 'bf16'), ('bf16', 'fp16'), ('bf16x3', 'bf16'), ('fp16', 'bf16x3')]:
        r = E.worst(refs[b][0].float(), refs[a][0], refs[a][1], tau)[0]
        assert r > 4, (a, b, r)
