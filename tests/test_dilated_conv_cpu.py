"""Host-side checks of the dilated 3x3 convolution and PReLU (ABI 14): the library's workspace query and argument checks, the
parameter containers' state_dict keys and the configurations they refuse.  No GPU call is made here."""
import os

import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


def test_dilated_workspace_query_and_argument_errors(lib):
    assert lib.srhip_abi_version() == 14
    sub = lambda c, d: 2 * d * d * (-(-13 // d)) * (-(-14 // d)) * c * 4          # n = 2, 13 x 14
    for d in (2, 3):
        assert lib.srhip_conv2d_dil_workspace(1, 2, 13, 14, 256, 64, d) >= sub(256, d) + sub(64, d)
        assert lib.srhip_conv2d_dil_workspace(2, 2, 13, 14, 256, 64, d) >= sub(256, d) + sub(64, d)
        assert lib.srhip_conv2d_dil_workspace(3, 2, 13, 14, 256, 64, d) >= sub(256, d) + sub(64, d) + 64 * 256 * 9 * 4
    assert lib.srhip_conv2d_dil_workspace(1, 2, 13, 14, 256, 64, 1) == 0
    assert lib.srhip_conv2d_dil_workspace(1, 2, 13, 14, 256, 64, 4) == 0                 # dilation 4: not served
    rc = lib.srhip_conv2d_fwd_dil(None, None, None, None, None, None, 0, 1, 4, 4, 4, 4, 2, 4, 4, 0.0, 0, None)
    assert rc == -1 and b'null tensor' in lib.srhip_last_error()
    assert lib.srhip_prelu_parts() > 0
    rc = lib.srhip_prelu_fwd(None, 4, None, 4, None, 1, 4, None)
    assert rc == -1 and b'prelu_fwd' in lib.srhip_last_error()


def test_containers_keep_keys_and_refuse_what_they_do_not_run():
    from sradsgan_amd import ops
    from sradsgan_amd.model.layers import HipConv2d, HipDilatedConv2d, HipPReLU
    for d in (1, 2, 3):
        m, r = HipDilatedConv2d(256, 256, 3, padding=d, dilation=d), torch.nn.Conv2d(256, 256, 3, padding=d, dilation=d)
        assert {k: v.shape for k, v in m.state_dict().items()} == {k: v.shape for k, v in r.state_dict().items()}
    p = HipPReLU()
    assert list(p.state_dict()) == ['weight'] and float(p.weight.detach()) == 0.25
    for kw in [dict(padding=1, dilation=2), dict(padding=4, dilation=4), dict(padding=2, dilation=2, stride=2),
               dict(padding=(2, 3), dilation=(2, 3))]:
        with pytest.raises(NotImplementedError):
            HipDilatedConv2d(8, 8, 3, **kw)
    with pytest.raises(NotImplementedError):
        HipConv2d(8, 8, 3, padding=2, dilation=2)                  # the plain container keeps refusing dilation
    with pytest.raises(NotImplementedError):
        HipPReLU(8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.conv2d_dil(torch.zeros(1, 8, 4, 4), torch.zeros(8, 8, 3, 3), None, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.prelu(torch.zeros(1, 8, 4, 4), torch.zeros(1))
