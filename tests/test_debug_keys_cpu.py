"""srhip_debug_set is one table of key -> knob: every key 0..19 is accepted, everything outside is an argument error.
Each key is set to its default value, so the library's state is what it was.  Needs the built library, no device."""
import os

import pytest

# defaults of the knobs behind the keys (csrc/conv_dev.h names them; each is defined in the file that owns it)
DEFAULTS = {k: 0 for k in range(20)}
DEFAULTS.update({8: 1, 10: 1, 11: 1, 12: 768, 14: 1, 17: 1, 18: 4, 19: 1})


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


@pytest.mark.parametrize('key', range(20))
def test_known_key_accepts_its_default(lib, key):
    assert lib.srhip_debug_set(key, DEFAULTS[key]) == 0


@pytest.mark.parametrize('key', [-1, 20])
def test_unknown_key_is_an_argument_error(lib, key):
    assert lib.srhip_debug_set(key, 0) != 0


def test_key_1_and_no_other_key_reaches_the_wgrad_knob(lib):
    """A permuted table would still return 0 everywhere.  Key 1 is observable without a device: value 7 turns the row-tap
    weight gradient off, which srhip_conv2d_wgrad_multi_ok reports.  Every other key set to 7 must leave that answer alone."""
    shape = (8, 54, 54, 64, 256, 3, 3, 1, 1)
    math = lib.srhip_get_conv_math()
    try:
        assert lib.srhip_set_conv_math(1) == 0
        assert lib.srhip_conv2d_wgrad_multi_ok(*shape) >= 2
        for key in range(20):
            assert lib.srhip_debug_set(key, 7) == 0
            assert (lib.srhip_conv2d_wgrad_multi_ok(*shape) == 0) == (key == 1), key
            assert lib.srhip_debug_set(key, DEFAULTS[key]) == 0
        assert lib.srhip_conv2d_wgrad_multi_ok(*shape) >= 2
    finally:
        for key in range(20):
            lib.srhip_debug_set(key, DEFAULTS[key])
        lib.srhip_set_conv_math(math)
