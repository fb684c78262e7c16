"""srhip_debug_set is one table of key -> knob: exactly the live keys are accepted, everything else -- the retired numbers
2, 6, 8, 9, 13, 15, 16 (holes in the table, never reused) and everything outside 0..19 -- is an argument error.
Each key is set to its default value, so the library's state is what it was.  Needs the built library, no device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# defaults of the knobs behind the live keys (csrc/conv_dev.h names them; each is defined in the file that owns it)
DEFAULTS = {0: 0, 1: 0, 3: 0, 4: 0, 5: 0, 7: 0, 10: 1, 11: 1, 12: 768, 14: 1, 17: 1, 18: 4, 19: 1}
RETIRED = [2, 6, 8, 9, 13, 15, 16]
assert sorted(list(DEFAULTS) + RETIRED) == list(range(20))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


@pytest.mark.parametrize('key', sorted(DEFAULTS))
def test_known_key_accepts_its_default(lib, key):
    assert lib.srhip_debug_set(key, DEFAULTS[key]) == 0


@pytest.mark.parametrize('key', [-1, 20] + RETIRED)
def test_unknown_key_is_an_argument_error(lib, key):
    assert lib.srhip_debug_set(key, 0) != 0


def test_key_1_and_no_other_key_reaches_the_wgrad_knob(lib):
    """A permuted table would still return 0 everywhere.  Key 1 is observable without a device: value 7 turns the row-tap
    weight gradient off, which srhip_conv2d_wgrad_multi_ok reports.  Every other live key set to 7 must leave that answer alone."""
    shape = (8, 54, 54, 64, 256, 3, 3, 1, 1)
    math = lib.srhip_get_conv_math()
    try:
        assert lib.srhip_set_conv_math(1) == 0
        assert lib.srhip_conv2d_wgrad_multi_ok(*shape) >= 2
        for key in sorted(DEFAULTS):
            assert lib.srhip_debug_set(key, 7) == 0
            assert (lib.srhip_conv2d_wgrad_multi_ok(*shape) == 0) == (key == 1), key
            assert lib.srhip_debug_set(key, DEFAULTS[key]) == 0
        assert lib.srhip_conv2d_wgrad_multi_ok(*shape) >= 2
    finally:
        for key in DEFAULTS:
            lib.srhip_debug_set(key, DEFAULTS[key])
        lib.srhip_set_conv_math(math)


def test_srhip_debug_with_a_retired_key_fails_loudly_at_load(lib):
    """SRHIP_DEBUG=key:value is applied when the library loads (no GPU call): a key the table refuses must stop the process and be
    named, not drop out of an A/B run in silence.  A child process, because this one has the library loaded already."""
    def load(setting):
        return subprocess.run([sys.executable, '-c', 'from sradsgan_amd import _hip; _hip.lib()'], cwd=ROOT,
                              env=dict(os.environ, SRHIP_DEBUG=setting), capture_output=True, text=True, timeout=300)
    bad = load('9:1')
    assert bad.returncode != 0
    assert 'HipLibraryError' in bad.stderr and 'key 9' in bad.stderr, bad.stderr
    good = load('10:1')
    assert good.returncode == 0, good.stderr
