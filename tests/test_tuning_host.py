"""cn_set_tuning / cn_get_tuning / cn_reset_tuning and native.tuning, without a GPU: which (key, value)
pairs the library accepts, every key's default, and that the header documents exactly the accepted keys.

EXPECTED is written out here on purpose, independent of the table in csrc/cn_tuning.h: it is the set the
library accepted before the knobs moved into that table (a sweep of keys -1 ... 64 over the values below:
43 keys, 17 414 accepted pairs) and the initialisers the knobs had, plus key 47 (1 ... 64: 44 keys, 17 478 pairs)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -2      # CN_ERR_UNSUPPORTED
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
VALUES = list(range(-2, 4100)) + [65535, 65536, 999999, 1000000, 1000001, INT_MAX, INT_MIN]
KEYS = range(-1, 65)


def _r(lo, hi):
    return set(range(lo, hi + 1))


# key: (accepted values, default); the retired keys 3 and 11 read back 0
EXPECTED = {
    1: (_r(0, 2), 0), 2: ({0, 1}, 0), 3: ({0, 64}, 0), 4: ({0, 64, 128}, 0), 5: ({0, 1}, 0), 6: ({0, 1}, 0),
    7: (_r(0, 2), 0), 8: ({0, 1}, 1), 9: (_r(0, 2047), 0), 10: ({0, 1}, 0), 11: ({0}, 0), 12: ({0, 1}, 1),
    13: ({0, 1, 3, 9}, 0), 14: (_r(0, 3), 0), 15: ({0, 1}, 1), 16: (_r(1, 64), 8), 17: (_r(1, 64), 16),
    18: (_r(0, 255), 100), 19: (_r(0, 2), 0), 20: ({0, 1}, 1), 21: (_r(0, 7), 0), 22: ({0, 1}, 1),
    23: (_r(0, 2) | _r(4, 7), 0), 24: (_r(0, 3), 1), 26: (_r(0, 3), 1), 27: ({0, 1}, 1), 28: (_r(0, 7), 1),
    29: (_r(0, 255), 0), 30: (_r(0, 255), 2), 31: ({0, 1}, 1), 32: ({0, 1}, 1), 33: ({0, 1}, 1), 36: (_r(0, 3), 3),
    37: (_r(1, 4096), 512), 38: (_r(0, 1024), 32), 39: ({0, 1}, 1), 40: (_r(0, 1000000), 768), 41: ({0, 1}, 1),
    42: (_r(1, 4096), 256), 43: (_r(0, 31), 0), 44: (_r(0, 1024), 0), 45: ({0, 1}, 1), 46: ({0, 1}, 1),
    47: (_r(1, 64), 64),
}
RETIRED = (3, 11)


@pytest.fixture
def lib():
    from centernet_amd import native
    l = native.lib()
    assert l.cn_reset_tuning() == 0
    yield l
    l.cn_reset_tuning()


def _get(lib, key):
    v = ctypes.c_int(-12345)
    assert lib.cn_get_tuning(key, ctypes.byref(v)) == 0, key
    return v.value


def test_version():
    from centernet_amd import native
    assert native.lib().cn_version() == 313


def test_accepted_pairs_are_exactly_the_recorded_ones(lib):
    assert len(EXPECTED) == 44
    swept = set(VALUES)
    want = {(k, v) for k, (vals, _) in EXPECTED.items() for v in vals & swept}
    assert len(want) == 17478
    got = set()
    for key in KEYS:
        for value in VALUES:
            rc = lib.cn_set_tuning(key, value)
            assert rc in (0, UNSUPPORTED), (key, value, rc)
            if rc == 0:
                got.add((key, value))
    assert got == want, (sorted(got - want)[:10], sorted(want - got)[:10])


def test_reset_restores_every_default(lib):
    for key, (vals, default) in EXPECTED.items():
        assert _get(lib, key) == default, key
        assert lib.cn_set_tuning(key, max(vals)) == 0
        assert lib.cn_set_tuning(key, min(vals)) == 0
    assert lib.cn_reset_tuning() == 0
    for key, (_, default) in EXPECTED.items():
        assert _get(lib, key) == default, key


def test_set_then_get_round_trips_and_a_refused_set_changes_nothing(lib):
    for key, (vals, default) in EXPECTED.items():
        for value in (min(vals), max(vals)):
            assert lib.cn_set_tuning(key, value) == 0, (key, value)
            assert _get(lib, key) == (0 if key in RETIRED else value), (key, value)
            for bad in (min(vals) - 1, max(vals) + 1, INT_MAX, INT_MIN):
                assert lib.cn_set_tuning(key, bad) == UNSUPPORTED, (key, bad)
                assert _get(lib, key) == (0 if key in RETIRED else value), (key, bad)
    assert lib.cn_set_tuning(23, 3) == UNSUPPORTED and lib.cn_set_tuning(13, 2) == UNSUPPORTED


def test_unknown_keys_cannot_be_read(lib):
    v = ctypes.c_int(7)
    for key in (0, 25, 34, 35, 48):
        assert lib.cn_get_tuning(key, ctypes.byref(v)) == UNSUPPORTED, key
        assert v.value == 7


def test_tuning_context_restores_on_exit_and_on_exception(lib):
    from centernet_amd import native
    lib.cn_set_tuning(30, 7)                      # not the default: the context restores what it FOUND
    with native.tuning({30: 0, 23: 5, 37: 4096}):
        assert (_get(lib, 30), _get(lib, 23), _get(lib, 37)) == (0, 5, 4096)
        with native.tuning({23: 2}):
            assert _get(lib, 23) == 2
        assert _get(lib, 23) == 5
    assert (_get(lib, 30), _get(lib, 23), _get(lib, 37)) == (7, 0, 512)
    with pytest.raises(ZeroDivisionError):
        with native.tuning({13: 9, 28: 0}):
            assert (_get(lib, 13), _get(lib, 28)) == (9, 0)
            1 / 0
    assert (_get(lib, 13), _get(lib, 28)) == (0, 1)
    # a refused value raises, and the keys set before it are put back
    with pytest.raises(native.NativeError):
        with native.tuning({13: 9, 23: 3}):
            pytest.fail("the block must not run")
    assert (_get(lib, 13), _get(lib, 23)) == (0, 0)
    with pytest.raises(native.NativeError):
        with native.tuning({25: 0}):
            pytest.fail("the block must not run")


def test_key_27_switches_the_f32s_stem_of_the_dla_base_layer(lib):
    """One effect that shows without a GPU: cn_stem_f32s_supported on DLA's base layer (B = 32, 3 x 512 x 512
    NCHW -> 16 channels NHWC, 7x7 / stride 1 / pad 3, CN_CONV_STEM_F32S) answers 1, with key 27 = 0 it
    answers 0, and 1 again after the context."""
    from centernet_amd import native
    from centernet_amd.native import ConvDesc, LAYOUT_NCHW, LAYOUT_NHWC, DTYPE_F32, CONV_STEM_F32S
    d = ConvDesc(B=32, H=512, W=512, Cin=3, Ho=512, Wo=512, Cout=16, KH=7, KW=7, stride=1, pad_h=3, pad_w=3,
                 dil=1, in_layout=LAYOUT_NCHW, in_pitch=3, out_layout=LAYOUT_NHWC, out_pitch=16, OH=512, OW=512,
                 oy_mul=1, oy_add=0, ox_mul=1, ox_add=0, relu=1, dtype=DTYPE_F32, flags=CONV_STEM_F32S)
    assert lib.cn_stem_f32s_supported(ctypes.byref(d)) == 1
    with native.tuning({27: 0}):
        assert lib.cn_stem_f32s_supported(ctypes.byref(d)) == 0
    assert lib.cn_stem_f32s_supported(ctypes.byref(d)) == 1


def test_header_documents_exactly_the_accepted_keys(lib):
    src = open(os.path.join(ROOT, "include", "centernet_amd.h")).read()
    end = src.index("int cn_set_tuning(")
    block = src[src.rindex("/*", 0, end):end]
    assert block.rstrip().endswith("*/") and "THREADING" in block
    documented = {int(k) for k in re.findall(r"\bkey (\d+)\b", block)}
    accepted = {k for k in KEYS if any(lib.cn_set_tuning(k, v) == 0 for v in (0, 1, 64))}
    assert accepted == set(EXPECTED)
    assert documented == accepted, (sorted(documented - accepted), sorted(accepted - documented))
