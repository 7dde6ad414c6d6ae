"""The half forms dla_34 needs, as far as they show without a GPU: the three new symbols, the route query
cn_conv16_f16_supported (a host function of the descriptor and the tuning keys), and the A1 exactness condition
of every case of tests/half_dla_cases.py on its float64 reference."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_cases as hc        # noqa: E402
import half_dla_cases as dc    # noqa: E402


@pytest.fixture
def lib():
    from centernet_amd import native
    l = native.lib()
    assert l.cn_reset_tuning() == 0
    yield l
    l.cn_reset_tuning()


def test_new_symbols_are_exported_and_bound(lib):
    for name in ("cn_dw_conv_transpose_f16", "cn_copy_channels_f16", "cn_conv16_f16_supported"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    assert len(lib.cn_dw_conv_transpose_f16.argtypes) == 10
    assert len(lib.cn_copy_channels_f16.argtypes) == 7
    assert len(lib.cn_conv16_f16_supported.argtypes) == 1


def _desc(Cout, s, W, dtype=None, flags=0):
    from centernet_amd import native
    c = dict(B=1, Cin=16, H=4 * s, W=W, Cout=Cout, k=3, s=s, p=1, relu=True, out_pitch=Cout)
    d = dc.conv_desc(c, native.DTYPE_F16 if dtype is None else dtype)
    d.flags = flags
    return d


YES = [(16, 1, 128), (32, 2, 256), (24, 1, 128)]


@pytest.mark.parametrize("Cout, s, W", YES)
def test_conv16_f16_supported(lib, Cout, s, W):
    from centernet_amd import native
    q = lambda d: lib.cn_conv16_f16_supported(ctypes.byref(d))
    assert q(_desc(Cout, s, W)) == 1
    assert q(_desc(Cout, s, W - 32 * s)) == 0                 # Wo = 96 + ..: not a multiple of 128
    assert q(_desc(Cout, s, W + 64 * s)) == 0
    assert q(_desc(48, s, W)) == 0
    assert q(_desc(Cout, s, W, native.DTYPE_F32)) == 0
    assert q(_desc(Cout, s, W, native.DTYPE_F32S, native.CONV_X_PLAIN | native.CONV_Y_PLAIN)) == 0
    # CN_CONV_Y_PLAIN with halves: y is plain fp32 at a pitch in floats -- not this form's store
    assert q(_desc(Cout, s, W, flags=native.CONV_Y_PLAIN)) == 0
    with native.tuning({dc.KEY: 0}):
        assert q(_desc(Cout, s, W)) == 0
    with native.tuning({10: 1}):              # everything on the implicit GEMM: this form as well
        assert q(_desc(Cout, s, W)) == 0
    assert q(_desc(Cout, s, W)) == 1
    assert lib.cn_conv16_f16_supported(None) == 0


def test_the_key_is_a_knob_with_default_one(lib):
    v = ctypes.c_int(-1)
    assert lib.cn_get_tuning(dc.KEY, ctypes.byref(v)) == 0 and v.value == 1
    assert lib.cn_set_tuning(dc.KEY, 2) != 0 and lib.cn_set_tuning(dc.KEY, -1) != 0
    assert lib.cn_set_tuning(dc.KEY, 0) == 0
    assert lib.cn_reset_tuning() == 0
    assert lib.cn_get_tuning(dc.KEY, ctypes.byref(v)) == 0 and v.value == 1


def test_every_conv16_case_is_one_the_query_accepts(lib):
    from centernet_amd import native
    for c in dc.CONV16:
        assert lib.cn_conv16_f16_supported(ctypes.byref(dc.conv_desc(c, native.DTYPE_F16))) == 1, c["id"]
    y = dc.conv_desc(dc.YPLAIN_CONV, native.DTYPE_F16, native.CONV_Y_PLAIN)
    assert lib.cn_conv16_f16_supported(ctypes.byref(y)) == 0


@pytest.mark.parametrize("cid", [c["id"] for c in dc.CONV16 + dc.OTHER_CONV])
def test_integer_conv_case_reference_is_exact_and_dense(cid):
    d = dc.int_case(cid)
    ok, top, nonzero = hc.exactness(d["ref"])
    print("%s: max |y| %.1f, non-zero %.3f" % (cid, top, nonzero))
    assert ok, (cid, top)
    assert nonzero >= 0.9, (cid, nonzero)
    for name in ("x", "w", "res", "bias"):
        t = d[name]
        if t is not None:
            assert torch.equal(t.half().float(), t) and torch.equal(t, t.round()), name


@pytest.mark.parametrize("run", dc.DW_RUNS, ids=dc.DW_IDS)
def test_integer_dw_case_reference_is_exact(run):
    shape, with_add = run
    d = dc.dw_int_case(shape, with_add)
    assert dc.dw_exact(d, shape[4]), (shape, float(d["mag"].max()))
    nonzero = float((d["ref"] != 0).double().mean())
    print("%s: max |y| %.1f, max sum |terms| %.1f, non-zero %.3f" % (
        shape, float(d["ref"].abs().max()), float(d["mag"].max()), nonzero))
    assert nonzero >= 0.9
