"""cn_conv_transpose4x4s2_route and cn_heads3x3_1x1_route on the host: every case of tests/deconv_route_cases.py and
tests/heads_route_cases.py is routed as its table says, and the tables reach every instantiation the ladders can
launch.  No GPU: the pointers are fabricated aligned addresses, which the queries never read."""
import ctypes
import os
import re
import sys

import pytest

from centernet_amd import native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_route_cases as dc   # noqa: E402
import heads_route_cases as hc    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "centernet_amd", "csrc")


@pytest.fixture(autouse=True)
def _default_tuning():
    native.lib().cn_reset_tuning()
    yield
    native.lib().cn_reset_tuning()


def _ask_deconv(c):
    p = dc.fake_pointers(c)
    return dc.query(c, p["x"], p["w"], p["scale"], p["shift"], p["y"])


def _ask_heads(c):
    p = hc.fake_pointers(c)
    return hc.query(c, p["x"], p["w1"], p["scale1"], p["bias1"], hc.fake_heads(c))


def test_constants_are_the_headers():
    header = open(os.path.join(ROOT, "include", "centernet_amd.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define CN_(\w+) (0x[0-9a-fA-F]+|\d+)\b", header)}
    c3 = [n for n in defs if n.startswith("C3_")]
    assert len(c3) == 8 and "C3_HREG" in c3, sorted(c3)
    for n in c3:
        assert getattr(native, n) == defs[n], n
    # a new bit is documented below the existing ones and collides with none of them (nor with the prefetch field)
    assert header.index("#define CN_C3_HREG") > header.index("#define CN_C3_PREFETCH")
    bits = [defs[n] for n in c3 if n not in ("C3_PERSIST", "C3_TILE")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 and not b & (3 << 12) and b >= 0x10 for b in bits)
    lib = native.lib()
    assert len(lib.cn_conv_transpose4x4s2_route.argtypes) == len(lib.cn_conv_transpose4x4s2.argtypes) + 1
    assert len(lib.cn_heads3x3_1x1_route.argtypes) == len(lib.cn_heads3x3_1x1.argtypes) + 1
    for name in ("cn_conv_transpose4x4s2", "cn_heads3x3_1x1"):
        flat = re.sub(r"\s+", " ", header)
        call = re.search(r"int %s\((.*?)\);" % name, flat).group(1)
        route = re.search(r"int %s_route\((.*?)\);" % name, flat).group(1)
        assert route == call + ", cn_conv_route_info *info", name
    for status, value in (("OK", dc.OK), ("ERR_UNSUPPORTED", dc.ERR_UNSUPPORTED), ("ERR_ALIGN", dc.ERR_ALIGN)):
        assert int(re.search(r"CN_%s\s*=\s*(-?\d+)" % status, header).group(1)) == value


# ---- the deconvolution ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in dc.CASES])
def test_the_deconvolution_query_says_what_the_table_says(cid):
    c = dc.BY_ID[cid]
    rc, info = _ask_deconv(c)
    assert dc.said(rc, info) == dc.expected(c), (info.variant, info.grid_x, info.grid_y)
    if rc != dc.OK:
        assert (info.ksplit, info.want, info.grid_x, info.grid_y) == (0, 0, 0, 0)
        return
    assert (info.ksplit, info.want) == (1, 1)
    if c["variant"] & dc.T:
        th, tw = (4, 32) if c["variant"] & native.C3_TW32 else (8, 16)
        assert (c["W"] >= 32) == bool(c["variant"] & native.C3_TW32)
        assert info.grid_x == c["B"] * -(-c["H"] // th) * -(-c["W"] // tw)
        assert info.grid_y == -(-c["Cout"] // c["n_tile"])
    else:
        assert (info.grid_x, info.grid_y) == (0, 0)
    # host-only: the null and alignment checks of the call, nothing else from the pointers
    p = dc.fake_pointers(c)
    lib, i2 = native.lib(), native.ConvRouteInfo()
    a = dc.args(c, p["x"], p["w"], p["scale"], p["shift"], p["y"])
    with native.tuning(c["keys"]):
        assert lib.cn_conv_transpose4x4s2_route(None, *a[1:], None, ctypes.byref(i2)) == -5
        assert lib.cn_conv_transpose4x4s2_route(*a, None, None) == -5
        assert lib.cn_conv_transpose4x4s2_route(ctypes.c_void_p(p["x"] + 4), *a[1:], None, ctypes.byref(i2)) == -6


def test_the_deconvolution_table_reaches_every_instantiation():
    # the instantiations, from the ladders' own text: every launch_c3 / launch_c3_occ4 of cn_deconv4x4s2_halo ...
    src = open(os.path.join(CSRC, "cn_conv3x3.hip")).read()
    body = src[src.index("int cn_deconv4x4s2_halo("):]
    names = {"float": dc.F32, "cn_f32s": dc.F32S, "_Float16": dc.F16}
    ladder = set()
    for m in re.finditer(r"launch_c3<(\w+), (\d+), (\d+), \d, \d, false, 128, false, true", body):
        ladder.add("tile<%s,TW%s,BN%s>" % (names[m.group(1)], m.group(2), m.group(3)))
    for m in re.finditer(r"launch_c3_occ4<(\w+), (\d+), true>", body):
        ladder.add("occ4<%s,TW%s>" % (names[m.group(1)], m.group(2)))
    assert len(ladder) == 14, sorted(ladder)
    # ... the persistent kernel's output form x schedule x MFMA shape (P3_LAUNCH4 of cn_deconv4x4s2_persist) ...
    src = open(os.path.join(CSRC, "cn_conv3x3p.hip")).read()
    body = src[src.index("int cn_deconv4x4s2_persist("):src.index("bool cn_conv3x3s2p_takes(")]
    assert len(re.findall(r"P3_LAUNCH4\((true|false), (true|false)\);", body)) == 4 and "P3_S16_DECONV" in body
    ladder |= {"persist<%s,%s,%s>" % (o, p, m) for o in ("f32s_out", "plain_out") for p in ("pipe", "nopipe")
               for m in ("m16x16x32", "m32x32x16")}
    # ... and the implicit GEMM's class x dtype (igemm_dispatch<A_DENSE, false> of cn_conv.hip)
    ladder |= {"igemm_parity<%s,BN%d>" % (dt, bn) for dt in (dc.F32, dc.F32S, dc.F16) for bn in (32, 64, 128)}
    assert ladder == set(dc.INSTANTIATIONS)
    pins = dc.pins()
    for name in dc.INSTANTIATIONS:
        assert pins[name], "no case reaches %s" % name
    # every case names an instantiation of the list; the pitches are exercised on every route
    assert set(pins) - {"refused"} == set(dc.INSTANTIATIONS)
    for kind in ("tile<", "occ4<", "persist<", "igemm_parity<"):
        mine = [c for c in dc.CASES if (dc.instantiation(c) or "").startswith(kind)]
        assert any(c["in_pitch"] and c["in_pitch"] > (dc.r32(c["Cin"]) if dc.packed_in(c) else c["Cin"])
                   for c in mine), kind
        assert any(c["c_off"] == 32 and dc.pitches(c)[1] > c["Cout"] + 32 for c in mine), kind
        assert any(c["exact"] for c in mine), kind
    keys = set()
    for c in dc.CASES:
        keys |= set(c["keys"].items())
    assert {(10, 1), (19, 1), (19, 2), (28, 2), (28, 0), (32, 0), (30, 0), (30, 4), (30, 6)} <= keys


def test_the_occ4_case_is_the_smallest_batch_the_rule_takes():
    c = dict(dc.OCC4_RULE)
    first = None
    for B in range(1, c["B"] + 1):
        c["B"] = B
        rc, info = _ask_deconv(c)
        assert rc == dc.OK
        if info.variant & native.C3_OCC4:
            first = B
            break
    assert first == dc.OCC4_RULE["B"]
    assert 768 < 4 * info.grid_x <= 1024 and info.grid_y == 1


def test_the_persistent_deconvolution_starts_at_256_items():
    def items(c):
        return 4 * c["B"] * -(-c["H"] // 8) * -(-c["W"] // 16) * -(-c["Cout"] // 64)
    assert items(dc.BY_ID["persist_by_rule"]) == 256
    below = dc.BY_ID["persist_by_rule_below"]
    assert items(below) < 256 and below["W"] == dc.BY_ID["persist_by_rule"]["W"] - 1


# ---- the heads --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES])
def test_the_heads_query_says_what_the_table_says(cid):
    c = hc.BY_ID[cid]
    rc, info = _ask_heads(c)
    assert hc.said(rc, info) == hc.expected(c), (info.variant, info.grid_x, info.grid_y)
    if rc != hc.OK:
        assert (info.ksplit, info.want, info.grid_x, info.grid_y) == (0, 0, 0, 0)
        return
    assert (info.ksplit, info.want) == (1, 1)
    if c["variant"] & hc.T:
        n, nh = hc.tiles(c), len(c["couts"])
        assert (c["W"] >= 32) == bool(c["variant"] & native.C3_TW32)
        folded = nh > 1 and n % 8 == 0 and c["keys"].get(24, 1) & 1
        assert (info.grid_x, info.grid_y) == ((n * nh, 1) if folded else (n, nh))
        if c["grid"]:
            assert (info.grid_x, info.grid_y) == c["grid"]
    else:
        assert (info.grid_x, info.grid_y) == (0, 0)
    p = hc.fake_pointers(c)
    lib, i2 = native.lib(), native.ConvRouteInfo()
    arr = hc.fake_heads(c)
    a = hc.args(c, p["x"], p["w1"], p["scale1"], p["bias1"], arr)
    with native.tuning(c["keys"]):
        assert lib.cn_heads3x3_1x1_route(None, *a[1:], None, ctypes.byref(i2)) == -5
        assert lib.cn_heads3x3_1x1_route(*a, None, None) == -5
        assert lib.cn_heads3x3_1x1_route(ctypes.c_void_p(p["x"] + 4), *a[1:], None, ctypes.byref(i2)) == -6
        arr[len(c["couts"]) - 1].y = None
        assert lib.cn_heads3x3_1x1_route(*a, None, ctypes.byref(i2)) == -5


def test_the_heads_table_reaches_every_instantiation():
    src = open(os.path.join(CSRC, "cn_conv3x3.hip")).read()
    body = src[src.index("static int heads_run("):src.index('extern "C" int cn_heads3x3_1x1(')]
    names = {"float": hc.F32, "cn_f32s": hc.F32S}
    ladder = set()
    for m in re.finditer(r"launch_c3<(\w+), (\d+), (\d+), (\d), (\d), true(, 128, false, false, 2, 1)?>", body):
        dt, tw, bn, wm, wn, deep = m.groups()
        if (wm, wn) == ("4", "1"):
            ladder.add("reg<%s,TW%s,BN%s>" % (names[dt], tw, bn))
        else:
            assert (wm, wn, bn) == ("2", "2", "64")
            ladder.add("lds<%s,TW%s,%s>" % (names[dt], tw, "slices" if deep else "one_slice"))
    assert len(ladder) == 10, sorted(ladder)
    src = open(os.path.join(CSRC, "cn_conv3x3p.hip")).read()
    body = src[src.index("int cn_heads3x3p("):src.index("// ---- 1x1 matrix of a head")]
    assert "P3_LAUNCHH(P3_S16_HEADS); else P3_LAUNCHH(false);" in body
    ladder |= {"persist<m16x16x32>", "persist<m32x32x16>"}
    assert ladder == set(hc.INSTANTIATIONS)
    pins = hc.pins()
    for name in hc.INSTANTIATIONS:
        assert pins[name], "no case reaches %s" % name
    assert set(pins) - {"refused"} == set(hc.INSTANTIATIONS)
    for kind in ("lds<", "reg<", "persist<"):
        assert any(c["exact"] for c in hc.CASES if (hc.instantiation(c) or "").startswith(kind)), kind
    keys = set()
    for c in hc.CASES:
        keys |= set(c["keys"].items())
    assert {(26, 0), (26, 2), (26, 3), (28, 2), (31, 0), (24, 0), (24, 2), (30, 6)} <= keys
    # the optional pointers, the second pass of the 1x1 on both tile shapes, the 1-D grid seen and not seen
    assert any(not c["oscale"] for c in hc.CASES) and any(not c["bias1"] for c in hc.CASES)
    assert any(not all(c["bias2"]) for c in hc.CASES)
    for tw32 in (0, native.C3_TW32):
        assert any(max(c["couts"]) > 96 and c["variant"] & hc.T and (c["variant"] & native.C3_TW32) == tw32
                   for c in hc.CASES if c["rc"] == hc.OK)
    assert {c["grid"][1] == 1 for c in hc.CASES if c["grid"] and len(c["couts"]) > 1} == {False, True}


def test_the_persistent_heads_start_at_256_items():
    def items(c):
        return c["B"] * -(-c["H"] // 8) * -(-c["W"] // 16) * len(c["couts"])
    assert items(hc.BY_ID["persist_by_rule"]) == 256
    below = hc.BY_ID["persist_by_rule_below"]
    assert items(below) < 256 and below["H"] == hc.BY_ID["persist_by_rule"]["H"] - 1

