"""cn_conv2d_route on the host: every case of tests/conv_route_cases.py is routed as the table says, the table
reaches every route and every variant, and over the grid of tests/golden/gen_conv_queries.py the new query agrees
with the four older ones.  No GPU: the pointers are fabricated aligned addresses, which the query never reads."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from centernet_amd import native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_route_cases as cc   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = ctypes.c_size_t(-1).value


@pytest.fixture(autouse=True)
def _default_tuning():
    native.lib().cn_reset_tuning()
    yield
    native.lib().cn_reset_tuning()


def _ask(c):
    p = cc.fake_pointers(c)
    return cc.query(c, p["x"], p["w"], p["scale"], p["shift"], p["res"], p["y"], p["ws"], p["ws_bytes"])


def test_constants_are_the_headers():
    header = open(os.path.join(ROOT, "include", "centernet_amd.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define CN_(\w+) (0x[0-9a-fA-F]+|\d+)\b", header)}
    names = [n for n in defs if n.startswith(("ROUTE_", "STEM_", "C3_")) and n not in ("STEM_F32S", "STEM_MAXPOOL",
                                                                                       "STEM_Y_F32S")]
    assert len(names) == 11 + 5 + 8, sorted(names)      # (8: CN_C3_HREG, the fused heads' register form)
    for n in names:
        assert getattr(native, n) == defs[n], n
    assert [native.conv_route_name(defs["ROUTE_" + n.upper()]) for n in native.CONV_ROUTE_NAMES] == \
        list(native.CONV_ROUTE_NAMES)
    assert re.search(r"#define CN_C3_PREFETCH\(v\) \(\(\(v\) >> 12\) & 3\)", header)
    assert native.c3_prefetch(cc.pf(3) | cc.T) == 3
    fields = re.search(r"typedef struct cn_conv_route_info \{(.*?)\} cn_conv_route_info;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert fields == [n for n, _ in native.ConvRouteInfo._fields_]
    lib = native.lib()
    assert len(lib.cn_conv2d_route.argtypes) == len(lib.cn_conv2d.argtypes) + 1


@pytest.mark.parametrize("cid", [c["id"] for c in cc.CASES])
def test_the_query_says_what_the_table_says(cid):
    c = cc.BY_ID[cid]
    rc, info = _ask(c)
    assert cc.said(rc, info) == cc.expected(c), (cc.variant_name(native.conv_route_name(info.route), info.variant),
                                                 info.want, info.grid_x, info.grid_y)
    need = cc.workspace_bytes(c)
    if rc != cc.OK:
        # a refused descriptor: the workspace query answers 0, and *info is zero
        assert need == 0 and (info.want, info.grid_x, info.grid_y) == (0, 0, 0)
        return
    ho, wo = cc.out_hw(c)
    assert need == (info.want * c["B"] * ho * wo * cc.r32(c["Cout"]) * 4 if info.want > 1 else 0)
    assert info.ksplit in (1, info.want) and (info.ksplit == 1 or c["ws"])
    if c["route"] in ("stem", "offconv") or (c["route"] == "halo" and c["variant"] != native.C3_PERSIST):
        assert info.grid_x >= 1 and info.grid_y >= 1
    # host-only also means: the null and alignment checks of cn_conv2d, nothing else from the pointers
    p = cc.fake_pointers(c)
    d, i2 = cc.desc(c), native.ConvRouteInfo()
    lib, vp = native.lib(), ctypes.c_void_p
    args = [vp(p[k]) for k in ("x", "w", "scale", "shift", "res", "y", "ws")] + [p["ws_bytes"], None]
    with native.tuning(c["keys"]):
        assert lib.cn_conv2d_route(ctypes.byref(d), None, *args[1:], ctypes.byref(i2)) == -5
        assert lib.cn_conv2d_route(ctypes.byref(d), *args, None) == -5
        assert lib.cn_conv2d_route(ctypes.byref(d), vp(p["x"] + 4), *args[1:], ctypes.byref(i2)) == -6


def test_the_table_reaches_every_route_and_every_variant():
    by_route = {}
    for c in cc.CASES:
        by_route.setdefault(c["route"], []).append(c)
    assert set(by_route) == set(native.CONV_ROUTE_NAMES)
    assert {c["variant"] for c in by_route["stem"]} == {native.STEM_WINDOW, native.STEM_PERSIST,
                                                        native.STEM_PERSIST_F32S, native.STEM_16S}
    assert {c["variant"] for c in by_route["offconv"]} == {1, 2}
    assert {c["ksplit"] for c in by_route["offconv"]} == {1, 2, 3}
    halo = by_route["halo"]
    assert any(c["variant"] == native.C3_PERSIST for c in halo)
    tiles = [c for c in halo if c["variant"] & native.C3_TILE]
    assert len(tiles) + sum(c["variant"] == native.C3_PERSIST for c in halo) == len(halo)
    for dt in (cc.F32, cc.F16, cc.F32S):
        mine = [c for c in tiles if c["dt"] == dt]
        assert {c["n_tile"] for c in mine} == {32, 64, 128}, dt
        assert {c["m_tile"] for c in mine} == {128, 256}, dt
        for bit in (native.C3_TW32, native.C3_WAVES8):
            assert {bool(c["variant"] & bit) for c in mine} == {False, True}, (dt, bit)
    f32 = [c for c in tiles if c["dt"] == cc.F32]
    for bit in (native.C3_OCC4, native.C3_KSKIP):
        assert {bool(c["variant"] & bit) for c in f32} == {False, True}, bit
        assert not any(c["variant"] & bit for c in tiles if c["dt"] != cc.F32)
    f32s = [c for c in tiles if c["dt"] == cc.F32S]
    assert {bool(c["variant"] & native.C3_WREG) for c in f32s} == {False, True}
    assert {native.c3_prefetch(c["variant"]) for c in f32s if not c["variant"] & native.C3_WREG} == {1, 2, 3}
    assert not any(c["variant"] >> 8 for c in tiles if c["dt"] != cc.F32S)
    # the 256-pixel tiles in both wave counts
    assert {bool(c["variant"] & native.C3_WAVES8) for c in f32s if c["m_tile"] == 256} == {False, True}
    gemm = by_route["igemm"]
    assert {(c["m_tile"], c["n_tile"]) for c in gemm} == {(128, 32), (128, 64), (64, 128), (128, 128)}
    assert any(c["ksplit"] > 1 for c in gemm) and any(c["nchw"] for c in gemm) and any(c["stem"] for c in gemm)
    for dt in (cc.F32, cc.F16, cc.F32S):
        assert any(c["ksplit"] > 1 and c["dt"] == dt for c in gemm), dt
    # every test key of the routes is flipped by some case
    keys = set()
    for c in cc.CASES:
        keys |= set(c["keys"].items())
    assert {(28, 2), (28, 0), (14, 1), (14, 2), (14, 3), (15, 0), (19, 1), (39, 0), (40, 1), (46, 0), (33, 0), (65, 0),
            (6, 1), (10, 1), (12, 0), (27, 0), (20, 0), (21, 1), (21, 2), (21, 4), (4, 128)} <= keys


def test_the_pool_case_is_the_smallest_batch_the_kernel_takes():
    lib = native.lib()
    c = dict(cc.POOL)
    first = None
    for B in range(1, c["B"] + 1):
        c["B"] = B
        if lib.cn_stem_maxpool_supported(ctypes.byref(cc.desc(c))):
            first = B
            break
    assert first == cc.POOL["B"]
    c["B"] = first - 1
    p = cc.fake_pointers(c)
    rc, info = cc.query(c, p["x"], p["w"], p["scale"], p["shift"], None, p["y"], None, 0)
    assert (rc, info.route) == (cc.ERR_UNSUPPORTED, native.ROUTE_NONE)     # the flag is refused, not dropped


def test_a_scattered_call_is_never_split():
    """The first stage of a K split stores the partial row of tile row r at rowoff[r], the OUTPUT pixel's index
    (b*OH + oy*oy_mul + oy_add)*OW + ox*ox_mul + ox_add; the second stage reads row m = (b*Ho + oy)*Wo + ox.  The
    two are the same number for the identity scatter only.  The arithmetic for the 8 x 8 grid with oy_mul = ox_mul =
    2 into a 16 x 16 map: slabs of M = 64 rows, but rows up to 238 are written (behind the slab, and for the last
    slab behind the workspace) and 48 of the 64 rows the reduction sums were written by nobody."""
    B, Ho, Wo, OH, OW = 1, 8, 8, 16, 16
    m = np.arange(B * Ho * Wo)
    b, oy, ox = m // (Ho * Wo), m % (Ho * Wo) // Wo, m % Wo
    rowoff = (b * OH + oy * 2 + 0) * OW + ox * 2 + 0
    M = m.size
    assert rowoff.max() == 238 >= M and np.intersect1d(rowoff, m).size == 16 and (rowoff != m).sum() == 63
    # ... so conv_route plans no split there, with or without a workspace, and the identity scatter still does
    for c in cc.CASES:
        if c["id"].startswith("scatter"):
            rc, info = _ask(c)
            plain = c["scatter"] is None
            assert rc == cc.OK and (info.want > 1) == plain and (info.ksplit > 1) == plain, c["id"]
            assert (cc.workspace_bytes(c) > 0) == plain


# ---- the grid of the four older queries ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    path = os.path.join(ROOT, "tests", "golden", "gen_conv_queries.py")
    spec = importlib.util.spec_from_file_location("gen_conv_queries", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _conv16_shape(d):
    plain2 = (d.flags & 3) == 3
    return (d.Cin == 16 and d.Cout <= 32 and (d.KH, d.KW, d.pad_h, d.pad_w, d.dil) == (3, 3, 1, 1, 1) and
            d.in_layout == native.LAYOUT_NHWC and d.out_layout == native.LAYOUT_NHWC and
            (d.dtype == native.DTYPE_F32 or (d.dtype == native.DTYPE_F32S and plain2)))


@pytest.mark.parametrize("knobs", [{}, {5: 1}, {6: 1}, {10: 1}, {12: 0}, {27: 0}, {65: 0}, {28: 2}],
                         ids=lambda k: "-".join("k%d=%d" % kv for kv in k.items()) or "default")
def test_the_query_agrees_with_the_four_older_ones(gen, knobs):
    lib, vp = native.lib(), ctypes.c_void_p
    X, W, S, R, Y, WS = (vp(0x7000_0000_0000 + (i << 36)) for i in range(6))
    info = native.ConvRouteInfo()

    def route(d, res=None, ws=None, ws_bytes=0, flags=None):
        keep = d.flags
        d.flags = keep if flags is None else flags
        rc = lib.cn_conv2d_route(ctypes.byref(d), X, W, S, S, res, Y, ws, ws_bytes, None, ctypes.byref(info))
        d.flags = keep
        return rc, info.route, info.variant, info.want
    seen = {"ws": 0, "pool": 0, "f32s": 0, "c16h": 0, "res": 0}
    with native.tuning(knobs):
        for d in gen.descriptors():
            ref = ctypes.byref(d)
            rc, r, v, want = route(d)
            M = d.B * d.Ho * d.Wo
            need = int(lib.cn_conv2d_workspace_bytes(ref))
            if rc == cc.OK:
                assert need == (want * M * cc.r32(d.Cout) * 4 if want > 1 else 0)
            else:     # what no kernel takes (R_NONE) may still have a split planned; what conv_fill refuses has not
                assert rc == cc.ERR_UNSUPPORTED
            seen["ws"] += need > 0
            pool = route(d, flags=d.flags | native.CONV_STEM_F32S | native.CONV_STEM_MAXPOOL)
            assert bool(lib.cn_stem_maxpool_supported(ref)) == (pool[1] == native.ROUTE_STEM_POOL)
            seen["pool"] += pool[1] == native.ROUTE_STEM_POOL
            s = route(d, flags=d.flags | native.CONV_STEM_F32S)
            f32s = s[1] == native.ROUTE_STEM_POOL or (s[1] == native.ROUTE_STEM and
                                                      s[2] in (native.STEM_PERSIST_F32S, native.STEM_16S))
            assert bool(lib.cn_stem_f32s_supported(ref)) == f32s
            seen["f32s"] += f32s
            assert bool(lib.cn_conv16_f16_supported(ref)) == (r == native.ROUTE_CONV16H)
            seen["c16h"] += r == native.ROUTE_CONV16H
            rr = route(d, res=R, ws=WS, ws_bytes=SIZE_MAX)
            halo = rr[1] == native.ROUTE_HALO and not _conv16_shape(d)
            assert bool(lib.cn_conv2d_res_pitch_supported(ref)) == halo, [getattr(d, f) for f, _ in d._fields_[:-1]]
            seen["res"] += halo
    assert bool(seen["res"]) == (knobs != {10: 1}) and bool(seen["ws"]) == (knobs != {5: 1})
    assert seen["pool"] and seen["f32s"]
    assert bool(seen["c16h"]) == (knobs not in ({65: 0}, {10: 1}))
