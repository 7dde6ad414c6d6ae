"""Case table of the fused heads cn_heads3x3_1x1: one call per row and what the host-only query cn_heads3x3_1x1_route
must say of it.  Shared by tests/test_deconv_heads_route_cases_host.py (no GPU) and
tests/test_gpu_deconv_heads_route.py (the same query with the real pointers, then the call against a float64
reference).  Not a test module.

The expectations were read off cn_heads3x3_1x1 (csrc/cn_conv3x3.hip) and cn_heads3x3p_takes (csrc/cn_conv3x3p.hip):
the persistent kernel for f32s tensors, head_conv = 64, every head <= 96 outputs with its w_frag given and enough
items; else, f32s at W >= 32 with key 26 set and every head <= 96 outputs, the form that keeps the hidden layer in
registers (CN_C3_HREG; from two slices on, or key 26 = 3); else the LDS form, 8 x 16 or 4 x 32 pixel tiles, its
weight prefetch one tap deep from two slices on.  n_tile is the width of a hidden slice, the grid (B * tiles,
n_heads) unless key 24 bit 0 folds the heads into grid_x (more than one head, B * tiles a multiple of 8).

Shapes: B 1..3, maps at most 20 x 33, Cin 8 / 40 / 96; larger only where the persistent kernel starts (256 items)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script: the list of cases per instantiation)
    sys.path.insert(0, ROOT)

from centernet_amd import native   # noqa: E402
from centernet_amd.native import (C3_HREG, C3_PERSIST, C3_TILE, C3_TW32, CONV_X_PLAIN, DTYPE_F32,   # noqa: E402
                                  DTYPE_F32S)

OK, ERR_UNSUPPORTED = 0, -2
F32, F32S = "f32", "f32s"
DTYPES = {F32: DTYPE_F32, F32S: DTYPE_F32S}
XP = CONV_X_PLAIN
T = C3_TILE


def pf(taps):
    return taps << 12


def r32(c):
    return (c + 31) // 32 * 32


def _c(id, variant=0, n_tile=0, grid=None, *, shape, hc=64, couts=(3, 2), dt=F32, flags=0, keys=None, in_pitch=None,
       frag=None, bias2=None, oscale=True, bias1=True, rc=OK, exact=False):
    """shape = (B, Cin, H, W); hc: head_conv; couts: outputs per head; frag: None = no w_frag, True = every head's,
    "misaligned" = given 8 bytes off; bias2: which heads have a bias (None: all); oscale: the 1x1 rows pre-scaled and
    undone by oscale, False = a null oscale; bias1: False = a null bias1; grid: (grid_x, grid_y) the query must say"""
    B, Cin, H, W = shape
    couts = tuple(couts)
    return dict(id=id, rc=rc, variant=variant, n_tile=n_tile, m_tile=128 if variant & T else 0, grid=grid, B=B,
                Cin=Cin, H=H, W=W, hc=hc, couts=couts, dt=dt, flags=flags, keys=dict(keys or {}), in_pitch=in_pitch,
                frag=frag, bias2=tuple(bias2) if bias2 else (True,) * len(couts), oscale=oscale, bias1=bias1,
                exact=exact)


P28 = {28: 2}
W32 = C3_TW32
CASES = [
    # ---- fp32: {TW 16 (W = 12), TW 32 (W = 33)} x {one slice, head_conv 128 and 256} --------------------------------
    _c("f32_w12_hc64", T, 64, (4, 2), shape=(2, 8, 9, 12), exact=True),
    _c("f32_w12_hc128", T, 64, shape=(1, 40, 9, 12), hc=128, couts=(5, 1)),
    _c("f32_w12_hc256", T, 64, shape=(1, 8, 5, 12), hc=256, couts=(96,)),
    _c("f32_w33_hc64", T | W32, 64, shape=(1, 40, 5, 33), couts=(33, 2, 1)),
    _c("f32_w33_hc128", T | W32, 64, shape=(1, 8, 9, 33), hc=128),
    _c("f32_w33_hc256", T | W32, 64, shape=(1, 40, 5, 33), hc=256, couts=(2, 65)),
    # ---- f32s, LDS form: the same, packed and plain input (W = 33 from two slices on: key 26 = 0) -------------------
    _c("f32s_w12_hc64", T | pf(3), 64, shape=(2, 8, 9, 12), dt=F32S, exact=True),
    _c("f32s_w12_hc128", T | pf(1), 64, shape=(1, 40, 9, 12), dt=F32S, hc=128, couts=(5, 1)),
    _c("f32s_w12_hc256", T | pf(1), 64, shape=(1, 8, 5, 12), dt=F32S, hc=256, couts=(96,)),
    _c("f32s_w33_hc64", T | W32 | pf(3), 64, shape=(1, 40, 5, 33), dt=F32S, couts=(33, 2, 1)),
    _c("f32s_w33_hc128_key26_0", T | W32 | pf(1), 64, shape=(1, 8, 9, 33), dt=F32S, hc=128, keys={26: 0}),
    _c("f32s_w33_hc256_key26_0", T | W32 | pf(1), 64, shape=(1, 40, 5, 33), dt=F32S, hc=256, couts=(2, 65),
       keys={26: 0}),
    _c("f32s_xplain_w12_hc64", T | pf(3), 64, shape=(1, 40, 9, 12), dt=F32S, flags=XP),
    _c("f32s_xplain_w12_hc128", T | pf(1), 64, shape=(1, 8, 9, 12), dt=F32S, flags=XP, hc=128),
    _c("f32s_xplain_w33_hc64", T | W32 | pf(3), 64, shape=(1, 8, 5, 33), dt=F32S, flags=XP),
    _c("f32s_xplain_w33_hc192_key26_0", T | W32 | pf(1), 64, shape=(1, 40, 5, 33), dt=F32S, flags=XP, hc=192,
       keys={26: 0}),
    # ---- f32s, hidden layer in registers ----------------------------------------------------------------------------
    _c("reg_hc128", T | W32 | C3_HREG | pf(1), 64, shape=(1, 40, 5, 33), dt=F32S, hc=128, couts=(33, 2), exact=True),
    _c("reg_hc256", T | W32 | C3_HREG | pf(1), 64, shape=(2, 8, 9, 33), dt=F32S, hc=256, couts=(96, 1)),
    _c("reg_hc64_key26_3", T | W32 | C3_HREG | pf(1), 64, shape=(1, 40, 9, 33), dt=F32S, keys={26: 3}),
    _c("reg_hc128_key26_2", T | W32 | C3_HREG | pf(1), 128, shape=(1, 8, 5, 33), dt=F32S, hc=128, keys={26: 2}),
    _c("reg_hc256_key26_2", T | W32 | C3_HREG | pf(1), 128, shape=(1, 40, 9, 33), dt=F32S, hc=256, couts=(65, 2),
       keys={26: 2}),
    _c("reg_hc192_key26_2", T | W32 | C3_HREG | pf(1), 64, shape=(1, 8, 5, 33), dt=F32S, hc=192, keys={26: 2}),
    _c("reg_xplain_hc128", T | W32 | C3_HREG | pf(1), 64, shape=(1, 8, 5, 33), dt=F32S, hc=128, flags=XP),
    # the same request at W = 20 says "LDS form, TW 16"; a head of 97 outputs says "LDS form"
    _c("reg_refused_w20", T | pf(1), 64, shape=(1, 40, 5, 20), dt=F32S, hc=128, couts=(33, 2)),
    _c("reg_refused_cout97", T | W32 | pf(3), 64, shape=(1, 8, 5, 33), dt=F32S, couts=(97, 2), keys={26: 3}),
    # ---- persistent kernel (key 28 = 2) -----------------------------------------------------------------------------
    _c("persist_one_head_of_1", C3_PERSIST, shape=(1, 8, 9, 17), dt=F32S, couts=(1,), keys=P28, frag=True),
    _c("persist_five_heads", C3_PERSIST, shape=(1, 40, 9, 17), dt=F32S, couts=(33, 96, 1, 64, 5), keys=P28,
       frag=True, bias2=(True, False, True, True, True), exact=True),
    _c("persist_ci96", C3_PERSIST, shape=(2, 96, 5, 15), dt=F32S, keys=P28, frag=True),
    _c("persist_ci40_pitch64", C3_PERSIST, shape=(1, 40, 9, 17), dt=F32S, keys=P28, frag=True, in_pitch=64),
    _c("persist_20x24", C3_PERSIST, shape=(1, 8, 20, 24), dt=F32S, couts=(80, 2, 2), keys=P28, frag=True),
    _c("persist_m32", C3_PERSIST, shape=(1, 8, 9, 17), dt=F32S, keys={28: 2, 30: 6}, frag=True),
    _c("persist_no_oscale_no_bias1", C3_PERSIST, shape=(1, 8, 9, 17), dt=F32S, keys=P28, frag=True, oscale=False,
       bias1=False),
    # by the library's own rule (key 28 = 1): B * ceil(H/8) * ceil(W/16) * n_heads >= 256
    _c("persist_by_rule", C3_PERSIST, shape=(2, 8, 57, 49), dt=F32S, couts=(3, 2, 1, 2), frag=True),
    _c("persist_by_rule_below", T | W32 | pf(3), 64, shape=(2, 8, 56, 49), dt=F32S, couts=(3, 2, 1, 2), frag=True),
    # each refusal says "tile"
    _c("persist_refused_key31_0", T | pf(3), 64, shape=(1, 8, 9, 17), dt=F32S, keys={28: 2, 31: 0}, frag=True),
    _c("persist_refused_no_frag", T | pf(3), 64, shape=(1, 8, 9, 17), dt=F32S, keys=P28),
    _c("persist_refused_frag_misaligned", T | pf(3), 64, shape=(1, 8, 9, 17), dt=F32S, keys=P28, frag="misaligned"),
    _c("persist_refused_cout97", T | pf(3), 64, shape=(1, 8, 9, 17), dt=F32S, couts=(97, 2), keys=P28, frag=True),
    _c("persist_refused_hc128", T | pf(1), 64, shape=(1, 8, 9, 17), dt=F32S, hc=128, keys=P28, frag=True),
    _c("persist_refused_xplain", T | pf(3), 64, shape=(1, 8, 9, 17), dt=F32S, flags=XP, keys=P28, frag=True),
    _c("refused_nine_heads", rc=ERR_UNSUPPORTED, shape=(1, 8, 9, 17), dt=F32S, couts=(1,) * 9, keys=P28, frag=True),
    # ---- more than 96 outputs at head_conv 64: two passes of the 1x1 ------------------------------------------------
    _c("two_pass_f32_w12_co130", T, 64, shape=(1, 8, 9, 12), couts=(130, 2), exact=True),
    _c("two_pass_f32_w33_co130", T | W32, 64, shape=(1, 8, 5, 33), couts=(2, 130)),
    _c("two_pass_f32s_w12_co130", T | pf(3), 64, shape=(1, 40, 9, 12), dt=F32S, couts=(130, 2)),
    _c("two_pass_f32s_w33_co130", T | W32 | pf(3), 64, shape=(1, 8, 5, 33), dt=F32S, couts=(130,)),
    _c("refused_hc128_cout97_f32", rc=ERR_UNSUPPORTED, shape=(1, 8, 9, 12), hc=128, couts=(97, 2)),
    _c("refused_hc128_cout97_f32s", rc=ERR_UNSUPPORTED, shape=(1, 8, 5, 33), dt=F32S, hc=128, couts=(2, 97)),
    # ---- key 24 bit 0: the heads folded into grid_x where B * tiles is a multiple of 8 -----------------------------
    _c("remap_on_grid8", T | W32, 64, (16, 1), shape=(1, 8, 13, 33)),
    _c("remap_off_grid8", T | W32, 64, (8, 2), shape=(1, 8, 13, 33), keys={24: 0}),
    _c("remap_on_grid6", T | W32, 64, (6, 2), shape=(1, 8, 9, 33)),
    _c("remap_off_grid6", T | W32, 64, (6, 2), shape=(1, 8, 9, 33), keys={24: 2}),
    _c("remap_on_grid8_f32s_reg", T | W32 | C3_HREG | pf(1), 64, (24, 1), shape=(1, 8, 13, 33), dt=F32S, hc=128,
       couts=(3, 2, 1)),
    _c("remap_on_one_head", T | W32, 64, (8, 1), shape=(1, 8, 13, 33), couts=(3,)),
    # ---- the optional pointers --------------------------------------------------------------------------------------
    _c("null_oscale_f32", T, 64, shape=(1, 8, 9, 12), oscale=False),
    _c("null_oscale_f32s", T | pf(3), 64, shape=(1, 8, 9, 12), dt=F32S, oscale=False),
    _c("null_bias1_f32", T, 64, shape=(1, 8, 9, 12), bias1=False, bias2=(False, True)),
    _c("null_bias1_f32s_reg", T | W32 | C3_HREG | pf(1), 64, shape=(1, 8, 5, 33), dt=F32S, hc=128, bias1=False,
       bias2=(True, False)),
]

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# every instantiation cn_heads3x3_1x1 and cn_heads3x3p can launch
INSTANTIATIONS = (["lds<%s,TW%d,%s>" % (dt, tw, s) for dt in (F32, F32S) for tw in (16, 32)
                   for s in ("one_slice", "slices")] +
                  ["reg<f32s,TW32,BN64>", "reg<f32s,TW32,BN128>", "persist<m16x16x32>", "persist<m32x32x16>"])


def instantiation(c):
    if c["rc"] != OK:
        return None
    if c["variant"] == C3_PERSIST:
        return "persist<%s>" % ("m32x32x16" if c["keys"].get(30, 2) & 4 else "m16x16x32")
    if c["variant"] & C3_HREG:
        return "reg<f32s,TW32,BN%d>" % c["n_tile"]
    return "lds<%s,TW%d,%s>" % (c["dt"], 32 if c["variant"] & C3_TW32 else 16,
                                "one_slice" if c["hc"] == 64 else "slices")


# ---- the arguments of a case -----------------------------------------------------------------------------------------
def packed_in(c):
    return c["dt"] == F32S and not c["flags"] & XP


def in_pitch(c):
    return c["in_pitch"] or (r32(c["Cin"]) if packed_in(c) else c["Cin"])


def head_array(c, w, bias, y, oscale, w_frag):
    """cn_head_out[]: lists of addresses per head (bias / oscale / w_frag entries may be None)"""
    arr = (native.HeadOut * len(c["couts"]))()
    for h, co in enumerate(c["couts"]):
        arr[h].w, arr[h].bias, arr[h].y, arr[h].cout = w[h], bias[h], y[h], co
        arr[h].oscale, arr[h].w_frag = oscale[h], w_frag[h]
    return arr


def args(c, x, w1, scale1, bias1, arr, ctl=None):
    """the argument list of cn_heads3x3_1x1 (without the stream)"""
    vp = ctypes.c_void_p
    return [vp(x), c["B"], c["H"], c["W"], c["Cin"], in_pitch(c), vp(w1), vp(scale1) if c["dt"] == F32S else None,
            vp(bias1) if c["bias1"] else None, c["hc"], len(c["couts"]), ctypes.cast(arr, vp), DTYPES[c["dt"]],
            c["flags"], ctl]


def query(c, x, w1, scale1, bias1, arr):
    info = native.ConvRouteInfo()
    with native.tuning(c["keys"]):
        rc = native.lib().cn_heads3x3_1x1_route(*args(c, x, w1, scale1, bias1, arr), None, ctypes.byref(info))
    return rc, info


def fake_heads(c):
    """cn_head_out[] of fabricated aligned addresses"""
    n = len(c["couts"])
    base = 0x7600_0000_0000
    frag = [None] * n
    if c["frag"]:
        frag = [base + 0x5000_0000 + (h << 20) + (8 if c["frag"] == "misaligned" else 0) for h in range(n)]
    return head_array(c, [base + (h << 20) for h in range(n)],
                      [base + 0x1000_0000 + (h << 20) if c["bias2"][h] else None for h in range(n)],
                      [base + 0x2000_0000 + (h << 24) for h in range(n)],
                      [base + 0x4000_0000 + (h << 20) if c["oscale"] else None for h in range(n)], frag)


def fake_pointers(c):
    return dict(x=0x7300_0000_0000, w1=0x7400_0000_0000, scale1=0x7500_0000_0000, bias1=0x7500_0001_0000)


def expected(c):
    return (c["rc"], "halo" if c["rc"] == OK else "none", c["variant"], c["n_tile"], c["m_tile"])


def said(rc, info):
    return (rc, native.conv_route_name(info.route), info.variant, info.n_tile, info.m_tile)


def tiles(c):
    """pixel tiles of the tile kernels: B * 8 x 16 tiles below W = 32, 4 x 32 tiles from there"""
    th, tw = (4, 32) if c["W"] >= 32 else (8, 16)
    return c["B"] * -(-c["H"] // th) * -(-c["W"] // tw)


def pins():
    """{instantiation: [case ids]}"""
    out = {n: [] for n in INSTANTIATIONS}
    for c in CASES:
        out.setdefault(instantiation(c) or "refused", []).append(c["id"])
    return out


if __name__ == "__main__":      # python tests/heads_route_cases.py: the list, per instantiation
    for name, ids in pins().items():
        print("%-24s %s" % (name, " ".join(ids) or "-- NONE --"))
