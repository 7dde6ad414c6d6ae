"""Case table of cn_conv_transpose4x4s2: one call per row and what the host-only query cn_conv_transpose4x4s2_route
must say of it.  Shared by tests/test_deconv_heads_route_cases_host.py (no GPU: fabricated aligned addresses) and
tests/test_gpu_deconv_heads_route.py (the same query with the real pointers, then the call against a float64
reference).  Not a test module.

The expectations were read off the ladder: cn_conv_transpose4x4s2 (csrc/cn_conv.hip: the implicit GEMM in parity form
for key 10 = 1, Cout <= 32 or an output that cannot take 16-byte stores), cn_deconv4x4s2_halo (csrc/cn_conv3x3.hip)
and cn_deconv4x4s2p_takes (csrc/cn_conv3x3p.hip).  instantiation(c) names the template instantiation a case's
expectation stands for; INSTANTIATIONS is the list the ladders can launch.  The LDS buffering of the implicit GEMM
(cn_set_tuning key 1) is not part of the query's answer and not told apart here.

Shapes are the smallest at which the kernel named still has a ragged edge in every tiled dimension: B 1..3, input
maps at most 9 x 33 (W = 15 / 17: 8 x 16 tiles, W = 33: 4 x 32), Cin = 8 / 40 (fp16: 40 / 72) for a ragged K chunk.
Larger only where a form starts at a number of workgroups or items (the occ4 rule, the persistent kernel's 256)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script: the list of cases per instantiation)
    sys.path.insert(0, ROOT)

from centernet_amd import native   # noqa: E402
from centernet_amd.native import (C3_OCC4, C3_PERSIST, C3_TILE, C3_TW32, C3_WAVES8, CONV_X_PLAIN,   # noqa: E402
                                  CONV_Y_PLAIN, DTYPE_F16, DTYPE_F32, DTYPE_F32S)

OK, ERR_UNSUPPORTED, ERR_ALIGN = 0, -2, -6
F32, F16, F32S = "f32", "f16", "f32s"
DTYPES = {F32: DTYPE_F32, F16: DTYPE_F16, F32S: DTYPE_F32S}
XP, YP = CONV_X_PLAIN, CONV_Y_PLAIN
T = C3_TILE


def pf(taps):
    return taps << 12


def r32(c):
    return (c + 31) // 32 * 32


def _c(id, route, variant=0, n_tile=0, m_tile=0, *, shape, dt=F32, flags=0, keys=None, in_pitch=None, out_pitch=None,
       c_off=0, rc=OK, scale=True, x_off=0, exact=False, relu=1):
    """shape = (B, Cin, H, W, Cout) of the INPUT map; in_pitch / out_pitch: None = the tensor's own width (f32s
    tensors: whole 32-channel groups; a plain output: the next multiple of 4, what 16-byte stores need); c_off:
    first channel of y inside its tensor (elements; moves the pointer); x_off: bytes the x pointer is moved by
    (refused calls); scale: False = a null scale; exact: also run the case on integer operands and require
    equality"""
    B, Cin, H, W, Cout = shape
    return dict(id=id, route=route, variant=variant, n_tile=n_tile, m_tile=m_tile, B=B, Cin=Cin, H=H, W=W, Cout=Cout,
                dt=dt, flags=flags, keys=dict(keys or {}), in_pitch=in_pitch, out_pitch=out_pitch, c_off=c_off, rc=rc,
                scale=scale, x_off=x_off, exact=exact, relu=relu)


P28 = {28: 2}          # the persistent kernel at every size
CASES = []

# ---- tile kernel: {fp32, f32s, fp16} x {TW 16, TW 32} x {Cout 33 -> 64-wide, Cout 65 and 129 -> 128-wide} ----------
for _dt, _ci in ((F32, (8, 40)), (F32S, (8, 40)), (F16, (40, 72))):
    _v64 = T | (pf(1) if _dt == F32S else 0)
    _v128 = T | C3_WAVES8 | (pf(3) if _dt == F32S else 0)
    CASES += [
        _c("tile_%s_w15_co33" % _dt, "halo", _v64, 64, 128, shape=(2, _ci[0], 5, 15, 33), dt=_dt, exact=True),
        _c("tile_%s_w17_co65" % _dt, "halo", _v128, 128, 128, shape=(1, _ci[1], 9, 17, 65), dt=_dt),
        _c("tile_%s_w17_co129" % _dt, "halo", _v128, 128, 128, shape=(1, _ci[0], 5, 17, 129), dt=_dt),
        _c("tile_%s_w33_co33" % _dt, "halo", _v64 | C3_TW32, 64, 128, shape=(1, _ci[1], 5, 33, 33), dt=_dt),
        _c("tile_%s_w33_co65" % _dt, "halo", _v128 | C3_TW32, 128, 128, shape=(1, _ci[0], 9, 33, 65), dt=_dt,
           exact=True),
        _c("tile_%s_w33_co129" % _dt, "halo", _v128 | C3_TW32, 128, 128, shape=(3, _ci[1], 5, 33, 129), dt=_dt),
    ]
CASES += [
    # f32s arithmetic with a plain tensor on one side; Cout = 40 packed: a ragged last 32-channel group
    _c("tile_f32s_xplain_w17_co65", "halo", T | C3_WAVES8 | pf(3), 128, 128, shape=(1, 40, 9, 17, 65), dt=F32S,
       flags=XP),
    _c("tile_f32s_xplain_w33_co33", "halo", T | C3_TW32 | pf(1), 64, 128, shape=(1, 8, 5, 33, 33), dt=F32S, flags=XP),
    _c("tile_f32s_yplain_w15_co33", "halo", T | pf(1), 64, 128, shape=(2, 8, 5, 15, 33), dt=F32S, flags=YP),
    _c("tile_f32s_yplain_w33_co129", "halo", T | C3_TW32 | C3_WAVES8 | pf(3), 128, 128, shape=(1, 40, 5, 33, 129),
       dt=F32S, flags=YP),
    _c("tile_f32s_w17_co40", "halo", T | pf(1), 64, 128, shape=(1, 40, 9, 17, 40), dt=F32S),
    # pitches: in_pitch > Cin, the output a member of a wider tensor (32 channels in)
    _c("tile_f32_pitches", "halo", T, 64, 128, shape=(1, 8, 9, 17, 33), in_pitch=12, out_pitch=72, c_off=32),
    _c("tile_f16_pitches", "halo", T, 64, 128, shape=(1, 40, 9, 17, 33), dt=F16, in_pitch=48, out_pitch=72, c_off=32),
    _c("tile_f32s_pitches", "halo", T | pf(1), 64, 128, shape=(1, 8, 9, 17, 33), dt=F32S, in_pitch=64, out_pitch=128,
       c_off=32),
    _c("tile_f32s_yplain_pitches", "halo", T | C3_WAVES8 | pf(3), 128, 128, shape=(1, 40, 5, 17, 65), dt=F32S,
       flags=YP, in_pitch=64, out_pitch=100, c_off=32),
    # ---- fp32, four workgroups per CU: key 19 = 1 at both tile shapes; by the rule and against it: OCC4_RULE below
    _c("occ4_f32_w17_key19_1", "halo", T | C3_OCC4, 64, 128, shape=(2, 40, 9, 17, 33), keys={19: 1}, exact=True),
    _c("occ4_f32_w33_key19_1", "halo", T | C3_OCC4 | C3_TW32, 64, 128, shape=(1, 8, 5, 33, 64), keys={19: 1}),
    _c("occ4_f32_pitches", "halo", T | C3_OCC4, 64, 128, shape=(1, 8, 9, 17, 33), keys={19: 1}, in_pitch=12,
       out_pitch=72, c_off=32),
    # ---- persistent kernel (key 28 = 2): f32s and plain output, key 30 at its default (2: pipelined) and with the
    # PIPE bit cleared, each in both MFMA shapes (bit 2); Cout 96: a half-empty second output block
    _c("persist_co64", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 64), dt=F32S, keys=P28, exact=True),
    _c("persist_co96", "halo", C3_PERSIST, shape=(2, 40, 5, 15, 96), dt=F32S, keys=P28),
    _c("persist_co64_yplain", "halo", C3_PERSIST, shape=(1, 40, 9, 17, 64), dt=F32S, keys=P28, flags=YP),
    _c("persist_co96_yplain", "halo", C3_PERSIST, shape=(1, 8, 5, 17, 96), dt=F32S, keys=P28, flags=YP),
    _c("persist_co64_nopipe", "halo", C3_PERSIST, shape=(1, 40, 9, 17, 64), dt=F32S, keys={28: 2, 30: 0}),
    _c("persist_co96_yplain_nopipe", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 96), dt=F32S, keys={28: 2, 30: 0},
       flags=YP),
    _c("persist_co64_m32", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 64), dt=F32S, keys={28: 2, 30: 6}),
    _c("persist_co64_yplain_m32", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 64), dt=F32S, keys={28: 2, 30: 6},
       flags=YP),
    _c("persist_co96_nopipe_m32", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 96), dt=F32S, keys={28: 2, 30: 4}),
    _c("persist_co64_yplain_nopipe_m32", "halo", C3_PERSIST, shape=(1, 40, 5, 15, 64), dt=F32S, keys={28: 2, 30: 4},
       flags=YP),
    _c("persist_pitches", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 64), dt=F32S, keys=P28, in_pitch=64, out_pitch=128,
       c_off=32),
    _c("persist_yplain_pitches", "halo", C3_PERSIST, shape=(1, 8, 9, 17, 64), dt=F32S, keys=P28, flags=YP,
       in_pitch=64, out_pitch=128, c_off=32),
    # by the library's own rule (key 28 = 1): 4 * B * ceil(H/8) * ceil(W/16) * ceil(Cout/64) >= 256
    _c("persist_by_rule", "halo", C3_PERSIST, shape=(2, 8, 9, 113, 96), dt=F32S),
    _c("persist_by_rule_below", "halo", T | C3_TW32 | C3_WAVES8 | pf(3), 128, 128, shape=(2, 8, 9, 112, 96), dt=F32S),
    # each refusal says "tile"
    _c("persist_refused_key32_0", "halo", T | pf(1), 64, 128, shape=(1, 8, 9, 17, 64), dt=F32S, keys={28: 2, 32: 0}),
    _c("persist_refused_key28_0", "halo", T | pf(1), 64, 128, shape=(1, 8, 9, 17, 64), dt=F32S, keys={28: 0}),
    _c("persist_refused_xplain", "halo", T | pf(1), 64, 128, shape=(1, 8, 9, 17, 64), dt=F32S, keys=P28, flags=XP),
    _c("persist_refused_co40", "halo", T | pf(1), 64, 128, shape=(1, 8, 9, 17, 40), dt=F32S, keys=P28),
    _c("persist_refused_null_scale", "halo", T | pf(1), 64, 128, shape=(1, 8, 9, 17, 64), dt=F32S, keys=P28,
       scale=False),
    _c("persist_refused_yplain_pitch100", "halo", T | C3_WAVES8 | pf(3), 128, 128, shape=(1, 8, 9, 17, 96), dt=F32S,
       keys=P28, flags=YP, out_pitch=100),
]
# ---- implicit GEMM in parity form: Cout = 24 and 32 (n_tile 32), key 10 = 1 at Cout 33 / 65 (n_tile 64 / 128) -------
for _dt, _ci in ((F32, 8), (F32S, 40), (F16, 40)):
    CASES += [
        _c("igemm_%s_co24" % _dt, "igemm", 0, 32, 128, shape=(2, _ci, 5, 15, 24), dt=_dt, exact=_dt == F32),
        _c("igemm_%s_co32" % _dt, "igemm", 0, 32, 128, shape=(1, _ci, 9, 17, 32), dt=_dt),
        _c("igemm_%s_co33_key10" % _dt, "igemm", 0, 64, 128, shape=(1, _ci, 9, 17, 33), dt=_dt, keys={10: 1}),
        _c("igemm_%s_co65_key10" % _dt, "igemm", 0, 128, 128, shape=(1, _ci, 5, 33, 65), dt=_dt, keys={10: 1},
           exact=_dt != F32),
    ]
CASES += [
    # an output that cannot take 16-byte stores runs here at every Cout: out_pitch % 4 != 0, y one element in
    _c("igemm_scalar_pitch27_f32", "igemm", 0, 32, 128, shape=(1, 8, 9, 17, 27), out_pitch=27),
    _c("igemm_scalar_pitch67_f32", "igemm", 0, 128, 128, shape=(1, 40, 9, 17, 65), out_pitch=67),
    _c("igemm_scalar_yoff1_f32", "igemm", 0, 128, 128, shape=(1, 8, 5, 17, 65), out_pitch=68, c_off=1, exact=True),
    _c("igemm_scalar_yoff1_f32s", "igemm", 0, 128, 128, shape=(1, 40, 5, 17, 65), dt=F32S, flags=YP, out_pitch=68,
       c_off=1),
    _c("igemm_scalar_pitch67_f32s", "igemm", 0, 128, 128, shape=(1, 8, 9, 17, 65), dt=F32S, flags=XP | YP,
       out_pitch=67),
    _c("igemm_scalar_yoff1_f16", "igemm", 0, 64, 128, shape=(1, 40, 5, 17, 33), dt=F16, out_pitch=40, c_off=1),
    _c("igemm_f32_pitches", "igemm", 0, 32, 128, shape=(1, 8, 9, 17, 24), in_pitch=12, out_pitch=64, c_off=32),
    _c("igemm_f32s_pitches", "igemm", 0, 32, 128, shape=(1, 8, 9, 17, 24), dt=F32S, in_pitch=64, out_pitch=96,
       c_off=32),
    _c("igemm_f16_pitches", "igemm", 0, 32, 128, shape=(1, 40, 9, 17, 24), dt=F16, in_pitch=48, out_pitch=64,
       c_off=32),
    # ---- refused calls: the same status from query and call, nothing written -------------------------------------
    _c("refused_f16_xplain", "none", rc=ERR_UNSUPPORTED, shape=(1, 40, 9, 17, 33), dt=F16, flags=XP),
    _c("refused_f16_yplain", "none", rc=ERR_UNSUPPORTED, shape=(1, 40, 9, 17, 33), dt=F16, flags=YP),
    _c("refused_cin6_f32", "none", rc=ERR_UNSUPPORTED, shape=(1, 6, 9, 17, 33), in_pitch=8),
    _c("refused_cin12_f16", "none", rc=ERR_UNSUPPORTED, shape=(1, 12, 9, 17, 33), dt=F16, in_pitch=16),
    _c("refused_f32s_in_pitch40", "none", rc=ERR_UNSUPPORTED, shape=(1, 40, 9, 17, 33), dt=F32S, in_pitch=40),
    _c("refused_f32s_out_pitch40", "none", rc=ERR_UNSUPPORTED, shape=(1, 8, 9, 17, 33), dt=F32S, out_pitch=40),
    _c("refused_f32s_x_off16", "none", rc=ERR_ALIGN, shape=(1, 8, 9, 17, 33), dt=F32S, x_off=16),
    _c("refused_f32s_y_off16", "none", rc=ERR_ALIGN, shape=(1, 8, 9, 17, 33), dt=F32S, out_pitch=64, c_off=4),
]

# fp32 occ4 by the rule (key 19 = 0): 4 * B * tiles in (768, 1024].  17 x 385 = 5 x 13 tiles of 4 x 32; B = 3 is the
# smallest batch (tests/test_deconv_heads_route_cases_host.py scans for it); key 19 = 2 on the same grid says "never"
OCC4_RULE = _c("occ4_f32_by_rule", "halo", T | C3_OCC4 | C3_TW32, 64, 128, shape=(3, 8, 17, 385, 33))
CASES += [OCC4_RULE,
          _c("occ4_f32_key19_2", "halo", T | C3_TW32, 64, 128, shape=(3, 8, 17, 385, 33), keys={19: 2})]

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# every instantiation the ladders can launch
INSTANTIATIONS = (["tile<%s,TW%d,BN%d>" % (dt, tw, bn) for dt in (F32, F32S, F16) for tw in (16, 32) for bn in (64, 128)] +
                  ["occ4<f32,TW%d>" % tw for tw in (16, 32)] +
                  ["persist<%s,%s,%s>" % (o, p, m) for o in ("f32s_out", "plain_out") for p in ("pipe", "nopipe")
                   for m in ("m16x16x32", "m32x32x16")] +
                  ["igemm_parity<%s,BN%d>" % (dt, bn) for dt in (F32, F32S, F16) for bn in (32, 64, 128)])


def instantiation(c):
    """the template instantiation the case's expectation stands for (None: a refused call)"""
    if c["rc"] != OK:
        return None
    if c["route"] == "igemm":
        return "igemm_parity<%s,BN%d>" % (c["dt"], c["n_tile"])
    if c["variant"] == C3_PERSIST:
        k30 = c["keys"].get(30, 2)
        return "persist<%s,%s,%s>" % ("plain_out" if c["flags"] & YP else "f32s_out", "pipe" if k30 & 2 else "nopipe",
                                      "m32x32x16" if k30 & 4 else "m16x16x32")
    tw = 32 if c["variant"] & C3_TW32 else 16
    if c["variant"] & C3_OCC4:
        return "occ4<%s,TW%d>" % (c["dt"], tw)
    return "tile<%s,TW%d,BN%d>" % (c["dt"], tw, c["n_tile"])


# ---- the arguments of a case -----------------------------------------------------------------------------------------
def packed_in(c):
    return c["dt"] == F32S and not c["flags"] & XP


def packed_out(c):
    return c["dt"] == F32S and not c["flags"] & YP


def pitches(c):
    ip = c["in_pitch"] or (r32(c["Cin"]) if packed_in(c) else c["Cin"])
    op = c["out_pitch"] or (r32(c["Cout"]) if packed_out(c) else (c["Cout"] + 3) // 4 * 4)
    return ip, op


def elem_bytes(c):
    return 2 if c["dt"] == F16 else 4


def args(c, x, w, scale, shift, y, ctl=None):
    """the argument list of cn_conv_transpose4x4s2 (without the stream) for these addresses"""
    vp = ctypes.c_void_p
    ip, op = pitches(c)
    return [vp(x), vp(w), vp(scale) if c["scale"] else None, vp(shift), vp(y), c["B"], c["H"], c["W"], c["Cin"],
            c["Cout"], ip, op, c["relu"], DTYPES[c["dt"]], c["flags"], ctl]


def query(c, x, w, scale, shift, y):
    info = native.ConvRouteInfo()
    with native.tuning(c["keys"]):
        rc = native.lib().cn_conv_transpose4x4s2_route(*args(c, x, w, scale, shift, y), None, ctypes.byref(info))
    return rc, info


def fake_pointers(c):
    """addresses for a host-only query: every tensor 256-byte aligned, x and y moved as the case says"""
    return dict(x=0x7300_0000_0000 + c["x_off"], w=0x7400_0000_0000, scale=0x7500_0000_0000, shift=0x7500_0001_0000,
                y=0x7000_0000_0000 + c["c_off"] * elem_bytes(c))


def expected(c):
    return (c["rc"], c["route"], c["variant"], c["n_tile"], c["m_tile"])


def said(rc, info):
    return (rc, native.conv_route_name(info.route), info.variant, info.n_tile, info.m_tile)


def pins():
    """{instantiation: [case ids]}"""
    out = {n: [] for n in INSTANTIATIONS}
    for c in CASES:
        out.setdefault(instantiation(c) or "refused", []).append(c["id"])
    return out


if __name__ == "__main__":      # python tests/deconv_route_cases.py: the list, per instantiation
    for name, ids in pins().items():
        print("%-36s %s" % (name, " ".join(ids) or "-- NONE --"))
