"""What cn_dcn_v2_forward_nhwc does with a call -- return code of its checks, kernel form, grid, K split, flags --
over a fixed grid of calls and tuning keys, and the answers of cn_dcn_v2_forward_nhwc_workspace_bytes
-> tests/golden/dcn_routes.json.  Needs no GPU: every pointer is made up and never followed.

Run against the library of the tree, the answers come from the host query cn_dcn_v2_route.
tests/test_dcn_route_host.py asserts that they are the recorded ones.

The file in the repository was recorded from the library as it was BEFORE the decision moved into dcn_route
(csrc/cn_dcn.hip), when it was spread over the entry in cn_conv.hip and the three launchers and no query could
state it.  That build carried the recording patch below (never committed): a process-global dry switch that
makes the three launch sites note what they would have launched and return CN_OK.  (The gather form is noted
where its launch computes the grid, launch_igemm_n, which is where the entry's igemm_dispatch<A_DCN...> call
ends, rather than at that call: the note then holds the grid of the launch, not a second derivation of it.)

To record again: check that commit out, apply the patch, build it, copy this file into its tests/golden/ and run
it there (it then binds that tree's library, which has no cn_dcn_v2_route, and takes the dry path of _answer):

    python tests/golden/gen_dcn_routes.py

--- a/centernet_amd/csrc/cn_internal.h
+++ b/centernet_amd/csrc/cn_internal.h
@@ -5,2 +5,5 @@
 #include "cn_common.h"
+// RECORDING PATCH: dry switch + the note of what a call would have launched
+struct CnDryNote { int on, family, v, grid_x, grid_y, grid_z, ksplit, flags, reduce; };
+extern CnDryNote cn_dry;
--- a/centernet_amd/csrc/cn_dcn_window.h
+++ b/centernet_amd/csrc/cn_dcn_window.h
@@ -12,1 +12,2 @@
 #include "cn_internal.h"
+#include <type_traits>
@@ -167,2 +168,7 @@ int dcnw_launch(const Args &a, unsigned n_blocks_y, hipStream_t st)
     const dim3 grid((unsigned)(a.B * a.tiles_x * a.tiles_y), n_blocks_y, (unsigned)a.ksplit);
+    if (cn_dry.on) {
+        cn_dry.grid_x = grid.x; cn_dry.grid_y = grid.y; cn_dry.grid_z = grid.z; cn_dry.ksplit = a.ksplit;
+        if constexpr (std::is_same<Args, DcnWinArgs>::value) cn_dry.flags = (a.prefetch ? 1 : 0) | (a.stagger ? 2 : 0);
+        return CN_OK;
+    }
     if (a.dbg && a.mask_sigmoid) {
--- a/centernet_amd/csrc/cn_dcn2.hip
+++ b/centernet_amd/csrc/cn_dcn2.hip
@@ -436,2 +436,3 @@ int cn_dcn_window_f32s(const DcnWinCall &c, int min_wgs, int *ksplit_out, hipStream_t st)
     if (ksplit_out) *ksplit_out = ksplit;
+    cn_dry.family = 2; cn_dry.v = bn;
     if (bn == 64)
--- a/centernet_amd/csrc/cn_dcn3.hip
+++ b/centernet_amd/csrc/cn_dcn3.hip
@@ -442,2 +442,3 @@ int cn_dcn_team_f32s(const DcnWinCall &c, int nmode, int *ksplit_out, hipStream_t st)
     if (ksplit_out) *ksplit_out = a.ksplit;
+    cn_dry.family = 3; cn_dry.v = nmode ? 1 : 0;
     if (nmode)
--- a/centernet_amd/csrc/cn_dcn4.hip
+++ b/centernet_amd/csrc/cn_dcn4.hip
@@ -513,2 +513,3 @@ int cn_dcn_wide_f32s(const DcnWinCall &c, int nb, int *ksplit_out, hipStream_t st)
     if (ksplit_out) *ksplit_out = a.ksplit;
+    cn_dry.family = 4; cn_dry.v = nb;
     // LDS: shared regions + epilogue constants + ring; the four-block form adds its second window
--- a/centernet_amd/csrc/cn_conv.hip
+++ b/centernet_amd/csrc/cn_conv.hip
@@ -765,2 +765,8 @@ int launch_igemm_n(const IgemmArgs &a, hipStream_t st)
     constexpr size_t lds = igemm_lds_bytes<BM, BN, WM, AMODE, OUT_NCHW, NBUF>();
+    if (cn_dry.on) {
+        cn_dry.family = AMODE == A_DCN ? 0 : (AMODE == A_DCN_PAD ? 1 : -1); cn_dry.v = BN;
+        cn_dry.grid_x = cn_cdiv(a.M, BM); cn_dry.grid_y = cn_cdiv(a.Cout, BN); cn_dry.grid_z = a.ksplit > 1 ? a.ksplit : 1;
+        cn_dry.ksplit = a.ksplit; cn_dry.flags = (a.tile2d ? 4 : 0) | (a.vec_out ? 8 : 0);
+        return CN_OK;
+    }
     CN_SET_MAX_LDS_ONCE((igemm_kernel<T, BM, BN, WM, WN, AMODE, OUT_NCHW, NBUF>), lds);
@@ -996,2 +1002,3 @@ int launch_splitk_reduce(int dtype, const IgemmArgs &a, int cap, hipStream_t st)
 {
+    if (cn_dry.on) { cn_dry.reduce = a.ksplit; return CN_OK; }
     const size_t total = (size_t)a.M * (a.cout_pad >> 2);
@@ -1619,2 +1626,5 @@
 CnTuning cn_knobs = cn_tuning_defaults();
+CnDryNote cn_dry = {};
+extern "C" void cn_dry_switch(int on) { cn_dry = {}; cn_dry.on = on; }   // also clears the note
+extern "C" void cn_dry_note(int *out9) { const int *p = &cn_dry.on; for (int i = 0; i < 9; ++i) out9[i] = p[i]; }
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dcn_routes.json")

F32, F16, F32S = 0, 1, 2
Y_PLAIN = 2
GATHER, GATHER_PAD, WINDOW, TEAM_T, TEAM_N, WIDE4, WIDE8 = range(7)   # cn_dcn_route_info.form
BATCHES = (1, 8, 32)
# (Cin, Cout, H, W): the deformable layers of resdcn_18 and dla_34 at a 512 x 512 image (512 -> 256 @ 16^2,
# 256 -> 128 @ 32^2, 128 -> 64 @ 64^2: both; then dla_34's up-sampling nodes and the projections of its last IDAUp)
LAYERS = ((512, 256, 16, 16), (256, 128, 32, 32), (128, 64, 64, 64),
          (256, 256, 32, 32), (128, 128, 64, 64), (64, 64, 128, 128), (256, 64, 32, 32))
# H not a multiple of 8, W not a multiple of 16, Cin % 32 != 0; then a sweep of Cout
OFF = ((64, 128, 12, 16), (64, 128, 8, 24), (48, 128, 8, 16)) + \
      tuple((64, co, 32, 32) for co in (24, 32, 36, 64, 66, 128, 192, 256))
# (B, Cin, Cout, H, W) at the coordinate limits of the window forms: W > 16383 (15-bit corner coordinates of the
# team / wide records), W > 32767 (16-bit ones of the register-sampling form), B * H * W = 2^24 (24-bit multiplies)
LIMITS = ((1, 32, 64, 8, 16400), (1, 32, 64, 8, 32784), (32, 32, 36, 1024, 512))
SHAPES = tuple((B,) + s for B in BATCHES for s in LAYERS + OFF) + LIMITS
DTYPE_FLAGS = ((F32, 0), (F32, Y_PLAIN), (F32S, 0), (F32S, Y_PLAIN))
# the workspace a call is given: none / what the workspace query answers / one float short of the slabs of each
# split of the window forms (2, 4, 8) and of the gather form (3, 9) / nine slabs / nine slabs, misaligned
WORKSPACES = ("none", "query", "short2", "short4", "short8", "short3", "short9", "ample", "misaligned")
OUT_PITCHES = ("cout", "larger", "odd")   # Cout (f32s tensors: rounded up to 32) / 32 more / not a multiple of 4
OM_PITCHES = (27, 32, 40)
# cn_set_tuning: the defaults, then one key changed at a time.  Keys 37 / 42 (the team / wide form's split
# target): far above and far below every workgroup count of the grid.  One pair: key 36 = 2 (T mode) differs from
# its default 3 (N mode where that fills the chip) only on calls the wide form would take, so also with key 41 = 0
KEYS = ({}, {23: 1}, {23: 2}, {23: 4}, {23: 5}, {23: 6}, {23: 7}, {5: 1}, {13: 1}, {13: 3}, {13: 9},
        {36: 0}, {36: 1}, {36: 2}, {41: 0}, {36: 2, 41: 0}, {37: 4096}, {37: 1}, {42: 4096}, {42: 1}, {9: 1}, {22: 0})
KEYS_PITCH = ({}, {23: 1}, {23: 2}, {23: 4}, {23: 6})          # the keys of the pitch / alignment grid
KEYS_QUERY = ({}, {5: 1}, {13: 1}, {13: 3}, {13: 9})           # the keys of the workspace query's golden
# made-up addresses, 128-byte aligned
X, WT, BIAS, OM, SCALE, SHIFT, Y, WS = (0x10000000 * (i + 1) for i in range(8))


def _r32(c):
    return (c + 31) // 32 * 32


def _slab(B, Cout, H, W):
    return 4 * B * H * W * _r32(Cout)


def _pitch(kind, Cout, dt, fl):
    base = _r32(Cout) if (dt == F32S and not fl & Y_PLAIN) else Cout
    if kind == "cout":
        return base
    if kind == "larger":
        return base + 32
    return Cout + (2 if (Cout + 1) % 4 == 0 else 1)


def main_grid():
    """(B, Cin, Cout, H, W, dtype, flags, out_pitch kind, om_pitch, om offset, y offset, workspace): every shape,
    dtype and workspace, at the usual pitches and alignments"""
    for shape in SHAPES:
        for (dt, fl) in DTYPE_FLAGS:
            for ws in WORKSPACES:
                yield shape + (dt, fl, "cout", 32, 0, 0, ws)


def pitch_grid():
    """every shape and dtype with the workspace the query asks for: out_pitch, om_pitch, om aligned to 8 bytes
    and to 4 only, y aligned and not"""
    for shape in SHAPES:
        for (dt, fl) in DTYPE_FLAGS:
            for op in OUT_PITCHES:
                for omp in OM_PITCHES:
                    for om_off in (0, 4):
                        for y_off in (0, 4):
                            yield shape + (dt, fl, op, omp, om_off, y_off, "query")


def bad_grid():
    """calls the entry's checks refuse, as overrides of one good f32s call: every check once"""
    good = dict(x=X, w=WT, om=OM, y=Y, B=2, Cin=64, H=16, W=16, Cout=64, out_pitch=64, om_pitch=32, dtype=F32S, flags=0)
    for over in (dict(x=0), dict(w=0), dict(om=0), dict(y=0), dict(B=0), dict(Cin=0), dict(H=0), dict(W=0),
                 dict(Cout=0), dict(out_pitch=63, flags=Y_PLAIN), dict(om_pitch=26), dict(Cin=30), dict(dtype=F16),
                 dict(dtype=3), dict(out_pitch=80), dict(x=X + 4), dict(w=WT + 8), dict(y=Y + 16),
                 dict(B=32, H=1024, W=512), dict()):
        yield dict(good, **over)


def _call_args(p, lib):
    """the argument list of cn_dcn_v2_forward_nhwc for a point of main_grid / pitch_grid"""
    B, Cin, Cout, H, W, dt, fl, op, omp, om_off, y_off, ws = p
    slab = _slab(B, Cout, H, W)
    wsp, wsb = WS, 9 * slab
    if ws == "none":
        wsp, wsb = None, 0
    elif ws == "query":
        wsb = int(lib.cn_dcn_v2_forward_nhwc_workspace_bytes(B, Cin, H, W, Cout))
        wsp = WS if wsb else None
    elif ws.startswith("short"):
        wsb = int(ws[5:]) * slab - 4
    elif ws == "misaligned":
        wsp = WS + 4
    return [X, WT, BIAS, OM + om_off, omp, SCALE, SHIFT, Y + y_off, _pitch(op, Cout, dt, fl), B, Cin, H, W, Cout, 1, 1,
            dt, fl, None, wsp, wsb, None]


def _bad_args(d):
    return [d["x"] or None, d["w"] or None, BIAS, d["om"] or None, d["om_pitch"], SCALE, SHIFT, d["y"] or None,
            d["out_pitch"], d["B"], d["Cin"], d["H"], d["W"], d["Cout"], 1, 1, d["dtype"], d["flags"], None, None, 0, None]


def _answer(lib, args):
    """[return code, form, grid_x, grid_y, ksplit, flags] of a call; a refused call: [code]"""
    from centernet_amd import native
    if hasattr(lib, "cn_dcn_v2_route"):
        info = native.DcnRouteInfo()
        rc = lib.cn_dcn_v2_route(*(args + [ctypes.byref(info)]))
        return [rc, info.form, info.grid_x, info.grid_y, info.ksplit, info.flags] if rc == 0 else [rc]
    # the recording build: run the call dry and read the note of its launch sites
    lib.cn_dry_switch(1)
    rc = lib.cn_dcn_v2_forward_nhwc(*args)
    note = (ctypes.c_int * 9)()
    lib.cn_dry_note(note)
    lib.cn_dry_switch(0)
    on, family, v, gx, gy, gz, ks, flags, reduce = note
    if rc != 0:
        assert family == 0 and gx == 0 and reduce == 0, list(note)     # refused before anything was launched
        return [rc]
    form = {(0, 128): GATHER, (0, 64): GATHER, (0, 32): GATHER, (1, 128): GATHER_PAD, (1, 64): GATHER_PAD,
            (1, 32): GATHER_PAD, (2, 64): WINDOW, (2, 128): WINDOW, (3, 0): TEAM_T, (3, 1): TEAM_N, (4, 4): WIDE4,
            (4, 8): WIDE8}[(family, v)]
    Cout = args[13]
    bn = {WINDOW: v, TEAM_T: 64, TEAM_N: 128, WIDE4: 128, WIDE8: 256}.get(form, v)
    assert gy == (Cout + bn - 1) // bn and gz == ks >= 1, list(note)
    assert reduce == (ks if ks > 1 else 0), list(note)                 # the reduce launch follows every split, and only a split
    return [rc, form, gx, gy, ks, flags]


def answers():
    """{"main" / "pitch": {keys: [answer per grid point]}, "bad": [answer per refused call], "query": {keys:
    [slabs the workspace query answers per shape]}}"""
    from centernet_amd import native
    lib = native.lib()
    lib.cn_reset_tuning()
    out = {"main": {}, "pitch": {}, "query": {}}
    for name, grid, keys in (("main", list(main_grid()), KEYS), ("pitch", list(pitch_grid()), KEYS_PITCH)):
        for k in keys:
            with native.tuning(k):
                out[name][json.dumps(k, sort_keys=True)] = [_answer(lib, _call_args(p, lib)) for p in grid]
    out["bad"] = [_answer(lib, _bad_args(d)) for d in bad_grid()]
    for k in KEYS_QUERY:
        with native.tuning(k):
            q = []
            for (B, Cin, Cout, H, W) in SHAPES:
                b = int(lib.cn_dcn_v2_forward_nhwc_workspace_bytes(B, Cin, H, W, Cout))
                assert b % _slab(B, Cout, H, W) == 0
                q.append(b // _slab(B, Cout, H, W))
            out["query"][json.dumps(k, sort_keys=True)] = q
    return out


def pack(a):
    """the JSON form: one table of the distinct answers, and per key setting a string of two base-36 digits per
    grid point that index it"""
    table = sorted({tuple(x) for g in ("main", "pitch") for v in a[g].values() for x in v} | {tuple(x) for x in a["bad"]})
    assert len(table) < 36 * 36
    index = {t: i for i, t in enumerate(table)}
    digits = "0123456789abcdefghijklmnopqrstuvwxyz"

    def enc(v):
        return "".join(digits[index[tuple(x)] // 36] + digits[index[tuple(x)] % 36] for x in v)
    return {"answers": [list(t) for t in table], "main": {k: enc(v) for k, v in a["main"].items()},
            "pitch": {k: enc(v) for k, v in a["pitch"].items()}, "bad": enc(a["bad"]),
            "query": {k: "".join(digits[s] for s in v) for k, v in a["query"].items()}}


def unpack(j):
    """the inverse of pack()"""
    def dec(s):
        return [j["answers"][int(s[i:i + 2], 36)] for i in range(0, len(s), 2)]
    return {"main": {k: dec(v) for k, v in j["main"].items()}, "pitch": {k: dec(v) for k, v in j["pitch"].items()},
            "bad": dec(j["bad"]), "query": {k: [int(c, 36) for c in v] for k, v in j["query"].items()}}


if __name__ == "__main__":
    a = answers()
    with open(OUT, "w") as f:
        json.dump(pack(a), f, indent=1, sort_keys=True)
        f.write("\n")
    for g in ("main", "pitch"):
        for k, v in a[g].items():
            forms = [x[1] for x in v if len(x) > 1]
            print(g, k, len(v), "points; forms", [forms.count(i) for i in range(7)], "splits", sorted({x[4] for x in v if len(x) > 1}))
