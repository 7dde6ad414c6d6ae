"""Answers of the host-only decode queries over a fixed grid of (B, C, H, W, K[, J]) ->
tests/golden/decode_queries.json.

    cn_ctdet_decode_workspace_bytes, cn_multi_pose_decode_workspace_bytes, cn_ddd_decode_workspace_bytes,
    cn_exct_decode_workspace_bytes, cn_agnex_ct_decode_workspace_bytes, cn_decode_state_region

The file in the repository was written by the library as it was BEFORE the queries moved onto cn_decode.hip's
topk_route (CENTERNET_AMD_LIB pointing at a build of that commit); tests/test_decode_route_host.py asserts that
the library of the tree gives the same answers.  Needs no GPU.

    CENTERNET_AMD_LIB=/path/to/libcenternet_amd.so python tests/golden/gen_decode_queries.py
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_queries.json")

# What bench.py decodes: (B, C, H, W, K, J) of its configurations at the default 512 x 512 input (ctdet
# resdcn_18 / dla_34 at batch 32, hourglass at batch 8, multi_pose dla_34 at batch 32) and of its batch-1 leg.
MODEL_SHAPES = ((32, 80, 128, 128, 100, 17), (8, 80, 128, 128, 100, 17), (1, 80, 128, 128, 100, 17),
                (32, 1, 128, 128, 100, 17), (1, 1, 128, 128, 100, 17))

BATCHES = (1, 8, 32)
# one class (the pose centre map), few, the joints, COCO, the most the one-launch form takes and one more
CLASSES = (1, 3, 17, 80, 1024, 1025)
# (H, W).  Both sides of: W & 3; planes of 128 x 128 (one launch) in H and in W; one band of 8192 cells per
# plane against several; W > 4096 (no band plan); and, with the largest K below, bands that must grow past
# 16384 cells to supply K candidates (no band plan either)
MAPS = ((1, 8), (7, 9), (10, 18), (16, 16), (23, 17), (64, 64), (72, 128), (128, 128), (129, 128), (128, 132),
        (96, 160), (152, 272), (200, 200), (4, 4096), (4, 4100), (8, 3000))
# around 4 K against the groups of an image (16 groups: 4 / 5), the detectors' 40 and 100, KMAX = 128 and past it,
# and a K no band can supply
TOPK = (1, 4, 5, 40, 100, 128, 129, 17000)
JOINTS = (1, 17)


def points():
    """The grid, in a fixed order: (B, C, H, W, K)."""
    seen = set()
    for s in MODEL_SHAPES:
        seen.add(s[:5])
        yield s[:5]
    for B in BATCHES:
        for C in CLASSES:
            for (H, W) in MAPS:
                for K in TOPK:
                    if (B, C, H, W, K) not in seen:
                        yield (B, C, H, W, K)


# ---- refused calls: which argument error each top-K entry reports when several apply.  Every call below is
# refused on the host before anything is launched -- at the latest for its workspace of 0 bytes (the shape has
# two bands per plane, so every entry wants one; the one-band shape comes with a null output) -- so the pointers
# are never followed: PTR is just an aligned non-null value, ODD a misaligned one.
PTR, ODD = 4096, 4100
ENTRIES = ("ctdet", "topk", "channel", "multi_pose", "multi_pose_match")
FAULTS = {
    "heat_null": dict(heat=None), "batch_0": dict(B=0), "k_past_map": dict(K=72 * 128 + 1), "k_past_kmax": dict(K=129),
    "too_wide": dict(W=4100), "misaligned": dict(heat=ODD), "out_null": dict(out=None), "ws_null": dict(ws=None),
    "no_joints": dict(J=0), "one_band": dict(H=16, W=16, out=None), "hm_hp_misaligned": dict(hm_hp=ODD),
}


def refused_calls():
    """(entry, faults) in a fixed order: no fault but the empty workspace, every fault, every pair of faults."""
    names = sorted(FAULTS)
    sets = [()] + [(a,) for a in names] + [(a, b) for i, a in enumerate(names) for b in names[i + 1:]]
    return [(e, s) for e in ENTRIES for s in sets]


def refuse(lib, entry, faults):
    a = dict(heat=PTR, B=2, C=4, H=72, W=128, K=8, J=3, out=PTR, ws=PTR, hm_hp=PTR)
    for f in faults:
        a.update(FAULTS[f])
    shape = (a["B"], a["C"], a["H"], a["W"], a["K"])
    if entry == "ctdet":
        return lib.cn_ctdet_decode_f32(a["heat"], PTR, PTR, *shape, 0, 1, a["out"], PTR, a["ws"], 0, None)
    if entry == "topk":
        return lib.cn_topk_f32(a["heat"], *shape, 1, a["out"], PTR, PTR, a["ws"], 0, None)
    if entry == "channel":
        return lib.cn_nms_topk_channel_f32(a["heat"], *shape, 1, a["out"], PTR, a["ws"], 0, None)
    if entry == "multi_pose":
        return lib.cn_multi_pose_decode_f32(a["heat"], PTR, PTR, PTR, a["hm_hp"], PTR, *shape[:4], a["J"], a["K"], 1,
                                            a["out"], a["ws"], 0, None)
    # the joints' map is this entry's heat-map
    hm_hp = a["hm_hp"] if a["heat"] == PTR else a["heat"]
    return lib.cn_multi_pose_match_f32(hm_hp, PTR, a["B"], a["J"], a["H"], a["W"], a["K"], 1, a["out"], a["ws"], 0,
                                       None)


def answers():
    """{query: one number per point of the grid}; multi_pose: per J of JOINTS; state region: return code,
    offset and bytes; "refused": the return code of every call of refused_calls()."""
    from centernet_amd import native
    lib = native.lib()
    grid = list(points())
    out = {"n": len(grid)}
    for q in ("ctdet", "ddd", "exct", "agnex_ct"):
        f = getattr(lib, "cn_%s_decode_workspace_bytes" % q)
        out[q] = [int(f(*p)) for p in grid]
    for J in JOINTS:
        out["multi_pose_j%d" % J] = [int(lib.cn_multi_pose_decode_workspace_bytes(B, C, H, W, J, K))
                                     for (B, C, H, W, K) in grid]
    rc, off, nb = [], [], []
    for p in grid:
        o, n = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
        rc.append(int(lib.cn_decode_state_region(*p, ctypes.byref(o), ctypes.byref(n))))
        off.append(int(o.value))
        nb.append(int(n.value))
    out["state_rc"], out["state_offset"], out["state_bytes"] = rc, off, nb
    out["refused"] = [int(refuse(lib, e, s)) for e, s in refused_calls()]
    return out


if __name__ == "__main__":
    a = answers()
    with open(OUT, "w") as f:
        json.dump(a, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    for k, v in sorted(a.items()):
        if k != "n":
            print(k, len(set(v)), "distinct answers,", sum(1 for x in v if x), "non-zero of", len(v))
