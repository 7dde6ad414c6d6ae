"""multi_pose run_tiles on the host (no GPU): the host tile merge (post_process.multi_pose_tiles_results -- the
specification of cn_multi_pose_tiles_merge_f32) on hand-made rows and against MultiPoseDetector.merge_outputs, the
workgroup-wide step form of soft-NMS that the kernel runs restated in numpy and held equal to cn_soft_nms_f32, the
refusals of the public entries and the new prototypes."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from centernet_amd import native, tiles
from centernet_amd.detectors.base_detector import BaseDetector
from centernet_amd.detectors.ctdet import CtdetDetector
from centernet_amd.detectors.multi_pose import MultiPoseDetector
from centernet_amd.post_process import multi_pose_tiles_results
from centernet_amd.soft_nms import soft_nms_39

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = np.array([-np.inf, -np.inf, np.inf, np.inf], F32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _detector(scales=(1.0,), nms=False, max_per_image=100, **opt):
    """A MultiPoseDetector without a device: what merge_outputs and the argument checks read"""
    det = MultiPoseDetector.__new__(MultiPoseDetector)
    det.opt = types.SimpleNamespace(nms=nms, fix_res=True, flip_test=False, input_h=128, input_w=128, K=100,
                                    num_classes=1, down_ratio=4, test_scales=list(scales))
    det.opt.__dict__.update(opt)
    det.scales, det.num_classes, det.max_per_image = list(scales), 1, max_per_image
    return det


def _row(cx, cy, w, h, score, tag=0.0):
    """one 39-column row; the joints carry ``tag`` so that a row can be told from its neighbours"""
    r = np.empty((39,), F32)
    r[:5] = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score]
    r[5:] = F32(tag) + np.arange(34, dtype=F32) / 64
    return r


def _rows(*rows):
    return np.array(rows, F32).reshape(-1, 39)


# ------------------------------------------------------------------------------------------------
# 1. the specification on hand-made rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [0, 4])
def test_core_edges_are_half_open(margin):
    g = tiles.tile_grid(128, 224, 128, 128, 32, margin)          # two tiles side by side, boundary x = 112
    lo, hi = F32(112 - margin), F32(112 + margin)
    assert g.T == 2 and g.cores[0, 2] == hi and g.cores[1, 0] == lo

    def run(cx, tile):
        per_tile = [np.zeros((0, 39), F32), np.zeros((0, 39), F32)]
        per_tile[tile] = _rows(_row(cx, 64.0, 10, 10, 0.5))
        return len(multi_pose_tiles_results(per_tile, g.cores, False, 100)[1])
    assert run(lo, 1) == 1                                        # exactly on b - m: kept by tile 1
    assert run(np.nextafter(lo, F32(0)), 1) == 0
    assert run(hi, 0) == 0                                        # exactly on b + m: not kept by tile 0
    assert run(np.nextafter(hi, F32(0)), 0) == 1
    assert run(112.0, 0) + run(112.0, 1) == (2 if margin else 1)  # inside the margin band both keep it
    assert run(float("nan"), 0) == 0 and run(float("nan"), 1) == 0


def test_tile_order_and_the_duplicate_in_the_margin():
    g = tiles.tile_grid(128, 224, 128, 128, 32, 4)
    a, b, c = _row(20, 64, 10, 10, 0.3, 1), _row(200, 64, 10, 10, 0.9, 2), _row(60, 30, 10, 10, 0.6, 3)
    # far apart: soft-NMS only sorts by score from the top (the argmax swap), the rows keep their numbers
    out = multi_pose_tiles_results([_rows(a, c), _rows(b)], g.cores, False, 100)[1]
    assert out.dtype == F32 and out.shape == (3, 39)
    assert np.array_equal(_bits(out), _bits(_rows(b, c, a)))
    # without the soft-NMS the order would be the tiles' (T > 1 always runs it: compare with one call per tile)
    one = multi_pose_tiles_results([_rows(a, c)], g.cores[:1], False, 100)[1]
    assert np.array_equal(_bits(one), _bits(_rows(a, c)))
    # the same person from both tiles, in the margin band: the copy decays below the threshold, the WHOLE array
    # is kept, so it is still there
    dup = _row(112, 64, 10, 10, 0.004, 7)
    out = multi_pose_tiles_results([_rows(dup), _rows(dup)], g.cores, False, 100)[1]
    assert out.shape == (2, 39) and out[0, 4] == F32(0.004) and out[1, 4] < 0.001


def test_one_tile_without_nms_is_the_identity():
    rng = np.random.RandomState(3)
    rows = rng.uniform(0, 100, (17, 39)).astype(F32)
    rows[:, 2:4] += rows[:, 0:2]
    keep = rows.copy()
    out = multi_pose_tiles_results([rows], INF[None], False, 17)[1]
    assert np.array_equal(_bits(out), _bits(keep)) and np.array_equal(_bits(rows), _bits(keep))
    # with --nms the same rows go through soft_nms_39
    want = keep.copy()
    soft_nms_39(want, Nt=0.5, method=2)
    out = multi_pose_tiles_results([rows], INF[None], True, 17)[1]
    assert np.array_equal(_bits(out), _bits(want)) and not np.array_equal(_bits(out), _bits(keep))


def test_cut_keeps_ties_and_order():
    # boxes far apart: the scores stay as they are; levels 5 4 4 3 3 3 2 over two tiles
    scores = [0.3, 0.5, 0.4, 0.2, 0.3, 0.4, 0.3]
    rows = _rows(*[_row(100.0 * i, 50, 10, 10, s, i) for i, s in enumerate(scores)])
    cores = np.tile(INF, (2, 1))
    full = multi_pose_tiles_results([rows[:4], rows[4:]], cores, False, 100)[1]
    assert len(full) == 7
    for cap, n in ((7, 7), (6, 6), (5, 6), (4, 6), (3, 3), (2, 3), (1, 1)):
        out = multi_pose_tiles_results([rows[:4], rows[4:]], cores, False, cap)[1]
        thresh = np.sort(full[:, 4])[::-1][cap - 1]
        assert len(out) == n and np.array_equal(_bits(out), _bits(full[full[:, 4] >= thresh])), cap


def test_min_score():
    nan = float("nan")
    scores = [0.5, 0.1, nan, 0.1000001, 0.0999999, 0.3]
    rows = _rows(*[_row(100.0 * i, 50, 10, 10, s, i) for i, s in enumerate(scores)])
    out = multi_pose_tiles_results([rows], INF[None], False, 100, min_score=0.1)[1]
    assert np.array_equal(_bits(out), _bits(rows[[0, 1, 3, 5]]))          # >= float32(0.1); the NaN score fails
    none = multi_pose_tiles_results([rows], INF[None], False, 100)[1]
    assert np.array_equal(_bits(none), _bits(rows))                      # None: no score test at all
    low = multi_pose_tiles_results([rows], INF[None], False, 100, min_score=-1e30)[1]
    assert np.array_equal(_bits(low), _bits(rows[[0, 1, 3, 4, 5]]))      # any threshold drops the NaN score
    # the test is made in float32: 0.1 as a double is below float32(0.1)
    edge = _rows(_row(0, 0, 10, 10, F32(0.1)))
    assert len(multi_pose_tiles_results([edge], INF[None], False, 100, min_score=0.1)[1]) == 1


def _clustered(rng, n):
    """boxes in a few dense clusters (the discard path runs), scores with repeats, some below the threshold"""
    centres = rng.uniform(0, 200, (max(1, n // 8), 2))
    c = centres[rng.randint(0, len(centres), n)] + rng.normal(0, rng.choice([0.5, 3.0, 15.0]), (n, 2))
    wh = rng.uniform(4, 40, (n, 2))
    rows = np.zeros((n, 39), F32)
    rows[:, 0:2] = c - wh / 2
    rows[:, 2:4] = c + wh / 2
    levels = rng.choice([4, 20, 1000])
    rows[:, 4] = (rng.randint(1, levels + 1, n) / levels) * rng.uniform(0.002, 1.0)
    rows[:, 5:] = rng.uniform(-5, 300, (n, 34))
    return rows


@pytest.mark.parametrize("T,nms", [(1, False), (1, True), (4, False), (6, True)])
def test_infinite_cores_is_merge_outputs(T, nms):
    rng = np.random.RandomState(11 + T)
    per_tile = [_clustered(rng, 40) for _ in range(T)]
    det = _detector(scales=(1.0,) * T, nms=nms)                  # the tiles as if they were test scales
    want = det.merge_outputs([{1: r.copy()} for r in per_tile], arrays=True)[1]
    got = multi_pose_tiles_results([r.copy() for r in per_tile], np.tile(INF, (T, 1)), nms, T * 40)
    assert sorted(got) == [1] and got[1].dtype == F32 and got[1].shape == want.shape == (T * 40, 39)
    assert np.array_equal(_bits(got[1]), _bits(want))


# ------------------------------------------------------------------------------------------------
# 2. the step form of the kernel, in numpy
# ------------------------------------------------------------------------------------------------
def _decay(rows, q, top, sigma, threshold):
    """decayed score and discard flag of the rows ``q`` against the box ``top``, each on its own"""
    b = rows[q]
    x1, y1, x2, y2, s = b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4]
    area = ((np.float64(1.0) + (x2 - x1)) * (np.float64(1.0) + (y2 - y1))).astype(F32)
    iw = ((np.minimum(top[2], x2) - np.maximum(top[0], x1)).astype(np.float64) + 1.0).astype(F32)
    ih = ((np.minimum(top[3], y2) - np.maximum(top[1], y1)).astype(np.float64) + 1.0).astype(F32)
    touched = (iw > 0) & (ih > 0)
    inter = (iw * ih).astype(F32)
    ta = (np.float64(top[2] - top[0]) + 1.0) * (np.float64(top[3] - top[1]) + 1.0)
    ua = ((ta + area.astype(np.float64)) - inter.astype(np.float64)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ov = (inter / ua).astype(F32)
        w = np.exp((-(ov * ov) / F32(sigma)).astype(F32).astype(np.float64)).astype(F32)
    ns = np.where(touched, (w * s).astype(F32), s)
    return ns, touched & (ns < F32(threshold))


def soft_nms_workgroup_form(rows, sigma=0.5, threshold=0.001):
    """Gaussian soft-NMS in place as pose_tiles_merge_kernel steps through it; returns the kept count.  What
    differs from the one-wave form of cn_tail.hip (tests/test_tta_host.py): the decay is computed on the rows as
    they lie BEFORE the argmax swap (position bpos stands for row i), the discard flags are 64-row ballot words,
    and the decayed scores reach their rows at the start of the next step."""
    n = rows.shape[0]
    N = n
    ns, orig, pending = np.zeros(n, F32), np.arange(n), False
    for i in range(n):
        if i >= N:
            break
        if pending:                                               # rows [i, N): what the argmax reads and writes
            rows[i:N, 4] = ns[orig[i:N]]
        sc = rows[i:N, 4]
        bpos = i + int(np.flatnonzero(sc == sc.max())[0])         # the first maximum
        top = rows[bpos, :4].copy()
        p = np.arange(i + 1, N)
        q = np.where(p == bpos, i, p)
        words = np.zeros(n // 64 + 1, np.uint64)
        if len(p):
            ns[p], disc = _decay(rows, q, top, sigma, threshold)
            orig[p] = p
            for hit in p[disc]:
                words[hit // 64] |= np.uint64(1) << np.uint64(hit % 64)
        # wave 0: the swap, then the walk
        tmp = rows[i].copy()
        rows[i] = rows[bpos]
        rows[bpos] = tmp

        def flagged(r):
            return bool((int(words[r // 64]) >> (r % 64)) & 1)
        pos = i + 1
        while pos < N:
            hit = next((r for r in range(pos, N) if flagged(r)), -1)
            if hit < 0:
                break
            while True:
                if hit == N - 1:
                    rows[hit, 4] = ns[orig[hit]]
                    N = hit
                    break
                last = N - 1
                rows[hit, :5] = rows[last, :5]
                tail = rows[hit, 5:].copy()
                rows[hit, 5:] = rows[last, 5:]
                rows[last, 5:] = tail
                orig[hit] = last
                N = last
                if not flagged(last):
                    break
            pos = hit + 1
        pending = True
    return N


def test_workgroup_form_equals_host_soft_nms():
    n_disc = 0
    for seed in range(20000, 21500):
        rng = np.random.RandomState(seed)
        rows = _clustered(rng, int(rng.choice([1, 2, 3, 8, 63, 64, 65, 130])))
        want = rows.copy()
        kept = len(soft_nms_39(want, Nt=0.5, method=2))
        got = rows.copy()
        assert soft_nms_workgroup_form(got) == kept, seed
        assert np.array_equal(_bits(got), _bits(want)), seed
        n_disc += len(rows) - kept
    assert n_disc > 1000          # the discard walk ran many times


# ------------------------------------------------------------------------------------------------
# 3. the entries
# ------------------------------------------------------------------------------------------------
def test_entries_and_refusals():
    assert hasattr(MultiPoseDetector, "run_tiles") and hasattr(MultiPoseDetector, "run_tiles_stream")
    assert hasattr(CtdetDetector, "run_tiles") and hasattr(CtdetDetector, "run_tiles_stream")
    assert not hasattr(BaseDetector, "run_tiles") and not hasattr(BaseDetector, "run_tiles_stream")
    ok = _detector()
    assert ok._tiles_args(None, None, 32, None) == ((32, 32), (8.0, 8.0), 32, 100)
    for det, word in ((_detector(fix_res=False), "keep_res"), (_detector(scales=(1.0, 0.5)), "test scale"),
                      (_detector(scales=(0.5,)), "test scale"), (_detector(flip_test=True), "flip_test")):
        with pytest.raises(ValueError, match=word):
            det.run_tiles([np.zeros((200, 296, 3), np.uint8)])
        with pytest.raises(ValueError, match=word):
            list(det.run_tiles_stream([[np.zeros((200, 296, 3), np.uint8)]]))
    for kw, word in ((dict(overlap=65), "overlap"), (dict(margin=-1), "margin"), (dict(tile_batch=0), "tile_batch"),
                     (dict(max_per_frame=0), "max_per_frame")):
        with pytest.raises(ValueError, match=word):
            ok.run_tiles([np.zeros((200, 296, 3), np.uint8)], **kw)
    mixed = [np.zeros((10, 12, 3), np.uint8), np.zeros((10, 13, 3), np.uint8)]
    with pytest.raises(ValueError, match="one size"):
        ok.run_tiles(mixed)
    import torch
    with pytest.raises(ValueError, match="host frames"):
        ok.run_tiles(torch.zeros((1, 200, 296, 3), dtype=torch.uint8))
    # min_score: a finite number or None, keyword only, pose only
    for bad in (float("nan"), float("inf"), -float("inf"), "0.1", True, [0.1]):
        with pytest.raises(ValueError, match="min_score"):
            ok.run_tiles(mixed[:1], min_score=bad)
        with pytest.raises(ValueError, match="min_score"):
            list(ok.run_tiles_stream([mixed[:1]], min_score=bad))
    assert MultiPoseDetector._tiles_min_score(None) is None
    assert MultiPoseDetector._tiles_min_score(np.float32(0.25)) == 0.25 and MultiPoseDetector._tiles_min_score(0) == 0.0
    with pytest.raises(TypeError):
        ok.run_tiles(mixed[:1], None, None, 32, None, 'bgr', False, 0.1)
    ctdet = CtdetDetector.__new__(CtdetDetector)
    with pytest.raises(TypeError):
        ctdet.run_tiles(mixed[:1], min_score=0.1)


def test_host_tail_is_post_batch_and_the_specification():
    """_tiles_host_tail on raw detections == _post_batch with the tile metas + the specification per frame"""
    rng = np.random.RandomState(5)
    det = _detector(K=12)
    g = tiles.tile_grid(200, 296, 128, 128, 32)
    B = 2
    dets = np.zeros((B * g.T, 12, 40), F32)
    ctr = rng.uniform(2, 30, (B * g.T, 12, 2))
    wh = rng.uniform(1, 6, (B * g.T, 12, 2))
    dets[:, :, 0:2], dets[:, :, 2:4] = ctr - wh, ctr + wh
    dets[:, :, 4] = rng.randint(1, 50, (B * g.T, 12)) / 50.0
    dets[:, :, 5:39] = rng.uniform(0, 32, (B * g.T, 12, 34))
    metas = tiles.tile_maps(g, 4)[0]
    posts = det._post_batch(dets, metas * B, 1.0)
    for kw in (dict(), dict(min_score=0.3), dict(arrays=True), dict(min_score=0.5, arrays=True)):
        got = det._tiles_host_tail(dets, g, B, 9, **kw)
        assert len(got) == B
        for b in range(B):
            want = multi_pose_tiles_results([p[1] for p in posts[b * g.T:(b + 1) * g.T]], g.cores, False, 9,
                                            kw.get('min_score'))[1]
            assert sorted(got[b]) == [1]
            if kw.get('arrays'):
                assert isinstance(got[b][1], np.ndarray) and np.array_equal(_bits(got[b][1]), _bits(want))
            else:
                assert got[b][1] == want.tolist()
            assert 9 <= len(want) < g.T * 12


# ------------------------------------------------------------------------------------------------
# 4. the prototypes
# ------------------------------------------------------------------------------------------------
def test_pose_tiles_merge_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "centernet_amd.h")).read()
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert "size_t cn_multi_pose_tiles_merge_workspace_bytes(int B, int T, int K);" in plain
    assert ("int cn_multi_pose_tiles_merge_f32(const float *rows, int B, int T, int K, const float *cores_dev, "
            "int apply_nms, int max_per_frame, float min_score, float *out_rows, int32_t *out_counts, "
            "int32_t *status, void *workspace, size_t workspace_bytes, void *stream);") in plain
    cap = int(re.search(r"#define CN_POSE_TILES_MAX_ROWS (\d+)", src).group(1))
    assert cap == native.POSE_TILES_MAX_ROWS and cap >= 4096 and cap % 64 == 0
    one = int(re.search(r"#define CN_POSE_TILES_ONE_WAVE_ROWS (\d+)", src).group(1))
    assert one == native.POSE_TILES_ONE_WAVE_ROWS and 64 <= one < cap
    # the LDS budget the header states: 28.125 bytes per row next to the static words, within 160 KB
    assert cap * 28 + cap // 8 + 10 * 1024 <= 160 * 1024
    lib = native.lib()
    vp, i, sz, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    assert lib.cn_multi_pose_tiles_merge_f32.restype is i
    assert list(lib.cn_multi_pose_tiles_merge_f32.argtypes) == [vp, i, i, i, vp, i, i, f, vp, vp, vp, vp, sz, vp]
    assert lib.cn_multi_pose_tiles_merge_workspace_bytes.restype is sz
    need = lib.cn_multi_pose_tiles_merge_workspace_bytes(2, 60, 100)        # host-side answers need no device
    assert need > 0 and need % 16 == 0 and lib.cn_multi_pose_tiles_merge_workspace_bytes(2, 0, 100) == 0
    assert lib.cn_multi_pose_tiles_merge_f32(None, 1, 1, 1, None, 0, 1, 0.0, None, None, None, None, 0, None) == -5
