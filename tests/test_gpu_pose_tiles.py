"""multi_pose run_tiles on the GPU: cn_multi_pose_tiles_merge_f32 against its host specification
(post_process.multi_pose_tiles_results) bit for bit on seeded 39-column rows -- the smallest shapes that reach
every path of the kernel, the long segment and the survivor cap -- and against cn_multi_pose_merge_f32, the
one-wave form, on the same rows; then the tile pipe against the host tail on the same raw detections,
_run_tiles_sync, the stream, NV12, run_frames (one tile per frame), --fp16 and its hand-back route."""
import contextlib
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth, tiles
from centernet_amd import image as I
from centernet_amd.post_process import multi_pose_tiles_results

pytestmark = pytest.mark.gpu
OK, SHAPE, WORKSPACE, NULL = 0, -1, -3, -5
F32 = np.float32
INF = np.array([-np.inf, -np.inf, np.inf, np.inf], F32)
CAP = native.POSE_TILES_MAX_ROWS
WG = 1024                        # threads of the merge kernel's workgroup
ONE = native.POSE_TILES_ONE_WAVE_ROWS


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# 1. the kernel
# ------------------------------------------------------------------------------------------------
def _merge(rows, B, T, cores, nms, cap, min_score=None, bad=()):
    """the call on rows (B * T, K, 39) -> (rc, out_rows, out_counts, status); ``bad``: arguments replaced for the
    refusal test"""
    lib = native.lib()
    K = rows.shape[1]
    a = dict(rows=torch.from_numpy(rows).cuda(), cores=torch.from_numpy(np.ascontiguousarray(cores, F32)).cuda(),
             T=T, K=K, out_rows=torch.full((B, T * K, 39), -7.0, device="cuda"),
             out_counts=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
             status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    need = int(lib.cn_multi_pose_tiles_merge_workspace_bytes(B, T, K))
    a.update(ws=torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda"), ws_bytes=need)
    outs = (a['out_rows'], a['out_counts'], a['status'])          # (a refused call is given None for one of them)
    a.update(dict(bad))
    rc = lib.cn_multi_pose_tiles_merge_f32(native.ptr(a['rows']), B, a['T'], a['K'], native.ptr(a['cores']), int(nms),
                                           cap, float("nan") if min_score is None else float(min_score),
                                           native.ptr(a['out_rows']), native.ptr(a['out_counts']),
                                           native.ptr(a['status']), native.ptr(a['ws']), a['ws_bytes'],
                                           native.stream_ptr())
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in outs)


def _check_frame(out_rows, out_count, want, what=""):
    assert out_count == len(want), what
    assert np.array_equal(_bits(out_rows[:out_count]), _bits(want)), what
    assert (out_rows[out_count:] == -7).all(), what               # nothing is written behind the count


def _run_case(rows, B, T, cores, nms, cap, min_score=None):
    """the kernel on (B * T, K, 39) rows == the specification, frame by frame -> the specification's rows"""
    rc, out_rows, out_counts, status = _merge(rows, B, T, cores, nms, cap, min_score)
    assert rc == OK and (status == 0).all()
    wants = []
    for b in range(B):
        want = multi_pose_tiles_results(list(rows[b * T:(b + 1) * T].copy()), cores, nms, cap, min_score)[1]
        _check_frame(out_rows[b], out_counts[b], want, b)
        wants.append(want)
    return wants, out_rows, out_counts


def _row(cx, cy, w, h, score, tag=0.0):
    r = np.empty((39,), F32)
    r[:5] = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score]
    r[5:] = F32(tag) + np.arange(34, dtype=F32) / 64
    return r


def _clustered(rng, n, spread=600.0):
    """(n, 39): the boxes of ``_clustered`` in tests/test_gpu_tiles.py -- twelve dense clusters, scores on 400
    levels (1 % of them below 0.01: soft-NMS discards their overlapped rows) -- with seeded joints"""
    c = rng.uniform(0, spread, (12, 2))[rng.randint(0, 12, n)] + rng.normal(0, 3.0, (n, 2))
    wh = rng.uniform(8, 50, (n, 2))
    rows = np.empty((n, 39), F32)
    rows[:, 0:2], rows[:, 2:4] = c - wh / 2, c + wh / 2
    rows[:, 4] = rng.randint(1, 400, n) / F32(400)
    rows[:, 5:] = rng.uniform(-50, 700, (n, 34))
    return rows


def test_pass_through():
    """B = 2, T = 1, K = 8 without nms: the rows of a short tile are followed by NaN rows, which no core keeps"""
    rng = np.random.RandomState(1)
    rows = np.full((2, 8, 39), np.nan, F32)
    rows[0], rows[1, :5] = _clustered(rng, 8), _clustered(rng, 5)
    wants, out_rows, out_counts = _run_case(rows, 2, 1, INF[None], False, 100)
    assert out_counts.tolist() == [8, 5]
    for b, n in enumerate((8, 5)):
        assert np.array_equal(_bits(out_rows[b, :n]), _bits(rows[b, :n]))


def _duplicate_rows():
    """B = 2, T = 4, K = 8: people on and next to the boundaries of a 2 x 2 grid, every tile listing the people
    whose centre lies on its pixels with their own numbers -- a person in an overlap is an exact duplicate in two
    or four tiles -> (grid, rows (B * T, K, 39), the people of every frame)"""
    rng = np.random.RandomState(2)
    B, K = 2, 8
    grid = tiles.tile_grid(200, 200, 128, 128, 32, 4)   # 2 x 2, boundaries x = 100 and y = 100, margin 4
    assert grid.T == 4 and grid.origins == [(0, 0), (0, 72), (72, 0), (72, 72)]
    rows = np.full((B * grid.T, K, 39), np.nan, F32)
    frames = []
    for b in range(B):
        people = []
        for i, (cx, cy) in enumerate([(100, 40), (30, 100), (150, 160), (104, 98)]):
            people.append(_row(cx, cy, 30, 24, 0.3 + 0.05 * i, 10 * b + i))
            # a partial overlap next to it, and for some a near-copy that soft-NMS decays below the threshold
            people.append(_row(cx + rng.uniform(-6, 6), cy + rng.uniform(-6, 6), 26, 28, 0.2 + 0.04 * i, 100 + i))
            if i % 3 == 0:
                people.append(_row(cx + 0.25, cy, 30, 24, 0.003, 200 + i))
        for t, (y0, x0) in enumerate(grid.origins):
            mine = [r for r in people if x0 <= (r[0] + r[2]) / 2 < x0 + 128 and y0 <= (r[1] + r[3]) / 2 < y0 + 128]
            assert 0 < len(mine) <= K
            rows[b * grid.T + t, :len(mine)] = mine
        frames.append(people)
    return grid, rows, frames


def test_cross_tile_duplicates():
    grid, rows, frames = _duplicate_rows()
    wants, _, _ = _run_case(rows, 2, grid.T, grid.cores, False, 100)
    for b, want in enumerate(wants):
        listed = int(np.isfinite(rows[b * grid.T:(b + 1) * grid.T, :, 4]).sum())
        assert len(frames[b]) < len(want) < listed      # the cores dropped rows, the margins kept duplicates
        assert (want[:, 4] < 0.001).any()               # ... which soft-NMS decayed


def test_cut_with_tied_scores():
    rng = np.random.RandomState(4)
    B, T, K, cap = 2, 4, 32, 20
    rows = np.full((B * T, K, 39), np.nan, F32)
    for i in range(B * T):                               # boxes far apart: soft-NMS leaves the score levels alone
        for k in range(K - i % 3):
            rows[i, k] = _row(100.0 * k, 100.0 * i, 10, 10, rng.randint(1, 6) / 8.0, i * K + k)
    wants, _, out_counts = _run_case(rows, B, T, np.tile(INF, (T, 1)), False, cap)
    assert (out_counts >= cap).all() and (out_counts > cap).any()        # ties at the threshold were kept
    _run_case(rows, B, T, np.tile(INF, (T, 1)), True, 1)


@pytest.mark.parametrize("T,K", [(3, 16), (16, 128)])
def test_against_the_one_wave_merge(T, K):
    """infinite cores, nms on, no cut: out_rows == cn_multi_pose_merge_f32 with the tiles as S = T test scales"""
    rng = np.random.RandomState(40 + T)
    B = 2
    rows = _clustered(rng, B * T * K).reshape(B * T, K, 39)
    assert T * K <= native.MERGE_MAX_ROWS
    wants, out_rows, out_counts = _run_case(rows, B, T, np.tile(INF, (T, 1)), True, T * K)
    assert out_counts.tolist() == [T * K] * B
    scales = torch.from_numpy(np.ascontiguousarray(rows.reshape(B, T, K, 39).transpose(1, 0, 2, 3))).cuda()
    merged = torch.full((B, T * K, 39), -7.0, device="cuda")
    native.check(native.lib().cn_multi_pose_merge_f32(native.ptr(scales), T, B, K, 1, native.ptr(merged),
                                                      native.stream_ptr()), "cn_multi_pose_merge_f32")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out_rows), _bits(merged.cpu().numpy()))


@pytest.mark.parametrize("n", [63, 64, 65, ONE - 1, ONE, ONE + 1, WG - 1, WG, WG + 1])
def test_ragged_survivor_counts(n):
    """exactly n survivors out of T * 128 rows: the ragged last turns of the chunked loops, and both sides of the
    segment length at which the soft-NMS goes from one wave to the workgroup"""
    rng = np.random.RandomState(500 + n)
    K, B = 128, 2
    T = -(-(n + 40) // K)
    core = np.array([-100, -100, 400, 400], F32)
    rows = _clustered(rng, B * T * K, spread=250.0).reshape(B, T * K, 39)
    for b in range(B):
        out = rng.permutation(T * K)[n:]                 # these lie outside every core
        rows[b, out, 0] += 5000
        rows[b, out, 2] += 5000
    rows = rows.reshape(B * T, K, 39)
    wants, _, out_counts = _run_case(rows, B, T, np.tile(core, (T, 1)), True, 2 * WG)
    assert out_counts.tolist() == [n, n]
    _run_case(rows, B, T, np.tile(core, (T, 1)), True, n - 7)


def test_long_segment():
    """3072 survivors per frame, above the 2048 of the one-wave form; the discard walk runs, its last-row case
    included"""
    rng = np.random.RandomState(6)
    B, T, K = 2, 24, 128
    n = T * K
    assert n == 3072 > native.MERGE_MAX_ROWS
    rows = _clustered(rng, B * n).reshape(B * T, K, 39)
    for b in range(B):                                   # the precondition, on the host
        host = rows[b * T:(b + 1) * T].reshape(n, 39).copy()
        kept = native.lib().cn_soft_nms_f32(host.ctypes.data, n, 39, 0.5, 0.5, 0.001, 2)
        assert 0 < kept <= n - 16
        # a row behind the kept count with a score below the threshold was discarded AS the last live row (it
        # took its own decayed score); every other discard leaves a live row's score (>= 0.001) behind
        assert (host[kept:, 4] < 0.001).any()
    _run_case(rows, B, T, np.tile(INF, (T, 1)), False, 100)
    _run_case(rows, B, T, np.tile(INF, (T, 1)), False, n)


def test_overflow_sets_the_status_of_its_frame_only():
    rng = np.random.RandomState(7)
    K, B = 128, 2
    T = -(-(CAP + 1) // K)
    core = np.array([-100, -100, 700, 700], F32)
    rows = _clustered(rng, B * T * K).reshape(B, T * K, 39)
    for b, n in enumerate((CAP + 1, CAP)):               # frame 0: one survivor too many; frame 1: exactly the cap
        rows[b, n:, 0] += 5000
        rows[b, n:, 2] += 5000
    rows = rows.reshape(B * T, K, 39)
    cores = np.tile(core, (T, 1))
    rc, out_rows, out_counts, status = _merge(rows, B, T, cores, False, 100)
    assert rc == OK and status.tolist() == [1, 0] and out_counts[0] == 0
    want = multi_pose_tiles_results(list(rows[T:].copy()), cores, False, 100)[1]
    _check_frame(out_rows[1], out_counts[1], want)


def test_min_score():
    rng = np.random.RandomState(8)
    B, T, K = 2, 2, 8
    rows = _clustered(rng, B * T * K).reshape(B * T, K, 39)
    rows[:, :, 4] = rng.randint(1, 5, (B * T, K)) / F32(8)       # equal scores: 0.125 ... 0.5
    rows[0, 3, 4] = rows[2, 0, 4] = rows[3, 7, 4] = np.nan
    cores = np.tile(INF, (T, 1))
    for min_score in (0.25, 0.2500001, 0.125, -1e30, 1.0):
        wants, _, out_counts = _run_case(rows, B, T, cores, False, 100, min_score)
        assert all(np.isfinite(w[:, 4]).all() for w in wants)    # the NaN scores fail any threshold
    assert _run_case(rows, B, T, cores, False, 100, 1.0)[2].tolist() == [0, 0]
    eq = _run_case(rows, B, T, cores, False, 100, 0.25)[2]
    above = _run_case(rows, B, T, cores, False, 100, 0.2500001)[2]
    assert (eq > above).all()                                    # score == min_score is kept


def test_argument_errors_launch_nothing():
    lib = native.lib()
    B, T, K = 1, 2, 8
    rows = _clustered(np.random.RandomState(9), T * K).reshape(T, K, 39)
    cores = np.tile(INF, (T, 1))

    def call(**bad):
        rc, out_rows, out_counts, status = _merge(rows, B, T, cores, False, 100, None, bad)
        if rc != OK:                                    # nothing ran: the outputs hold their fill
            assert (out_rows == -7).all() and (out_counts == -7).all() and (status == -7).all()
        return rc
    assert call() == OK
    for name in ("rows", "cores", "out_rows", "out_counts", "status", "ws"):
        assert call(**{name: None}) == NULL, name
    need = int(lib.cn_multi_pose_tiles_merge_workspace_bytes(B, T, K))
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    # the limits: T * K rows per frame, K rows per tile (the arrays are never touched: the refusal comes first)
    assert call(T=native.TILES_MAX_ROWS // K + 1) == SHAPE
    assert call(K=129) == SHAPE and call(T=0) == SHAPE
    assert _merge(rows, B, T, cores, False, 0)[0] == SHAPE


# ------------------------------------------------------------------------------------------------
# 2. the tile pipe
# ------------------------------------------------------------------------------------------------
def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _detector(extra=()):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["multi_pose", "--arch", "dla_34", "--input_h", "128", "--input_w", "128"] + list(extra))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


@pytest.fixture(scope="module")
def pose(dev):
    return _detector()


def _same(a, b, what=""):
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb) == [1]
        x, y = np.asarray(ra[1], F32).reshape(-1, 39), np.asarray(rb[1], F32).reshape(-1, 39)
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i)


def _pipe_equals_the_host_tail(det):
    """two 200 x 296 frames, overlap 32, tile_batch 8: T = 6, chunks of 8 + 4 tiles"""
    det.tail_fallbacks = 0
    frames = [_img(200, 296, 10), _img(200, 296, 11)]
    args = det._tiles_args(32, None, 8, None)
    pipe = det._tile_pipe_for(frames, 1, *args, 'bgr', min_score=None)
    assert pipe.tail is not None and (pipe.T, pipe.N, pipe.C) == (6, 12, 8)
    assert [(lv.lo, lv.n) for lv in pipe.levels] == [(0, 8), (8, 4)]
    seen, run_scale = [], det._run_scale

    def spy(batch, flip, **kw):                          # every chunk's raw detections as they ran
        dets = run_scale(batch, flip, **kw)
        seen.append(dets.clone())
        return dets
    det._run_scale = spy
    try:
        pipe.submit(0, frames)
        got = pipe.collect(0, frames)
    finally:
        del det._run_scale
    assert len(seen) == 2
    raw = np.concatenate([d.cpu().numpy()[:lv.n] for d, lv in zip(seen, pipe.levels)], axis=0)
    assert det.range_ok()
    _same(got, det._tiles_host_tail(raw, pipe.grid, 2, pipe.max_per_frame), "host tail on the same detections")
    assert all(isinstance(r[1], list) and len(r[1]) > 0 for r in got)
    assert det.tail_fallbacks == 0
    return frames, args, got


def test_pipe_equals_host_tail_sync_path_and_arrays(dev, pose):
    det = pose
    frames, args, got = _pipe_equals_the_host_tail(det)
    _same(det.run_tiles(frames, overlap=32, tile_batch=8), got, "run_tiles")
    _same(got, det._run_tiles_sync(frames, *args), "_run_tiles_sync")
    arr = det.run_tiles(frames, overlap=32, tile_batch=8, arrays=True)
    assert all(isinstance(r[1], np.ndarray) and r[1].dtype == F32 and r[1].shape[1] == 39 for r in arr)
    _same(arr, got, "arrays")
    # min_score: a pipe of its own, the host tail with the same threshold
    some = det.run_tiles(frames, overlap=32, tile_batch=8, arrays=True, min_score=0.1)
    _same(some, det._run_tiles_sync(frames, *args, min_score=0.1), "min_score")
    assert det.tail_fallbacks == 0


def test_pipe_equals_host_tail_fp16(dev):
    _pipe_equals_the_host_tail(_detector(["--fp16"]))


def test_stream_equals_run_tiles(dev, pose):
    pose.tail_fallbacks = 0
    batches = [[_img(200, 296, 30 + 2 * k), _img(200, 296, 31 + 2 * k)] for k in range(3)]
    alone = [pose.run_tiles(b, overlap=32, tile_batch=8) for b in batches]
    streamed = list(pose.run_tiles_stream(iter(batches), depth=2, overlap=32, tile_batch=8))
    assert len(streamed) == 3
    for a, s in zip(alone, streamed):
        _same(s, a)
    with pytest.raises(ValueError, match="one size"):
        list(pose.run_tiles_stream(iter([batches[0], batches[1][:1]]), overlap=32, tile_batch=8))
    assert pose.tail_fallbacks == 0


def test_nv12_frames(dev, pose):
    pose.tail_fallbacks = 0
    nv12 = [I.bgr_to_nv12(_img(200, 296, 40 + i)) for i in range(2)]
    got = pose.run_tiles(nv12, overlap=32, tile_batch=8, pixel_format='nv12')
    _same(got, pose.run_tiles([I.nv12_to_bgr(f) for f in nv12], overlap=32, tile_batch=8))
    assert pose.tail_fallbacks == 0


def test_one_tile_per_frame_equals_run_frames(dev, pose):
    frames = [_img(128, 128, 20 + i) for i in range(3)]
    pose.tail_fallbacks = 0
    assert pose.max_per_image >= pose.opt.K
    _same(pose.run_tiles(frames, tile_batch=len(frames)), pose.run_frames(frames))
    _same(pose.run_tiles(frames, tile_batch=len(frames), arrays=True), pose.run_frames(frames, arrays=True))
    assert pose.tail_fallbacks == 0


def test_status_hands_the_batch_back(dev, pose):
    """A frame of 56 tiles whose prepared rows all lie inside their tiles' cores: 5600 survivors, above the cap of
    the merge.  The tail reports it, the pipe runs the batch through _run_tiles_sync and counts it."""
    det = pose
    det.tail_fallbacks = 0
    frames = [_img(896, 1024, 50)]
    args = det._tiles_args(0, None, 32, None)
    pipe = det._tile_pipe_for(frames, 1, *args, 'bgr', min_score=None)
    K = det.opt.K
    assert (pipe.T, pipe.C, len(pipe.levels)) == (56, 32, 2) and pipe.T * K > CAP
    pipe.submit(0, frames)
    torch.cuda.synchronize()
    rows = np.zeros((56, K, 39), F32)
    for t, (y0, x0) in enumerate(pipe.grid.origins):
        rows[t, :, :5] = [x0 + 54.0, y0 + 54.0, x0 + 74.0, y0 + 74.0, 0.5]
    rows[:, :, 4] = np.linspace(0.1, 0.9, 56 * K, dtype=F32).reshape(56, K)
    pipe.tail.tile_rows.copy_(torch.from_numpy(rows))
    pipe.tail.finish(0)
    pipe.ev_done[0].record()
    torch.cuda.synchronize()
    assert pipe.tail.host('status', 0).numpy().tolist() == [1] and pipe.tail.results(0, 1) is None
    assert pipe.tail.host('counts', 0).numpy().tolist() == [0]
    got = pipe.collect(0, frames)
    assert det.tail_fallbacks == 1
    _same(got, det._run_tiles_sync(frames, *args), "_run_tiles_sync")
