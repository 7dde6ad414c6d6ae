"""run_tiles on the GPU: cn_ctdet_tiles_merge_f32 against its host restatement (post_process.ctdet_tiles_results)
bit for bit on seeded rows -- the smallest shapes that reach every path of the three launches -- and the tile
pipe against the single-image pre-process (its batches), the host tail on the same raw detections (its
results), _run_tiles_sync, run_frames (one tile per frame) and its hand-back route."""
import contextlib
import ctypes
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth, tiles
from centernet_amd import image as I
from centernet_amd.post_process import ctdet_tiles_results

pytestmark = pytest.mark.gpu
OK, SHAPE, WORKSPACE, NULL = 0, -1, -3, -5
INF = np.array([-np.inf, -np.inf, np.inf, np.inf], np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------
def _pack(tile_lists, K, nc):
    """[image][(class, row)] in any order -> rows (N, K, 5) / bounds (N, nc + 1) as cn_ctdet_post_process_f32
    leaves them (grouped by class, a class's rows in their order, NaN behind the last bound) and the per-image
    {class: rows} of the host side"""
    N = len(tile_lists)
    rows = np.full((N, K, 5), np.nan, np.float32)
    bounds = np.zeros((N, nc + 1), np.int32)
    dicts = []
    for i, items in enumerate(tile_lists):
        assert len(items) <= K
        cls = np.array([c for c, _ in items], np.int64).reshape(-1)
        r = np.array([row for _, row in items], np.float32).reshape(-1, 5)
        order = np.argsort(cls, kind='stable')
        cls, r = cls[order], r[order]
        rows[i, :len(r)] = r
        bounds[i] = np.searchsorted(cls, np.arange(nc + 1))
        dicts.append({j + 1: r[bounds[i, j]:bounds[i, j + 1]].copy() for j in range(nc)})
    return rows, bounds, dicts


def _merge(rows, bounds, B, T, nc, cores, nms, cap, bad=()):
    """the call -> (rc, out_rows, out_bounds, status); ``bad``: arguments replaced for the refusal test"""
    lib = native.lib()
    K = rows.shape[1]
    a = dict(rows=torch.from_numpy(rows).cuda(), bounds=torch.from_numpy(bounds).cuda(),
             cores=torch.from_numpy(np.ascontiguousarray(cores, np.float32)).cuda(), T=T, K=K,
             out_rows=torch.full((B, T * K, 5), -7.0, device="cuda"),
             out_bounds=torch.full((B, nc + 1), -7, dtype=torch.int32, device="cuda"),
             status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    need = int(lib.cn_ctdet_tiles_merge_workspace_bytes(B, T, K, nc))
    a.update(ws=torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda"), ws_bytes=need)
    outs = (a['out_rows'], a['out_bounds'], a['status'])         # (a refused call is given None for one of them)
    a.update(dict(bad))
    rc = lib.cn_ctdet_tiles_merge_f32(native.ptr(a['rows']), native.ptr(a['bounds']), B, a['T'], a['K'], nc,
                                      native.ptr(a['cores']), int(nms), cap, native.ptr(a['out_rows']),
                                      native.ptr(a['out_bounds']), native.ptr(a['status']), native.ptr(a['ws']),
                                      a['ws_bytes'], native.stream_ptr())
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in outs)


def _check_frame(out_rows, out_bounds, want, nc, what=""):
    assert out_bounds[0] == 0 and out_bounds[nc] == sum(len(v) for v in want.values()), what
    for j in range(nc):
        got = out_rows[out_bounds[j]:out_bounds[j + 1]]
        assert got.shape == want[j + 1].shape, (what, j)
        assert np.array_equal(_bits(got), _bits(want[j + 1])), (what, j)


def _run_case(tile_lists, B, T, K, nc, cores, nms, cap):
    rows, bounds, dicts = _pack(tile_lists, K, nc)
    rc, out_rows, out_bounds, status = _merge(rows, bounds, B, T, nc, cores, nms, cap)
    assert rc == OK and (status == 0).all()
    wants = []
    for b in range(B):
        want = ctdet_tiles_results(dicts[b * T:(b + 1) * T], cores, nc, nms, cap)
        _check_frame(out_rows[b], out_bounds[b], want, nc, b)
        wants.append(want)
    return wants, out_rows, out_bounds


def _box(cx, cy, w, h, score):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score]


def test_pass_through():
    rng = np.random.RandomState(1)
    B, T, K, nc = 2, 1, 8, 3
    lists = [[(int(c), _box(*rng.uniform(10, 90, 2), 8, 8, s)) for c, s in zip(np.sort(rng.randint(0, nc, n)),
                                                                              rng.uniform(0.1, 0.9, n))]
             for n in (8, 5)]
    rows, bounds, _ = _pack(lists, K, nc)
    wants, out_rows, out_bounds = _run_case(lists, B, T, K, nc, INF[None], False, 100)
    for b, n in enumerate((8, 5)):                      # no NMS, cut not reached: the input itself
        assert np.array_equal(out_bounds[b], bounds[b])
        assert np.array_equal(_bits(out_rows[b, :n]), _bits(rows[b, :n]))


def _objects_to_tiles(objects, grid, K):
    """every tile lists the objects whose centre lies on its pixels, with the objects' own numbers: an object in
    an overlap is an exact duplicate in both tiles"""
    out = []
    for y0, x0 in grid.origins:
        items = [(c, box) for c, box in objects
                 if x0 <= (box[0] + box[2]) / 2 < x0 + grid.tw and y0 <= (box[1] + box[3]) / 2 < y0 + grid.th]
        assert len(items) <= K
        out.append(items)
    return out


def test_cross_tile_duplicates():
    rng = np.random.RandomState(2)
    B, K, nc = 2, 16, 3
    grid = tiles.tile_grid(200, 296, 128, 128, 32)      # 2 x 3, boundaries x = 112, 196 and y = 100, margin 8
    assert grid.T == 6
    lists = []
    for b in range(B):
        spots = [(112, 50), (110, 102), (196, 100), (199, 30), (40, 97), (250, 150), (60, 40), (150, 104), (98, 150)]
        objects = []
        for i, (cx, cy) in enumerate(spots):
            c = 1 if b == 1 else i % 2                  # frame 1: every row in one class; class 2 always empty
            objects.append((c, _box(cx, cy, 30, 24, 0.3 + 0.05 * i)))
            # a partial overlap next to it, and for some a near-copy that soft-NMS decays below the threshold
            objects.append((c, _box(cx + rng.uniform(-6, 6), cy + rng.uniform(-6, 6), 26, 28, 0.2 + 0.04 * i)))
            if i % 3 == 0:
                objects.append((c, _box(cx + 0.25, cy, 30, 24, 0.003)))
        lists += _objects_to_tiles(objects, grid, K)
    wants, _, out_bounds = _run_case(lists, B, grid.T, K, nc, grid.cores, True, 100)
    assert (out_bounds[0, 3] - out_bounds[0, 2]) == 0 and out_bounds[1, 1] == 0
    per_tile_rows = sum(len(items) for items in lists[:grid.T])
    assert sum(len(v) for v in wants[0].values()) < per_tile_rows           # the core filter dropped rows ...
    assert sum(len(v) for v in wants[0].values()) > 9 * 2 + 3               # ... and the margins kept duplicates


@pytest.mark.parametrize("margin", [0, 4])
def test_core_edges(margin):
    grid = tiles.tile_grid(128, 224, 128, 128, 32, margin)                # two tiles, boundary x = 112
    lo, hi = np.float32(112 - margin), np.float32(112 + margin)
    xs = [lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(0)), np.float32(112), np.float32(20),
          np.float32(200), np.float32("nan")]
    items = [(i % 2, _box(np.float32(x), np.float32(64), np.float32(10), np.float32(10), 0.5 + 0.01 * i))
             for i, x in enumerate(xs)]
    wants, _, _ = _run_case([items, items], 1, 2, 8, 2, grid.cores, False, 100)
    n = sum(len(v) for v in wants[0].values())
    # tile 0 keeps x < hi, tile 1 keeps x >= lo; the NaN centre is kept by nobody
    assert n == sum(1 for x in xs if x < hi) + sum(1 for x in xs if x >= lo)


def test_cut_with_ties():
    rng = np.random.RandomState(4)
    B, T, K, nc, cap = 2, 4, 32, 3, 20
    lists = []
    for i in range(B * T):                               # boxes far apart: soft-NMS leaves the score levels alone
        lists.append([(int(rng.randint(0, nc)), _box(100.0 * k, 100.0 * (i % T), 10, 10, rng.randint(1, 6) / 8.0))
                      for k in range(K - i % 3)])
    cores = np.tile(INF, (T, 1))
    wants, _, _ = _run_case(lists, B, T, K, nc, cores, False, cap)
    for want in wants:
        assert sum(len(v) for v in want.values()) > cap  # ties at the threshold were kept


def _clustered(rng, n, classes):
    c = rng.uniform(0, 600, (12, 2))[rng.randint(0, 12, n)] + rng.normal(0, 3.0, (n, 2))
    wh = rng.uniform(8, 50, (n, 2))
    score = rng.randint(1, 400, n) / np.float32(400)
    return [(int(k), [x - w / 2, y - h / 2, x + w / 2, y + h / 2, s])
            for k, (x, y), (w, h), s in zip(classes, c, wh, score)]


def test_above_the_row_cap_of_the_scale_merge():
    rng = np.random.RandomState(5)
    B, T, K, nc = 2, 24, 128, 4
    assert T * K == 3072 > native.MERGE_MAX_ROWS
    lists = [_clustered(rng, K, np.arange(K) % nc) for _ in range(B * T)]     # 768 rows per class and frame
    _run_case(lists, B, T, K, nc, np.tile(INF, (T, 1)), False, 100)


def test_class_overflow_sets_the_status_of_its_frame_only():
    rng = np.random.RandomState(6)
    B, T, K, nc = 2, 21, 128, 4
    lists = [_clustered(rng, K, np.zeros(K, int)) for _ in range(T)]          # frame 0: 2688 rows of class 0
    # frame 1: class 0 with exactly CN_MERGE_MAX_ROWS rows (16 tiles), the other classes share the rest
    lists += [_clustered(rng, K, np.zeros(K, int) if t < 16 else 1 + np.arange(K) % 3) for t in range(T)]
    rows, bounds, dicts = _pack(lists, K, nc)
    cores = np.tile(INF, (T, 1))
    rc, out_rows, out_bounds, status = _merge(rows, bounds, B, T, nc, cores, False, 100)
    assert rc == OK and status[0] != 0 and status[1] == 0
    assert (out_bounds[0] == 0).all()
    want = ctdet_tiles_results(dicts[T:], cores, nc, False, 100)
    _check_frame(out_rows[1], out_bounds[1], want, nc)


def test_argument_errors_launch_nothing():
    lib = native.lib()
    B, T, K, nc = 1, 2, 8, 3
    rows, bounds, _ = _pack([[(0, _box(5, 5, 2, 2, 0.5))]] * 2, K, nc)
    cores = np.tile(INF, (T, 1))

    def call(**bad):
        rc, out_rows, out_bounds, status = _merge(rows, bounds, B, T, nc, cores, False, 100, bad)
        if rc != OK:                                    # nothing ran: the outputs hold their fill
            assert (out_rows == -7).all() and (out_bounds == -7).all() and (status == -7).all()
        return rc
    assert call() == OK
    for name in ("rows", "bounds", "cores", "out_rows", "out_bounds", "status", "ws"):
        assert call(**{name: None}) == NULL, name
    need = int(lib.cn_ctdet_tiles_merge_workspace_bytes(B, T, K, nc))
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    # the limits: T * K rows per frame, K rows per tile (the arrays are never touched: the refusal comes first)
    assert call(T=native.TILES_MAX_ROWS // K + 1) == SHAPE
    assert call(K=129) == SHAPE and call(T=0) == SHAPE
    assert lib.cn_ctdet_tiles_merge_workspace_bytes(1, 512, 128, 80) > 0      # T * K at the cap is taken


# ------------------------------------------------------------------------------------------------
# 2. the tile pipe
# ------------------------------------------------------------------------------------------------
def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def ctdet(dev):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet", "--arch", "resdcn_18", "--input_h", "128", "--input_w", "128"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


def _same(a, b, what=""):
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb)
        for j in ra:
            x, y = np.asarray(ra[j], np.float32), np.asarray(rb[j], np.float32)
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i, j)


def test_ragged_last_chunk(dev, ctdet):
    det = ctdet
    det.tail_fallbacks = 0
    frames = [_img(200, 296, 10), _img(200, 296, 11)]
    args = det._tiles_args(32, None, 8, None)
    pipe = det._tile_pipe_for(frames, 1, *args, 'bgr')
    assert pipe.tail is not None and (pipe.T, pipe.N, pipe.C) == (6, 12, 8)
    assert [(lv.lo, lv.n) for lv in pipe.levels] == [(0, 8), (8, 4)]
    seen, run_scale = [], det._run_scale

    def spy(batch, flip, **kw):                          # every chunk's batch and raw detections as they ran
        dets = run_scale(batch, flip, **kw)
        seen.append((batch.clone(), dets.clone()))
        return dets
    det._run_scale = spy
    try:
        pipe.submit(0, frames)
        got = pipe.collect(0, frames)
    finally:
        del det._run_scale
    assert len(seen) == 2 and all(b.shape == (8, 3, 128, 128) for b, _ in seen)
    # (a) every chunk batch == the single-image pre-process of its tiles; the surplus slices are zero
    lib = native.lib()
    mean = (ctypes.c_float * 3)(*[float(v) for v in det.mean.reshape(-1)])
    std = (ctypes.c_float * 3)(*[float(v) for v in det.std.reshape(-1)])
    dst_to_src = tiles.tile_maps(pipe.grid, det.opt.down_ratio)[1]
    for (batch, _), lv in zip(seen, pipe.levels):
        for j in range(lv.n):
            b, t = divmod(lv.lo + j, pipe.T)
            frame = torch.from_numpy(frames[b]).cuda()
            one = torch.full((1, 3, 128, 128), float("nan"), device=dev)
            native.check(lib.cn_warp_normalize_u8_f32(native.ptr(frame), 200, 296, 296 * 3,
                                                      (ctypes.c_double * 6)(*dst_to_src[t]), 128, 128, mean, std, 0,
                                                      native.ptr(one), native.stream_ptr()), "warp")
            assert torch.equal(batch[j:j + 1].view(torch.int32), one.view(torch.int32)), (lv.lo, j)
        assert (batch[lv.n:] == 0).all()
    # (b) the results == the host tail on the same raw detections
    raw = np.concatenate([d.cpu().numpy()[:lv.n] for (_, d), lv in zip(seen, pipe.levels)], axis=0)
    assert det.range_ok()
    _same(got, det._tiles_host_tail(raw, pipe.grid, 2, pipe.max_per_frame), "host tail on the same detections")
    assert sum(len(v) for r in got for v in r.values()) > 0
    # (c) the public entry and the synchronous path
    _same(det.run_tiles(frames, overlap=32, tile_batch=8), got, "run_tiles")
    _same(got, det._run_tiles_sync(frames, *args), "_run_tiles_sync")
    assert det.tail_fallbacks == 0


def test_one_tile_per_frame_equals_run_frames(dev, ctdet):
    frames = [_img(128, 128, 20 + i) for i in range(3)]
    ctdet.tail_fallbacks = 0
    _same(ctdet.run_tiles(frames, tile_batch=len(frames)), ctdet.run_frames(frames))
    assert ctdet.tail_fallbacks == 0


def test_stream_equals_run_tiles(dev, ctdet):
    batches = [[_img(200, 296, 30 + 2 * k), _img(200, 296, 31 + 2 * k)] for k in range(3)]
    alone = [ctdet.run_tiles(b, overlap=32, tile_batch=8) for b in batches]
    streamed = list(ctdet.run_tiles_stream(iter(batches), depth=2, overlap=32, tile_batch=8))
    assert len(streamed) == 3
    for a, s in zip(alone, streamed):
        _same(s, a)
    with pytest.raises(ValueError, match="one size"):
        list(ctdet.run_tiles_stream(iter([batches[0], batches[1][:1]]), overlap=32, tile_batch=8))


def test_nv12_frames(dev, ctdet):
    nv12 = [I.bgr_to_nv12(_img(200, 296, 40 + i)) for i in range(2)]
    got = ctdet.run_tiles(nv12, overlap=32, tile_batch=8, pixel_format='nv12')
    _same(got, ctdet.run_tiles([I.nv12_to_bgr(f) for f in nv12], overlap=32, tile_batch=8))


def test_status_hands_the_batch_back(dev, ctdet):
    """A frame of 25 tiles whose prepared rows are all of class 0 and all inside their tiles' cores: 2500
    survivors in one segment, above the 2048 of one soft-NMS.  The tail reports it, the pipe runs the batch
    through _run_tiles_sync and counts it."""
    det = ctdet
    det.tail_fallbacks = 0
    frames = [_img(640, 640, 50)]
    args = det._tiles_args(0, None, 32, None)
    pipe = det._tile_pipe_for(frames, 1, *args, 'bgr')
    K, nc = det.opt.K, det.opt.num_classes
    assert (pipe.T, pipe.C, len(pipe.levels)) == (25, 25, 1) and pipe.T * K > native.MERGE_MAX_ROWS
    pipe.submit(0, frames)
    torch.cuda.synchronize()
    assert pipe.tail.results(0, 1) is not None           # the network's own rows fit
    rows = np.zeros((25, K, 5), np.float32)
    for t, (y0, x0) in enumerate(pipe.grid.origins):
        rows[t] = _box(x0 + 64.0, y0 + 64.0, 20.0, 20.0, 0.5)
    rows[:, :, 4] = np.linspace(0.1, 0.9, 25 * K, dtype=np.float32).reshape(25, K)
    bounds = np.zeros((25, nc + 1), np.int32)
    bounds[:, 1:] = K
    pipe.tail.tile_rows.copy_(torch.from_numpy(rows))
    pipe.tail.tile_bounds.copy_(torch.from_numpy(bounds))
    pipe.tail.finish(0)
    pipe.ev_done[0].record()
    torch.cuda.synchronize()
    assert pipe.tail.host('status', 0).numpy().tolist() == [1] and pipe.tail.results(0, 1) is None
    got = pipe.collect(0, frames)
    assert det.tail_fallbacks == 1
    _same(got, det._run_tiles_sync(frames, *args), "_run_tiles_sync")
