"""The tile pyramid of ctdet's run_tiles on the GPU: cn_tile_box_normalize_u8_f32 against image.tile_box_normalize,
the ragged warp (level 0) and the half-size resize + warp (level 1), bit for bit; cn_ctdet_tiles_merge_gated_f32
against post_process.ctdet_pyramid_results and, with open gates, against cn_ctdet_tiles_merge_f32; and the tile
pipe with ``levels`` against the call without them (levels=(0,)), _run_tiles_sync and the host tail."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, tiles
from centernet_amd import image as I
from centernet_amd.post_process import ctdet_pyramid_results

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_tiles import _bits, _box, _check_frame, _clustered, _img, _merge, _pack, _same, ctdet   # noqa: E402,F401

pytestmark = pytest.mark.gpu
OK, SHAPE, WORKSPACE, NULL, ALIGN = 0, -1, -3, -5, -6
INF = np.float32(np.inf)
MEAN, STD = np.float32([0.408, 0.447, 0.47]), np.float32([0.289, 0.274, 0.278])
TH, TW = 16, 24


def _c3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


# ------------------------------------------------------------------------------------------------
# 1. the box kernel
# ------------------------------------------------------------------------------------------------
def _packed(frames, pitches, offsets, size):
    """the frames at their offsets and pitches in one buffer; every byte between them is 255"""
    buf = np.full((size,), 255, np.uint8)
    for f, p, o in zip(frames, pitches, offsets):
        H, W = f.shape[:2]
        assert p >= 3 * W and o + H * p <= size
        for y in range(H):
            buf[o + y * p:o + y * p + 3 * W] = f[y].reshape(-1)
    return buf


def _descs(items):
    """[(offset, H, W, pitch, level, y0, x0)] -> the descriptor table"""
    d = np.zeros((len(items),), native.TILE_BOX_DESC)
    for i, it in enumerate(items):
        d[i] = tuple(it)
    return d


def _box_kernel(buf, descs, th=TH, tw=TW, bad=()):
    """the call -> (rc, out); the output starts as -7 everywhere; ``buf``: a numpy buffer or a device tensor"""
    a = dict(buf=torch.from_numpy(buf).cuda() if isinstance(buf, np.ndarray) else buf,
             descs=torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).cuda(), N=len(descs), th=th, tw=tw,
             mean=_c3(MEAN), std=_c3(STD), out=torch.full((len(descs), 3, th, tw), -7.0, device="cuda"))
    out = a['out']
    a.update(dict(bad))
    rc = native.lib().cn_tile_box_normalize_u8_f32(native.ptr(a['buf']), native.ptr(a['descs']), a['N'], a['th'],
                                                   a['tw'], a['mean'], a['std'], native.ptr(a['out']),
                                                   native.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _spec(frame, level, y0, x0, th=TH, tw=TW):
    return I.tile_box_normalize(frame, level, y0, x0, th, tw, MEAN, STD)


def test_box_kernel_against_the_specification():
    H, W, pitch = 37, 53, 3 * 53 + 5
    frames = [_img(H, W, 60), _img(H, W, 61)]
    offsets = [0, H * pitch + 1]                         # the second frame at an odd byte
    buf = _packed(frames, [pitch] * 2, offsets, offsets[1] + H * pitch + 3)
    where = [(0, 0, 0), (0, 21, 29), (0, 30, 40), (0, -3, -5),      # inside, flush, over the edge, before the origin
             (1, 0, 0), (1, 3, 3), (1, 10, 20),                     # level image 19 x 27: partial blocks on both edges
             (2, 0, 0), (2, 2, 1),                                  # 10 x 14: smaller than the tile
             (3, 0, 0), (3, 1, 2)]                                  # 5 x 7
    items, frame_of = [], []
    for b in range(2):
        for level, y0, x0 in where:
            items.append((offsets[b], H, W, pitch, level, y0, x0))
            frame_of.append(b)
    items.insert(5, (offsets[1], 0, W, pitch, 1, 0, 0))             # a skipped descriptor
    frame_of.insert(5, None)
    rc, out = _box_kernel(buf, _descs(items))
    assert rc == OK
    for n, (it, b) in enumerate(zip(items, frame_of)):
        if b is None:
            assert (out[n] == -7).all()
            continue
        want = _spec(frames[b], *it[4:])
        assert np.array_equal(_bits(out[n]), _bits(want)), it


@pytest.mark.parametrize("W", [64, 53])
def test_box_kernel_aligned_and_byte_routes(W):
    """The same pixels at a 16-byte aligned place (pitch 3 * W: at W = 64 every row start is aligned, at W = 53
    one row in 16) and one byte further on, where no 16-byte load is possible."""
    H = 40
    frame = _img(H, W, 62)
    buf = torch.zeros((H * 3 * W + 64,), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    flat = torch.from_numpy(frame.reshape(-1)).cuda()
    where = [(0, 0, 0), (0, 8, 16), (0, 24, 32), (0, 3, 5), (1, 0, 0), (1, 4, 8), (1, 5, 11), (2, 0, 0), (2, 1, 4),
             (3, 0, 0), (3, 2, 2)]
    outs = []
    for off in (0, 1):
        buf.fill_(255)
        buf[off:off + flat.numel()] = flat
        rc, out = _box_kernel(buf, _descs([(off, H, W, 3 * W, l, y0, x0) for l, y0, x0 in where]))
        assert rc == OK
        outs.append(out)
    for n, w in enumerate(where):
        assert np.array_equal(_bits(outs[0][n]), _bits(_spec(frame, *w))), (W, w)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def _ragged_warp(img_dev, H, W, pitch, dst_to_src, th=TH, tw=TW):
    d = np.zeros((len(dst_to_src),), native.IMAGE_DESC)
    d['H'], d['W'], d['pitch'], d['dst_to_src'] = H, W, pitch, dst_to_src
    dd = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.full((len(d), 3, th, tw), -7.0, device="cuda")
    native.check(native.lib().cn_warp_normalize_u8_f32_ragged(native.ptr(img_dev), native.ptr(dd), len(d), th, tw,
                                                              _c3(MEAN), _c3(STD), 0, native.ptr(out),
                                                              native.stream_ptr()), "ragged warp")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_level_0_is_the_ragged_warp_at_the_tile_translation():
    H, W, pitch = 37, 53, 3 * 53 + 5
    frame = _img(H, W, 63)
    buf = torch.from_numpy(_packed([frame], [pitch], [0], H * pitch)).cuda()
    grid = tiles.tile_grid(H, W, TH, TW, (4, 6))
    assert grid.T > 4
    want = _ragged_warp(buf, H, W, pitch, tiles.tile_maps(grid, 4)[1])
    rc, got = _box_kernel(buf, _descs([(0, H, W, pitch, 0, y0, x0) for y0, x0 in grid.origins]))
    assert rc == OK and np.array_equal(_bits(got), _bits(want))


def test_level_1_is_the_half_size_resize_and_the_ragged_warp():
    H, W = 40, 56
    frame = torch.from_numpy(_img(H, W, 64)).cuda()
    half = torch.empty((H // 2, W // 2, 3), dtype=torch.uint8, device="cuda")
    native.check(native.lib().cn_resize_bilinear_u8(native.ptr(frame), H, W, 3 * W, H // 2, W // 2, native.ptr(half),
                                                    native.stream_ptr()), "resize")
    grid = tiles.tile_grid(H // 2, W // 2, TH, TW, (4, 6))
    assert grid.T == 4
    want = _ragged_warp(half, H // 2, W // 2, 3 * (W // 2), tiles.tile_maps(grid, 4)[1])
    rc, got = _box_kernel(frame.reshape(-1), _descs([(0, H, W, 3 * W, 1, y0, x0) for y0, x0 in grid.origins]))
    assert rc == OK and np.array_equal(_bits(got), _bits(want))


def test_box_kernel_argument_errors_write_nothing():
    frame = _img(20, 30, 65)
    buf = frame.reshape(-1).copy()
    descs = _descs([(0, 20, 30, 90, 1, 0, 0)])

    def call(**bad):
        rc, out = _box_kernel(buf, descs, bad=bad)
        if rc != OK:
            assert (out == -7).all()
        return rc
    assert call() == OK
    for name in ("buf", "descs", "out"):
        assert call(**{name: None}) == NULL, name
    assert call(mean=None) == NULL and call(std=None) == NULL
    assert call(N=0) == SHAPE and call(N=65536) == SHAPE and call(th=0) == SHAPE and call(tw=0) == SHAPE
    assert call(th=65536) == SHAPE and call(std=_c3([0.3, 0.0, 0.3])) == SHAPE


# ------------------------------------------------------------------------------------------------
# 2. the gated merge
# ------------------------------------------------------------------------------------------------
def _merge_gated(rows, bounds, B, T, nc, cores, gates, nms, cap, bad=()):
    """the call -> (rc, out_rows, out_bounds, status), the outputs filled with -7 (test_gpu_tiles._merge's twin)"""
    lib = native.lib()
    K = rows.shape[1]
    a = dict(rows=torch.from_numpy(rows).cuda(), bounds=torch.from_numpy(bounds).cuda(),
             cores=torch.from_numpy(np.ascontiguousarray(cores, np.float32)).cuda(),
             gates=torch.from_numpy(np.ascontiguousarray(gates, np.float32)).cuda(), T=T, K=K,
             out_rows=torch.full((B, T * K, 5), -7.0, device="cuda"),
             out_bounds=torch.full((B, nc + 1), -7, dtype=torch.int32, device="cuda"),
             status=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    need = int(lib.cn_ctdet_tiles_merge_gated_workspace_bytes(B, T, K, nc))
    assert need == int(lib.cn_ctdet_tiles_merge_workspace_bytes(B, T, K, nc))
    a.update(ws=torch.empty((max(need, 16) + 16,), dtype=torch.uint8, device="cuda"), ws_bytes=need)
    outs = (a['out_rows'], a['out_bounds'], a['status'])
    a.update(dict(bad))
    rc = lib.cn_ctdet_tiles_merge_gated_f32(native.ptr(a['rows']), native.ptr(a['bounds']), B, a['T'], a['K'], nc,
                                            native.ptr(a['cores']), native.ptr(a['gates']), int(nms), cap,
                                            native.ptr(a['out_rows']), native.ptr(a['out_bounds']),
                                            native.ptr(a['status']), native.ptr(a['ws']), a['ws_bytes'],
                                            native.stream_ptr())
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in outs)


def _pyramid_rows():
    """B = 2 frames of 128 x 416 under 128-tiles at overlap 32 and levels 0..2: T = 4 + 2 + 1 tiles of K = 32
    rows in 3 classes.  Every tile lists boxes all over the frame (the cores decide); sizes on a quarter-pixel
    raster so that x2 - x1 is exact, among them both edges of every band, and one NaN box per frame."""
    grid = tiles.pyramid_grid(128, 416, 128, 128, 32, None, (0, 1, 2), None, 0.25)
    assert grid.level_T == [4, 2, 1] and grid.bands.tolist() == [[-np.inf, 40.0], [24.0, 80.0], [48.0, np.inf]]
    rng = np.random.RandomState(7)
    B, K, nc = 2, 32, 3
    edges = [24.0, 40.0, 48.0, 80.0]
    edges += [float(np.nextafter(np.float32(e), np.float32(0))) for e in edges]
    lists = []
    for i in range(B * grid.T):
        items = []
        for k in range(K - i % 3):
            s = edges[rng.randint(len(edges))] if k % 3 == 0 else rng.randint(20, 480) / 4.0
            other = min(s, rng.randint(8, 200) / 4.0)
            w, h = (s, other) if rng.randint(2) else (other, s)
            x1, y1 = rng.randint(0, 4 * 416) / 4.0 - w / 2, rng.randint(0, 4 * 128) / 4.0 - h / 2
            x1, y1 = np.floor(x1 * 4) / 4, np.floor(y1 * 4) / 4
            items.append((int(rng.randint(nc)), [x1, y1, x1 + w, y1 + h, rng.randint(1, 2000) / np.float32(2000)]))
        items[5] = (items[5][0], [10.0, 10.0, 30.0, float("nan"), 0.99])          # a NaN height
        lists.append(items)
    return grid, lists, B, K, nc


@pytest.mark.parametrize("nms", [False, True])
@pytest.mark.parametrize("cap", [5, 1000])
def test_gated_merge_against_the_host(nms, cap):
    grid, lists, B, K, nc = _pyramid_rows()
    rows, bounds, dicts = _pack(lists, K, nc)
    rc, out_rows, out_bounds, status = _merge_gated(rows, bounds, B, grid.T, nc, grid.cores, grid.gates, nms, cap)
    assert rc == OK and (status == 0).all()
    rows_in = sum(len(x) for x in lists[:grid.T])
    for b in range(B):
        want = ctdet_pyramid_results(dicts[b * grid.T:(b + 1) * grid.T], grid.cores, grid.gates, nc, nms, cap)
        _check_frame(out_rows[b], out_bounds[b], want, nc, (b, nms, cap))
        n = sum(len(v) for v in want.values())
        assert (5 <= n < 20) if cap == 5 else (20 < n < rows_in)      # the cut below / above the survivors


def test_open_gates_are_the_ungated_merge():
    grid, lists, B, K, nc = _pyramid_rows()
    rows, bounds, _ = _pack(lists, K, nc)
    gates = np.tile(np.float32([-INF, INF]), (grid.T, 1))
    for nms, cap in ((False, 1000), (True, 20)):
        got = _merge_gated(rows, bounds, B, grid.T, nc, grid.cores, gates, nms, cap)
        old = _merge(rows, bounds, B, grid.T, nc, grid.cores, nms, cap)
        assert got[0] == old[0] == OK
        assert np.array_equal(got[2], old[2]) and np.array_equal(got[3], old[3]) and (got[3] == 0).all()
        for b in range(B):
            n = got[2][b, nc]
            assert n > 0 and np.array_equal(_bits(got[1][b, :n]), _bits(old[1][b, :n]))


def test_a_class_segment_of_2049_survivors_sets_its_frame_status_only():
    rng = np.random.RandomState(6)
    B, T, K, nc = 2, 21, 128, 4
    lists = [_clustered(rng, K, np.zeros(K, int)) for _ in range(T)]          # frame 0: 2688 rows of class 0
    lists += [_clustered(rng, K, np.zeros(K, int) if t < 16 else 1 + np.arange(K) % 3) for t in range(T)]
    rows, bounds, _ = _pack(lists, K, nc)
    # sizes: 20 passes the gate, 60 does not.  Frame 0: 2049 rows of class 0 pass; frame 1: all 2048 of class 0
    size = np.full((B * T * K,), 20.0, np.float32)
    size[2049:T * K] = 60.0
    rows = rows.reshape(-1, 5)
    rows[:, 2], rows[:, 3] = rows[:, 0] + size, rows[:, 1] + np.float32(10)
    rows = rows.reshape(B * T, K, 5)
    dicts = [{j + 1: rows[i, bounds[i, j]:bounds[i, j + 1]].copy() for j in range(nc)} for i in range(B * T)]
    cores = np.tile(np.float32([-INF, -INF, INF, INF]), (T, 1))
    gates = np.tile(np.float32([-INF, 40.0]), (T, 1))
    rc, out_rows, out_bounds, status = _merge_gated(rows, bounds, B, T, nc, cores, gates, False, 100)
    assert rc == OK and status[0] != 0 and status[1] == 0
    assert (out_bounds[0] == 0).all()
    want = ctdet_pyramid_results(dicts[T:], cores, gates, nc, False, 100)
    _check_frame(out_rows[1], out_bounds[1], want, nc)
    # one survivor fewer in frame 0 and it is merged
    rows[2048 // K, 2048 % K, 2] = rows[2048 // K, 2048 % K, 0] + np.float32(60)
    rc, _, out_bounds, status = _merge_gated(rows, bounds, B, T, nc, cores, gates, False, 100)
    assert rc == OK and (status == 0).all() and out_bounds[0, nc] > 0


def test_gated_merge_argument_errors_launch_nothing():
    lib = native.lib()
    B, T, K, nc = 1, 2, 8, 3
    rows, bounds, _ = _pack([[(0, _box(5, 5, 2, 2, 0.5))]] * 2, K, nc)
    cores = np.tile(np.float32([-INF, -INF, INF, INF]), (T, 1))
    gates = np.tile(np.float32([-INF, INF]), (T, 1))

    def call(**bad):
        rc, out_rows, out_bounds, status = _merge_gated(rows, bounds, B, T, nc, cores, gates, False, 100, bad)
        if rc != OK:
            assert (out_rows == -7).all() and (out_bounds == -7).all() and (status == -7).all()
        return rc
    assert call() == OK
    for name in ("rows", "bounds", "cores", "gates", "out_rows", "out_bounds", "status", "ws"):
        assert call(**{name: None}) == NULL, name
    need = int(lib.cn_ctdet_tiles_merge_gated_workspace_bytes(B, T, K, nc))
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    ws = torch.empty((need + 32,), dtype=torch.uint8, device="cuda")
    assert call(ws=ws[4:]) == ALIGN
    assert call(T=native.TILES_MAX_ROWS // K + 1) == SHAPE
    assert call(K=129) == SHAPE and call(T=0) == SHAPE
    assert lib.cn_ctdet_tiles_merge_gated_workspace_bytes(1, 0, 8, 3) == 0


# ------------------------------------------------------------------------------------------------
# 3. the tile pipe with levels
# ------------------------------------------------------------------------------------------------
def _frames(seed):
    return [_img(200, 296, seed), _img(200, 296, seed + 1)]


def test_level_0_alone_equals_run_tiles(dev, ctdet):
    ctdet.tail_fallbacks = 0
    frames = _frames(70)
    plain = ctdet.run_tiles(frames, overlap=32, tile_batch=8)
    _same(ctdet.run_tiles(frames, overlap=32, tile_batch=8, levels=(0,)), plain, "levels=(0,)")
    assert sum(len(v) for r in plain for v in r.values()) > 0 and ctdet.tail_fallbacks == 0


def test_two_levels_against_the_sync_path_and_the_host_tail(dev, ctdet):
    det = ctdet
    det.tail_fallbacks = 0
    frames = _frames(72)
    args = det._tiles_args(32, None, 8, None)
    options = det._pyramid_options(args, (0, 1), None, 0.25)
    assert options == dict(levels=(0, 1), size_gate=32.0, gate_slack=0.25)
    pipe = det._tile_pipe_for(frames, 1, *args, 'bgr', **options)
    assert pipe.tail is not None and pipe.gates_dev is not None and (pipe.T, pipe.N, pipe.C) == (8, 16, 8)
    assert pipe.grid.level_T == [6, 2]
    seen, run_scale = [], det._run_scale

    def spy(batch, flip, **kw):
        dets = run_scale(batch, flip, **kw)
        seen.append((batch.clone(), dets.clone()))
        return dets
    det._run_scale = spy
    try:
        pipe.submit(0, frames)
        got = pipe.collect(0, frames)
    finally:
        del det._run_scale
    assert len(seen) == 2
    # (a) every tile of the batches == the host specification of the box pre-process
    for (batch, _), lv in zip(seen, pipe.levels):
        host = batch.cpu().numpy()
        for j in range(lv.n):
            b, t = divmod(lv.lo + j, pipe.T)
            want = I.tile_box_normalize(frames[b], pipe.grid.level[t], *pipe.grid.origins[t], 128, 128,
                                        det.mean.reshape(-1), det.std.reshape(-1))
            assert np.array_equal(_bits(host[j]), _bits(want)), (lv.lo, j)
    # (b) the results == the host tail on the same raw detections, (c) == the synchronous path
    raw = np.concatenate([d.cpu().numpy()[:lv.n] for (_, d), lv in zip(seen, pipe.levels)], axis=0)
    assert det.range_ok()
    _same(got, det._tiles_host_tail(raw, pipe.grid, 2, pipe.max_per_frame, **options), "host tail")
    assert sum(len(v) for r in got for v in r.values()) > 0
    _same(det.run_tiles(frames, overlap=32, tile_batch=8, levels=(0, 1)), got, "run_tiles")
    _same(got, det._run_tiles_sync(frames, *args, **options), "_run_tiles_sync")
    assert det.tail_fallbacks == 0


def test_stream_with_levels_equals_the_single_calls(dev, ctdet):
    ctdet.tail_fallbacks = 0
    batches = [_frames(80 + 2 * k) for k in range(3)]
    kw = dict(overlap=32, tile_batch=8, levels=(0, 1))
    alone = [ctdet.run_tiles(b, **kw) for b in batches]
    streamed = list(ctdet.run_tiles_stream(iter(batches), depth=3, **kw))
    assert len(streamed) == 3
    for a, s in zip(alone, streamed):
        _same(s, a)
    assert ctdet.tail_fallbacks == 0


def test_nv12_frames_with_levels(dev, ctdet):
    ctdet.tail_fallbacks = 0
    nv12 = [I.bgr_to_nv12(f) for f in _frames(90)]
    kw = dict(overlap=32, tile_batch=8, levels=(0, 1))
    _same(ctdet.run_tiles(nv12, pixel_format='nv12', **kw), ctdet.run_tiles([I.nv12_to_bgr(f) for f in nv12], **kw))
    assert ctdet.tail_fallbacks == 0


def test_a_chunk_boundary_inside_a_level(dev, ctdet):
    ctdet.tail_fallbacks = 0
    frames = _frames(94)
    kw = dict(overlap=32, levels=(0, 1))
    _same(ctdet.run_tiles(frames, tile_batch=5, **kw), ctdet.run_tiles(frames, tile_batch=32, **kw), "tile_batch")
    assert ctdet.tail_fallbacks == 0


def test_too_many_rows_are_refused_before_any_device_work(dev, ctdet):
    frames = [np.zeros((2160, 3840, 3), np.uint8)]
    before = len(ctdet.__dict__.get("_pipes", {}))
    with pytest.raises(ValueError, match="rows per frame"):
        ctdet.run_tiles(frames, levels=(0, 1, 2))                 # 128-tiles: above a thousand of K = 100
    with pytest.raises(ValueError, match="levels"):
        ctdet.run_tiles(frames, levels=(1, 0))
    assert len(ctdet.__dict__.get("_pipes", {})) == before
