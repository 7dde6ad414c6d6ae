"""run_tiles on the host (no GPU): the tile geometry (tiles.tile_grid), the tile meta, the host tile merge
(post_process.ctdet_tiles_results -- the specification of cn_ctdet_tiles_merge_f32) against
CtdetDetector.merge_outputs, the refusals of the public entries and the new prototypes."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

from centernet_amd import native, tiles
from centernet_amd.detectors.ctdet import CtdetDetector
from centernet_amd.image import get_affine_transform, invert_affine
from centernet_amd.post_process import ctdet_tiles_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _detector(scales=(1.0,), nms=False, max_per_image=100, **opt):
    """A CtdetDetector without a device: what merge_outputs and the argument checks read"""
    det = CtdetDetector.__new__(CtdetDetector)
    det.opt = types.SimpleNamespace(nms=nms, fix_res=True, flip_test=False, input_h=128, input_w=128, K=100,
                                    num_classes=NC, down_ratio=4)
    det.opt.__dict__.update(opt)
    det.scales, det.num_classes, det.max_per_image = list(scales), NC, max_per_image
    return det


# ------------------------------------------------------------------------------------------------
# 1. tile_grid
# ------------------------------------------------------------------------------------------------
def test_axis_origins_counts_and_edges():
    assert tiles.axis_origins(100, 128, 32) == [0]
    assert tiles.axis_origins(128, 128, 32) == [0]
    assert tiles.axis_origins(129, 128, 32) == [0, 1]
    assert tiles.axis_origins(3840, 512, 128) == [0, 384, 768, 1152, 1536, 1920, 2304, 2688, 3072, 3328]
    assert len(tiles.axis_origins(2160, 512, 128)) == 6
    for L in list(range(1, 700, 7)) + [128, 129, 224, 225, 4096]:
        for t, o in ((128, 0), (128, 32), (128, 64), (96, 17), (7, 3)):
            xs = tiles.axis_origins(L, t, o)
            n = 1 if L <= t else math.ceil((L - t) / (t - o)) + 1
            assert len(xs) == n and xs[0] == 0
            assert all(0 <= x <= max(L - t, 0) for x in xs)
            assert xs[-1] == max(L - t, 0)                       # flush with the edge
            assert all(b > a for a, b in zip(xs, xs[1:]))
            covered = np.zeros(L, bool)
            for x in xs:
                covered[x:x + t] = True
            assert covered.all()
            assert all(b - a <= t - o for a, b in zip(xs, xs[1:]))   # neighbours share at least the overlap


def test_grid_order_and_cores():
    g = tiles.tile_grid(200, 296, 128, 128, 32)
    assert (g.ny, g.nx, g.T) == (2, 3, 6)
    assert g.origins == [(0, 0), (0, 96), (0, 168), (72, 0), (72, 96), (72, 168)]      # row-major
    assert g.cores.dtype == np.float32 and g.cores.shape == (6, 4)
    # boundaries: the middle of the overlaps; default margin = overlap / 4 = 8
    assert g.cores[0].tolist() == [-np.inf, -np.inf, (96 + 0 + 128) / 2 + 8, (72 + 0 + 128) / 2 + 8]
    assert g.cores[4].tolist() == [112 - 8, 100 - 8, (168 + 96 + 128) / 2 + 8, np.inf]
    assert g.cores[5].tolist() == [196 - 8, 100 - 8, np.inf, np.inf]
    one = tiles.tile_grid(100, 60, 128, 128, 32)
    assert one.T == 1 and one.origins == [(0, 0)] and one.cores[0].tolist() == [-np.inf, -np.inf, np.inf, np.inf]
    both = tiles.tile_grid(300, 200, 128, 96, (32, 16), (0, 2.5))        # per-axis overlap and margin
    assert both.xs == tiles.axis_origins(200, 96, 16) and both.ys == tiles.axis_origins(300, 128, 32)
    assert both.cores[0, 2] == np.float32((both.xs[1] + 96) / 2 + 2.5) and both.cores[0, 3] == (both.ys[1] + 128) / 2


def test_cores_without_margin_partition_the_plane():
    g = tiles.tile_grid(200, 300, 128, 128, 32, 0)
    ys, xs = np.arange(0, 200, 0.5, dtype=np.float32), np.arange(0, 300, 0.5, dtype=np.float32)
    px, py = np.meshgrid(xs, ys)
    rows = np.stack([px, py, px, py, np.ones_like(px)], axis=-1).reshape(-1, 5)      # a point box: centre = point
    count = sum(tiles.in_core(rows, core).astype(np.int32) for core in g.cores)
    assert count.shape == (400 * 600,) and (count == 1).all()
    wide = tiles.tile_grid(200, 300, 128, 128, 32, 4)                   # with a margin: bands seen twice
    count = sum(tiles.in_core(rows, core).astype(np.int32) for core in wide.cores)
    assert count.min() == 1 and count.max() == 4


def test_grid_refusals():
    for bad in (-1, 65, 1.5, (32, 65)):
        with pytest.raises(ValueError, match="overlap"):
            tiles.tile_grid(300, 300, 128, 128, bad)
    with pytest.raises(ValueError, match="margin"):
        tiles.tile_grid(300, 300, 128, 128, 32, -0.5)
    with pytest.raises(ValueError, match="margin"):
        tiles.tile_grid(300, 300, 128, 128, 32, float("nan"))
    tiles.tile_grid(300, 300, 128, 128, 64)                              # t // 2 itself is fine
    tiles.tile_grid(300, 300, 128, 128, 0, 0)


def test_entry_refusals():
    ok = _detector()
    assert ok._tiles_args(None, None, 32, None) == ((32, 32), (8.0, 8.0), 32, 100)
    assert ok._tiles_args(16, 1, 4, 7) == ((16, 16), (1.0, 1.0), 4, 7)
    for det, word in ((_detector(fix_res=False), "keep_res"), (_detector(scales=(1.0, 0.5)), "test scale"),
                      (_detector(scales=(0.5,)), "test scale"), (_detector(flip_test=True), "flip_test")):
        with pytest.raises(ValueError, match=word):
            det._tiles_args(None, None, 32, None)
    for kw, word in ((dict(overlap=65), "overlap"), (dict(overlap=-1), "overlap"), (dict(margin=-1), "margin"),
                     (dict(tile_batch=0), "tile_batch"), (dict(max_per_frame=0), "max_per_frame")):
        a = dict(overlap=None, margin=None, tile_batch=32, max_per_frame=None)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            ok._tiles_args(**a)
    frames = [np.zeros((10, 12, 3), np.uint8), np.zeros((10, 13, 3), np.uint8)]
    with pytest.raises(ValueError, match="one size"):
        ok._tiles_frames(frames, 'bgr')
    with pytest.raises(ValueError):
        ok._tiles_frames(frames[:1], 'rgb')
    # the other tasks do not get the methods
    from centernet_amd.detectors.base_detector import BaseDetector
    assert not hasattr(BaseDetector, "run_tiles") and not hasattr(BaseDetector, "run_tiles_stream")


# ------------------------------------------------------------------------------------------------
# 2. the tile meta: a pure translation at scale 1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,tw", [(128, 128), (512, 512), (96, 160), (160, 96)])
def test_tile_meta_is_the_translation(th, tw):
    # origins up to an 8K frame's; the float64 elimination's error grows with the origin (a few 1e-14 of it)
    for y0, x0 in ((0, 0), (72, 168), (1648, 3328), (4224, 7584)):
        m = tiles.tile_meta(y0, x0, th, tw, 4)
        assert m['c'].dtype == np.float32 and m['c'].tolist() == [x0 + tw / 2, y0 + th / 2]
        assert m['s'] == float(tw) and m['out_height'] == th // 4 and m['out_width'] == tw // 4
        t = get_affine_transform(m['c'], m['s'], 0, [tw, th])
        # all six entries within 1e-9 (the elimination of get_affine_transform leaves ~1e-16 in an off-diagonal
        # entry for some centres, as it does for every fixed-resolution image: no new arithmetic here)
        assert np.abs(t - np.array([[1, 0, -x0], [0, 1, -y0]], np.float64)).max() <= 1e-9
        back = invert_affine(t)
        assert abs(back[0, 2] - x0) <= 1e-9 and abs(back[1, 2] - y0) <= 1e-9
    g = tiles.tile_grid(200, 296, th, tw, 16)
    metas, dst_to_src, to_source = tiles.tile_maps(g, 4)
    assert len(metas) == g.T and dst_to_src.shape == to_source.shape == (g.T, 6)
    for (y0, x0), d, s in zip(g.origins, dst_to_src, to_source):
        assert np.allclose(d, [1, 0, x0, 0, 1, y0], atol=1e-9, rtol=0)
        assert np.allclose(s, [4, 0, x0, 0, 4, y0], atol=1e-9, rtol=0)


# ------------------------------------------------------------------------------------------------
# 3. the host merge
# ------------------------------------------------------------------------------------------------
def _tile_rows(rng, T, K, levels=50):
    """per tile {class: (n, 5)}: clustered boxes (soft-NMS has work to do), scores on steps (ties)"""
    centres = rng.uniform(20, 280, (6, 2))
    out = []
    for _ in range(T):
        cls = np.sort(rng.randint(0, NC, K))
        c = centres[rng.randint(0, 6, K)] + rng.normal(0, 2.0, (K, 2))
        wh = rng.uniform(8, 40, (K, 2))
        r = np.concatenate([c - wh / 2, c + wh / 2, rng.randint(1, levels + 1, (K, 1)) / levels * 0.9], axis=1)
        r = r.astype(np.float32)
        out.append({j + 1: r[cls == j].copy() for j in range(NC)})
    return out


@pytest.mark.parametrize("T,nms,cap", [(1, False, 100), (1, True, 100), (4, False, 100), (6, True, 37), (3, False, 1000)])
def test_host_merge_with_infinite_cores_is_merge_outputs(T, nms, cap):
    rng = np.random.RandomState(7 + T)
    per_tile = _tile_rows(rng, T, 60)
    cores = np.tile(np.array([[-np.inf, -np.inf, np.inf, np.inf]], np.float32), (T, 1))
    det = _detector(scales=(1.0,) * T, nms=nms, max_per_image=cap)          # the tiles as if they were scales
    want = det.merge_outputs([{c: v.copy() for c, v in d.items()} for d in per_tile])
    got = ctdet_tiles_results([{c: v.copy() for c, v in d.items()} for d in per_tile], cores, NC, nms, cap)
    assert sorted(got) == sorted(want) == list(range(1, NC + 1))
    for c in want:
        assert got[c].shape == want[c].shape and got[c].dtype == np.float32
        assert np.array_equal(_bits(got[c]), _bits(want[c])), c
    if cap == 37:
        assert sum(len(v) for v in got.values()) >= 37                         # the cut was reached


def test_host_merge_core_edges_are_half_open():
    g = tiles.tile_grid(128, 224, 128, 128, 32, 4)           # two tiles side by side, b_1 = 112, margin 4
    assert g.T == 2 and g.cores[0, 2] == 116 and g.cores[1, 0] == 108

    def box(cx, cy=64.0, score=0.5):
        return np.array([[cx - 5, cy - 5, cx + 5, cy + 5, score]], np.float32)

    def run(cx, tile):
        per_tile = [{c: np.zeros((0, 5), np.float32) for c in range(1, NC + 1)} for _ in range(2)]
        per_tile[tile][1] = box(cx)
        return len(ctdet_tiles_results(per_tile, g.cores, NC, False, 100)[1])
    assert run(108.0, 1) == 1                 # exactly on b_1 - m: kept by tile 1
    assert run(np.nextafter(np.float32(108), np.float32(0)), 1) == 0
    assert run(116.0, 0) == 0                 # exactly on b_1 + m: not kept by tile 0
    assert run(np.nextafter(np.float32(116), np.float32(0)), 0) == 1
    assert run(112.0, 0) == 1 and run(112.0, 1) == 1          # inside the margin band: both keep it
    assert run(float("nan"), 0) == 0
    # ... and soft-NMS removes the copy: the same box from both tiles decays below the threshold
    per_tile = [{c: np.zeros((0, 5), np.float32) for c in range(1, NC + 1)} for _ in range(2)]
    per_tile[0][1], per_tile[1][1] = box(112.0, score=0.004), box(112.0, score=0.004)
    out = ctdet_tiles_results(per_tile, g.cores, NC, False, 100)[1]
    assert out.shape == (2, 5) and out[0, 4] == np.float32(0.004) and out[1, 4] < 0.001   # (whole array kept)


# ------------------------------------------------------------------------------------------------
# 4. the prototypes
# ------------------------------------------------------------------------------------------------
def test_tiles_merge_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "centernet_amd.h")).read()
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert "size_t cn_ctdet_tiles_merge_workspace_bytes(int B, int T, int K, int num_classes);" in plain
    assert ("int cn_ctdet_tiles_merge_f32(const float *rows, const int32_t *bounds, int B, int T, int K, "
            "int num_classes, const float *cores_dev, int apply_nms, int max_per_frame, float *out_rows, "
            "int32_t *out_bounds, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);") in plain
    assert int(re.search(r"#define CN_TILES_MAX_ROWS (\d+)", src).group(1)) == native.TILES_MAX_ROWS == 65536
    lib = native.lib()
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert lib.cn_ctdet_tiles_merge_f32.restype is i
    assert list(lib.cn_ctdet_tiles_merge_f32.argtypes) == [vp, vp, i, i, i, i, vp, i, i, vp, vp, vp, vp, sz, vp]
    assert lib.cn_ctdet_tiles_merge_workspace_bytes.restype is sz
    # host-side answers need no device
    need = lib.cn_ctdet_tiles_merge_workspace_bytes(2, 60, 100, 80)
    assert need >= 2 * 60 * 100 * 5 * 4 + 2 * 81 * 4 and need % 16 == 0
    assert lib.cn_ctdet_tiles_merge_f32(None, None, 1, 1, 1, 1, None, 0, 1, None, None, None, None, 0, None) == -5
