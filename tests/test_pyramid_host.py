"""The tile pyramid of ctdet's run_tiles on the host (no GPU): tiles.pyramid_grid (level grids, cores, maps and
size gates), the refusals, post_process.ctdet_pyramid_results on hand-made rows and image.tile_box_normalize
against a plain double loop."""
import numpy as np
import pytest

from centernet_amd import image as I
from centernet_amd import tiles
from centernet_amd.post_process import ctdet_pyramid_results, ctdet_tiles_results

INF = np.float32(np.inf)


def test_level_0_alone_is_tile_grid_bit_for_bit():
    for H, W, th, tw, ov, margin in ((200, 296, 128, 128, 32, None), (37, 53, 16, 24, (4, 6), 0),
                                    (10, 300, 128, 128, 0, None)):
        plain = tiles.tile_grid(H, W, th, tw, ov, margin)
        pyr = tiles.pyramid_grid(H, W, th, tw, ov, margin, (0,), None, 0.25, down_ratio=4)
        assert pyr.T == plain.T and pyr.origins == plain.origins and pyr.level == [0] * plain.T
        assert pyr.level_lo == [0] and pyr.level_T == [plain.T]
        assert pyr.cores.dtype == np.float32 and pyr.cores.tobytes() == plain.cores.tobytes()
        metas, _, to_source = tiles.tile_maps(plain, 4)
        assert pyr.to_source.dtype == np.float64 and pyr.to_source.tobytes() == to_source.tobytes()
        assert pyr.gates.dtype == np.float32 and pyr.gates.shape == (plain.T, 2)
        assert (pyr.gates[:, 0] == -INF).all() and (pyr.gates[:, 1] == INF).all()
        for a, b in zip(pyr.metas, metas):
            assert a['c'].tobytes() == b['c'].tobytes() and a['s'] == b['s']


def test_every_pixel_centre_lies_in_one_core_of_every_level():
    H, W = 37, 53
    g = tiles.pyramid_grid(H, W, 16, 24, (4, 6), 0, (0, 1, 2, 3), None, 0.25)
    assert g.levels == (0, 1, 2, 3) and sum(g.level_T) == g.T == len(g.origins) == len(g.level)
    assert g.level_T[0] == tiles.tile_grid(37, 53, 16, 24, (4, 6), 0).T and g.level_T[3] == 1    # 5 x 7: one tile
    ys, xs = np.mgrid[0:H, 0:W]
    rows = np.zeros((H * W, 5), np.float32)
    rows[:, 0] = rows[:, 2] = xs.reshape(-1)
    rows[:, 1] = rows[:, 3] = ys.reshape(-1)
    for lo, n, l in zip(g.level_lo, g.level_T, g.levels):
        assert g.level[lo:lo + n] == [l] * n
        count = sum(tiles.in_core(rows, g.cores[t]).astype(int) for t in range(lo, lo + n))
        assert (count == 1).all(), l


def test_maps_send_the_first_output_cell_to_the_first_block_centre():
    g = tiles.pyramid_grid(300, 500, 64, 64, 16, None, (0, 1, 2, 3), None, 0.25, down_ratio=4)
    maps = tiles.pyramid_maps(g, 4)[1]
    assert maps.tobytes() == g.to_source.tobytes() and maps.shape == (g.T, 6)
    for t, ((y0, x0), l) in enumerate(zip(g.origins, g.level)):
        f = 1 << l
        m = g.to_source[t].reshape(2, 3)
        assert abs(m[0, 2] - (f * x0 + (f - 1) / 2.0)) < 1e-3 and abs(m[1, 2] - (f * y0 + (f - 1) / 2.0)) < 1e-3
        assert abs(m[0, 0] - 4.0 * f) < 1e-4 and abs(m[1, 1] - 4.0 * f) < 1e-4     # one output cell: 4 level pixels
        assert np.array_equal(np.asarray(g.metas[t]['to_source']).reshape(-1), g.to_source[t])
    # the cores of a coarse level are its level bounds under u = v * f + (f - 1) / 2, rounded once
    lo, l = g.level_lo[2], 2
    lv = tiles.tile_grid(75, 125, 64, 64, 16, None)
    want = (lv.cores.astype(np.float64) * 4 + 1.5).astype(np.float32)
    assert g.cores[lo:lo + lv.T].tobytes() == want.tobytes() and np.isinf(want).any()


def test_default_gates():
    g = tiles.pyramid_grid(2160, 3840, 512, 512, (128, 96), None, (0, 1, 3), None, 0.25)
    band = {l: g.gates[lo] for l, lo in zip(g.levels, g.level_lo)}
    f32 = np.float32
    assert band[0][0] == -INF and band[0][1] == f32(96 * 1.25)            # g = min(overlap) = 96
    assert band[1][0] == f32(96 * 0.75) and band[1][1] == f32(96 * 2 * 1.25)
    assert band[3][0] == f32(96 * 2 * 0.75) and band[3][1] == INF
    assert band[1][0] < band[0][1] and band[3][0] < band[1][1]             # consecutive bands overlap
    for lo, n in zip(g.level_lo, g.level_T):                               # one band per level, repeated
        assert (g.gates[lo:lo + n] == g.gates[lo]).all()
    exact = tiles.level_gates((0, 1, 2), 100.0, 0.0)
    assert exact.tolist() == [[-np.inf, 100.0], [100.0, 200.0], [200.0, np.inf]]
    third = tiles.level_gates((1, 2), 10, 0.1)                             # float64, then one rounding
    assert third[0, 1] == f32(20 * 1.1) and third[1, 0] == f32(20 * 0.9)


@pytest.mark.parametrize("levels", [(), (4,), (-1, 0), (1, 1), (2, 1), (0, 1.5), 2, None, (True,)])
def test_bad_levels(levels):
    with pytest.raises(ValueError, match="levels"):
        tiles.pyramid_grid(100, 100, 32, 32, 8, None, levels, None, 0.25)


def test_bad_gates_and_row_cap():
    for g in (0, -3.0, float("nan")):
        with pytest.raises(ValueError, match="size_gate"):
            tiles.pyramid_grid(100, 100, 32, 32, 8, None, (0, 1), g, 0.25)
    for s in (-0.1, 1.0, 2, float("nan")):
        with pytest.raises(ValueError, match="gate_slack"):
            tiles.pyramid_grid(100, 100, 32, 32, 8, None, (0, 1), None, s)
    with pytest.raises(ValueError, match="size_gate"):                     # the default at overlap 0 is no gate
        tiles.pyramid_grid(100, 100, 32, 32, 0, None, (0, 1), None, 0.25)
    g = tiles.pyramid_grid(2160, 3840, 128, 128, 32, None, (0, 1, 2), None, 0.25)
    assert g.T * 100 > 65536
    with pytest.raises(ValueError, match="rows per frame"):
        tiles.check_pyramid_rows(g.T, 100, 65536)
    tiles.check_pyramid_rows(512, 128, 65536)                              # at the cap: taken


def _box(cx, cy, w, h, score):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score]


def _count(res):
    return sum(len(v) for v in res.values())


def test_pyramid_results_drop_the_fragment_and_keep_the_whole_box():
    """A 150-pixel object in a 256 x 128 frame of two 128-tiles (overlap 32, so the level-0 band ends at 40):
    level 0 sees two clipped fragments, level 1 (one tile) the whole box."""
    g = tiles.pyramid_grid(128, 224, 128, 128, 32, None, (0, 1), None, 0.25)
    assert g.T == 3 and g.gates[0, 1] == 40.0 and g.gates[2, 0] == 24.0
    frag_a, frag_b = _box(64, 64, 120, 40, 0.8), _box(170, 64, 100, 40, 0.7)      # clipped at the tiles' borders
    whole, small = _box(110, 64, 150, 40, 0.9), _box(30, 30, 10, 12, 0.6)
    e = np.zeros((0, 5), np.float32)
    per_tile = [{1: np.array([frag_a, small], np.float32), 2: e}, {1: np.array([frag_b], np.float32), 2: e},
                {1: np.array([whole, _box(30, 30, 11, 12, 0.5)], np.float32), 2: e}]
    got = ctdet_pyramid_results(per_tile, g.cores, g.gates, 2, False, 100)
    boxes = got[1][:, :4].tolist()
    assert np.float32(whole[:4]).tolist() in boxes and np.float32(small[:4]).tolist() in boxes
    assert np.float32(frag_a[:4]).tolist() not in boxes and np.float32(frag_b[:4]).tolist() not in boxes
    assert len(got[1]) == 2 and len(got[2]) == 0          # (level 1's copy of the small object is below its band)
    # without the gate the fragments survive: what the feature is for
    plain = ctdet_tiles_results(per_tile, g.cores, 2, False, 100)
    assert np.float32(frag_a[:4]).tolist() in plain[1][:, :4].tolist() and len(plain[1]) == 5


def test_gate_edges_and_nan():
    lo, hi = np.float32(24.0), np.float32(40.0)
    below_hi, below_lo = np.nextafter(hi, np.float32(0)), np.nextafter(lo, np.float32(0))
    nan = np.float32("nan")
    rows = np.array([[0, 0, lo, 5, .9], [0, 0, 5, hi, .8], [0, 0, below_hi, 1, .7], [0, 0, below_lo, below_lo, .6],
                     [0, 0, 30, nan, .5], [nan, 0, 30, 30, .4], [0, 0, 30, 30, .3], [10, 0, 5, 30, .2]], np.float32)
    assert tiles.in_gate(rows, (lo, hi)).tolist() == [True, False, True, False, False, False, True, True]
    assert tiles.in_gate(rows, (-INF, INF)).tolist() == [True] * 4 + [False, False, True, True]
    cores = np.array([[-INF, -INF, INF, INF]], np.float32)
    got = ctdet_pyramid_results([{1: rows}], cores, np.array([[lo, hi]], np.float32), 1, False, 100)
    assert got[1][:, 4].tolist() == np.float32([.9, .7, .3, .2]).tolist()


def _box_loop(frame, level, y0, x0, th, tw, mean, std):
    f = 1 << level
    H, W = frame.shape[:2]
    out = np.empty((3, th, tw), np.float32)
    for y in range(th):
        for x in range(tw):
            for c in range(3):
                s = 0
                for dy in range(f):
                    for dx in range(f):
                        sy, sx = (y0 + y) * f + dy, (x0 + x) * f + dx
                        if 0 <= sy < H and 0 <= sx < W:
                            s += int(frame[sy, sx, c])
                v = (s + (f * f >> 1)) >> (2 * level)
                out[c, y, x] = np.float32((np.float64(v) / 255.0 - np.float64(mean[c])) / np.float64(std[c]))
    return out


def test_box_pre_process_against_a_plain_loop():
    frame = np.random.RandomState(3).randint(0, 256, (7, 9, 3)).astype(np.uint8)
    mean, std = np.float32([0.408, 0.447, 0.47]), np.float32([0.289, 0.274, 0.278])
    for level, y0, x0 in ((0, 0, 0), (0, 2, 3), (1, 0, 0), (1, 1, 2), (2, 0, 0), (2, 1, 1), (3, 0, 0), (1, -1, -1)):
        got = I.tile_box_normalize(frame, level, y0, x0, 4, 6, mean, std)
        want = _box_loop(frame, level, y0, x0, 4, 6, mean, std)
        assert got.dtype == np.float32 and got.shape == (3, 4, 6)
        assert got.tobytes() == want.tobytes(), (level, y0, x0)
    zero = np.float32((0.0 / 255.0 - np.float64(mean[0])) / np.float64(std[0]))
    assert I.tile_box_normalize(frame, 3, 0, 0, 4, 6, mean, std)[0, 1, 2] == zero      # behind the level image
    with pytest.raises(ValueError):
        I.tile_box_normalize(frame, 4, 0, 0, 4, 6, mean, std)


def test_new_entries_are_declared_exported_and_bound():
    """The three new prototypes of include/centernet_amd.h, character for character after white space is
    collapsed (tests/golden/abi_prototypes.txt keeps the earlier ones and is not edited), the symbols in the
    library and native.py's bindings."""
    import ctypes
    import os
    import re
    from centernet_amd import native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "centernet_amd.h")).read()
    src = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for proto in (
            "int cn_tile_box_normalize_u8_f32(const uint8_t *packed, const cn_tile_box_desc *descs_dev, int N, "
            "int out_h, int out_w, const float *mean3, const float *std3, float *out_nchw, void *stream);",
            "size_t cn_ctdet_tiles_merge_gated_workspace_bytes(int B, int T, int K, int num_classes);",
            "int cn_ctdet_tiles_merge_gated_f32(const float *rows, const int32_t *bounds, int B, int T, int K, "
            "int num_classes, const float *cores_dev, const float *gates_dev, int apply_nms, int max_per_frame, "
            "float *out_rows, int32_t *out_bounds, int32_t *status, void *workspace, size_t workspace_bytes, "
            "void *stream);"):
        assert proto in src, proto
    lib = native.lib()
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    old, new = list(lib.cn_ctdet_tiles_merge_f32.argtypes), list(lib.cn_ctdet_tiles_merge_gated_f32.argtypes)
    assert new == old[:7] + [vp] + old[7:] and lib.cn_ctdet_tiles_merge_gated_f32.restype is i
    assert lib.cn_ctdet_tiles_merge_gated_workspace_bytes.restype is sz
    assert lib.cn_ctdet_tiles_merge_gated_workspace_bytes(2, 7, 32, 3) == \
        lib.cn_ctdet_tiles_merge_workspace_bytes(2, 7, 32, 3) > 0
    assert native.TILE_BOX_DESC.itemsize == 32
    # host-side refusals need no device
    assert lib.cn_tile_box_normalize_u8_f32(None, None, 1, 16, 16, None, None, None, None) == -5
    assert lib.cn_ctdet_tiles_merge_gated_f32(*([None, None, 1, 1, 8, 3, None, None, 0, 10] + [None] * 4 + [0, None])) == -5
