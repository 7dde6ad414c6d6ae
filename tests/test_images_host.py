"""run_images, the host side (no device): the per-image descriptor / map tables of a mixed-size batch against
input_geometry, get_affine_transform, invert_affine and _meta -- what run(image) computes -- bit for bit, the
packing offsets, and the argument checks."""
import numpy as np
import pytest

from centernet_amd import native
from centernet_amd.detectors.base_detector import BaseDetector
from centernet_amd.frame_pipe import ImageTables
from centernet_amd.image import get_affine_transform, invert_affine
from centernet_amd.opts import opts

SHAPES = [(100, 140), (64, 48), (131, 97), (300, 200), (64, 48), (1, 1)]
SCALES = (1.0, 0.5, 0.75, 2.0)


def _detector(args=()):
    opt = opts().init(["ctdet", "--input_h", "128", "--input_w", "160"] + list(args))
    det = BaseDetector.__new__(BaseDetector)
    det.opt = opt
    det.mean = np.array(opt.mean, dtype=np.float32).reshape(1, 1, 3)
    det.std = np.array(opt.std, dtype=np.float32).reshape(1, 1, 3)
    det.scales = list(SCALES)
    return det


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _tables(det, shapes, scales):
    desc = np.zeros((len(scales), 2, len(shapes)), native.IMAGE_DESC)
    to_source = np.zeros((len(scales), len(shapes), 6), np.float64)
    return (desc, to_source) + ImageTables(det, scales).fill(shapes, desc, to_source)


def test_descriptor_layout_is_the_c_struct():
    d = native.IMAGE_DESC
    assert d.itemsize == 88 and d.itemsize % 8 == 0
    assert [d.fields[n][1] for n in ("offset", "H", "W", "pitch", "reserved", "dst_to_src", "scale")] == \
        [0, 8, 12, 16, 20, 24, 72]


def test_tables_equal_the_single_image_geometry():
    det = _detector()
    shapes = [s for s in SHAPES if s != (1, 1)]
    desc, to_source, nbytes, offsets, metas, plan = _tables(det, shapes, SCALES)
    for l, scale in enumerate(SCALES):
        any_resize = False
        for j, (H, W) in enumerate(shapes):
            g = det.input_geometry(H, W, scale)
            meta = det._meta(g)
            src, dst = desc[l, 0, j], desc[l, 1, j]
            assert (src['H'], src['W'], src['pitch']) == (H, W, 3 * W)
            assert (dst['H'], dst['W'], dst['pitch']) == (g.scaled_h, g.scaled_w, 3 * g.scaled_w)
            to_input = get_affine_transform(g.center, g.extent, 0, [g.inp_w, g.inp_h])
            assert np.array_equal(_bits(dst['dst_to_src']), _bits(invert_affine(to_input).reshape(-1)))
            inv = get_affine_transform(meta['c'], meta['s'], 0, (meta['out_width'], meta['out_height']), inv=1)
            assert np.array_equal(_bits(to_source[l, j]), _bits(np.asarray(inv).reshape(-1)))
            assert np.array_equal(_bits(dst['scale']), _bits([1.0 / (float(g.scaled_w) / float(W)),
                                                              1.0 / (float(g.scaled_h) / float(H))]))
            m = metas[l][j]
            assert sorted(m) == sorted(meta)
            assert np.array_equal(m['c'], meta['c']) and m['c'].dtype == meta['c'].dtype
            assert np.array_equal(np.asarray(m['s']), np.asarray(meta['s']))
            assert (m['out_height'], m['out_width']) == (meta['out_height'], meta['out_width']) == (32, 40)
            any_resize |= (g.scaled_h, g.scaled_w) != (H, W)
        assert plan[l][0] == any_resize == (scale != 1.0)


def test_packing_offsets_are_contiguous():
    det = _detector()
    desc, _, nbytes, offsets, _, plan = _tables(det, SHAPES, (1.0, 2.0))
    sizes = [h * w * 3 for h, w in SHAPES]
    assert nbytes == sum(sizes)
    assert list(offsets) == [sum(sizes[:j]) for j in range(len(SHAPES))]
    for l in range(2):
        assert list(desc['offset'][l, 0]) == list(offsets)
    # scale 1: no resize, the warp reads the sources; scale 2: the scaled images, packed back to back
    assert plan[0] == (False, 0, 0, 0)
    assert list(desc['offset'][0, 1]) == list(offsets)
    scaled = [(2 * h) * (2 * w) * 3 for h, w in SHAPES]
    assert list(desc['offset'][1, 1]) == [sum(scaled[:j]) for j in range(len(SHAPES))]
    assert plan[1] == (True, 600, 400, sum(scaled))


def test_tables_refuse_images_without_pixels():
    det = _detector()
    with pytest.raises(ValueError):
        _tables(det, [(1, 1)], (0.5,))          # int(1 * 0.5) = 0 rows
    with pytest.raises(ValueError):
        _tables(det, [(40000, 8)], (1.0,))


def test_argument_checks():
    det = _detector()
    ok = np.zeros((8, 9, 3), np.uint8)
    assert det._images_one_size([ok, ok], "run_images") is True
    assert det._images_one_size([ok, np.zeros((9, 8, 3), np.uint8)], "run_images") is False
    for bad in ([], [ok.astype(np.float32)], [ok[:, :, 0]], [np.zeros((8, 9, 4), np.uint8)], [ok, None]):
        with pytest.raises(ValueError):
            det._images_one_size(bad, "run_images")
    with pytest.raises(ValueError):
        list(det.run_images_stream(iter([[ok.astype(np.int8)]])))


def test_keep_res_refuses_mixed_sizes():
    det = _detector(["--keep_res"])
    a, b = np.zeros((8, 9, 3), np.uint8), np.zeros((9, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="keep_res"):
        det.run_images([a, b])
    with pytest.raises(ValueError, match="keep_res"):
        list(det.run_images_stream(iter([[a, b]])))
    assert det._images_one_size([a, a], "run_images") is True


def test_ddd_refuses():
    from centernet_amd.detectors.ddd import DddDetector
    det = DddDetector.__new__(DddDetector)
    img = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        det.run_images([img])
    with pytest.raises(NotImplementedError):
        det.run_images_stream(iter([[img]]))
