"""run_images of the ddd task, the host side (no device): the per-image descriptor / map tables of a mixed-size
batch against _frame_geometry, get_affine_transform and invert_affine -- what run(image, calib) computes -- bit
for bit, with and without --keep_res; the forms of ``calibs``; the refusals."""
import contextlib
import sys

import numpy as np
import pytest

from centernet_amd import native
from centernet_amd.detectors.ddd import DddDetector
from centernet_amd.frame_pipe import ImageTables
from centernet_amd.image import get_affine_transform, invert_affine
from centernet_amd.opts import opts
from test_ddd_tail_host import DEFAULT, KITTI

SHAPES = [(37, 124), (40, 120), (1, 1), (96, 300), (37, 124)]


def _host_detector(extra=()):
    """A DddDetector without its network (the constructor needs the device): host methods only."""
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ddd", "--input_h", "96", "--input_w", "320"] + list(extra))
    det = DddDetector.__new__(DddDetector)
    det.opt, det.num_classes, det.scales = opt, opt.num_classes, opt.test_scales
    det.mean = np.asarray(opt.mean, np.float32).reshape(1, 1, 3)
    det.std = np.asarray(opt.std, np.float32).reshape(1, 1, 3)
    det.calib = DEFAULT
    return det


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.parametrize("extra", [(), ("--keep_res",)])
def test_tables_equal_the_single_image_geometry(extra):
    det = _host_detector(extra)
    scales = det._pipe_scales()
    assert len(scales) == 1
    desc = np.zeros((1, 2, len(SHAPES)), native.IMAGE_DESC)
    to_source = np.zeros((1, len(SHAPES), 6), np.float64)
    tables = ImageTables(det, scales)
    nbytes, offsets, metas, plan = tables.fill(SHAPES, desc, to_source)
    sizes = [h * w * 3 for h, w in SHAPES]
    assert nbytes == sum(sizes)
    assert list(offsets) == [sum(sizes[:j]) for j in range(len(SHAPES))]       # the running byte sums
    assert plan == [(False, 0, 0, 0)]                                          # no level resizes
    out_w, out_h = det.opt.input_w // det.opt.down_ratio, det.opt.input_h // det.opt.down_ratio
    for j, (H, W) in enumerate(SHAPES):
        c, s, to_input = det._frame_geometry(H, W)
        assert list(s) == ([det.opt.input_w, det.opt.input_h] if extra else [W, H])
        for k in (0, 1):                # the warp reads the sources: both descriptors describe them
            d = desc[0, k, j]
            assert (d['H'], d['W'], d['pitch'], d['offset']) == (H, W, 3 * W, offsets[j])
        assert np.array_equal(_bits(desc[0, 1, j]['dst_to_src']), _bits(invert_affine(to_input).reshape(-1)))
        inv = get_affine_transform(c, s, 0, (out_w, out_h), inv=1)
        assert np.array_equal(_bits(to_source[0, j]), _bits(np.asarray(inv).reshape(-1)))
        m = metas[0][j]
        assert np.array_equal(m['c'], c) and m['c'].dtype == np.float32
        assert np.array_equal(m['s'], s) and m['s'].dtype == np.int32
        assert (m['out_height'], m['out_width']) == (out_h, out_w)
        assert np.array_equal(m['calib'], DEFAULT)
        assert not tables.of(H, W).resize[0]
    assert np.array_equal(_bits(to_source[0, 0]), _bits(to_source[0, 4]))      # equal sizes, equal maps
    assert not np.array_equal(to_source[0, 0], to_source[0, 1])


class _Pipe(object):
    """Stands in for the device pipe: keeps what ``run_images`` hands it."""

    def __init__(self):
        self.calls = []

    def submit(self, i, images, side=None):
        self.calls.append(("submit", i, images, side))

    def collect(self, i, images, arrays=False):
        self.calls.append(("collect", i, images))
        return ["result"] * len(images)


def _with_pipe(det):
    pipe = _Pipe()
    det._image_pipe_for = lambda images, depth: pipe
    return pipe


def _images(shapes=((8, 9), (9, 8), (5, 5))):
    return [np.zeros((h, w, 3), np.uint8) for h, w in shapes]


@pytest.mark.parametrize("extra", [(), ("--keep_res",)])
def test_calibs_forms(extra):
    det = _host_detector(extra)           # mixed sizes under --keep_res too: the input size stays fixed
    pipe, images = _with_pipe(det), _images()
    assert det.run_images(images, KITTI) == ["result"] * 3
    side = pipe.calls[0][3]
    assert side.shape == (3, 3, 4) and side.dtype == np.float32 and side.flags.c_contiguous
    assert all(np.array_equal(m, KITTI) for m in side)
    det.run_images(images, [KITTI, None, KITTI.tolist()])
    side = pipe.calls[2][3]
    assert np.array_equal(side[0], KITTI) and np.array_equal(side[1], DEFAULT) and np.array_equal(side[2], KITTI)
    assert [c[0] for c in pipe.calls] == ["submit", "collect"] * 2 and pipe.calls[2][2] is images
    # the stream: pairs, the side array riding with its batch
    got = list(det.run_images_stream(iter([(images, KITTI), (images[::-1], [None, KITTI, None])]), depth=2))
    assert got == [["result"] * 3] * 2
    sides = [c[3] for c in pipe.calls[4:] if c[0] == "submit"]
    assert len(sides) == 2 and np.array_equal(sides[0], np.stack([KITTI] * 3))
    assert np.array_equal(sides[1], np.stack([DEFAULT, KITTI, DEFAULT]))


@pytest.mark.parametrize("bad", [[KITTI, KITTI], [KITTI] * 4, np.zeros((3, 3)), np.zeros((4, 3)),
                                 [KITTI, None, np.zeros((3, 3))], np.zeros((3, 4, 1)), "calib"])
def test_malformed_calibs_raise_value_error(bad):
    det = _host_detector()
    pipe, images = _with_pipe(det), _images()
    with pytest.raises(ValueError):
        det.run_images(images, bad)
    with pytest.raises(ValueError):
        list(det.run_images_stream([(images, bad)]))
    assert not pipe.calls


def test_argument_checks():
    det = _host_detector()
    pipe = _with_pipe(det)
    ok = np.zeros((8, 9, 3), np.uint8)
    for bad in ([ok.astype(np.float32)], [ok[:, :, 0]], []):
        with pytest.raises(ValueError):
            det.run_images(bad, KITTI)
    with pytest.raises(ValueError, match="one length"):
        list(det.run_images_stream([([ok, ok], KITTI), ([ok], KITTI)]))
    assert [c[0] for c in pipe.calls] == ["submit"]                   # the first batch of the stream only


def test_refusals():
    det = DddDetector.__new__(DddDetector)          # no opt: refused before anything else is looked at
    img = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="calibs"):
        det.run_images([img])
    with pytest.raises(NotImplementedError, match="calibs"):
        det.run_images_stream(iter([[img]]))                          # at the call, not at the first next()
    with pytest.raises(NotImplementedError, match="calibs"):
        det.run_images_stream(iter([[img, img]]))                     # two images are no (images, calibs) pair
    with pytest.raises(NotImplementedError, match="calibs"):
        det.run_images_stream([([img], None)])
    # a later item without matrices: when the generator reaches it
    det = _host_detector()
    _with_pipe(det)
    stream = det.run_images_stream([([img], KITTI), ([img], None)], depth=1)
    with pytest.raises(NotImplementedError, match="calibs"):
        list(stream)
    assert list(det.run_images_stream([])) == []
