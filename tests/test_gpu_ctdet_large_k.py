"""CtdetDetector with --K in (128, 1024]: the large-K top-K (csrc/cn_decode_large.hip) on the dense wh / reg maps
and the host tails, through every entry of the detector.  resdcn_18 with seeded weights at a 128 x 128 input, the
smallest the plans take that gives a 32 x 32 map."""
import contextlib
import sys

import numpy as np
import pytest
import torch

from centernet_amd import synth
from test_gpu_frames_tta import _assert_close_multi
from test_gpu_heads_at_cells import TOL

pytestmark = pytest.mark.gpu
SMALL = ["--arch", "resdcn_18", "--input_h", "128", "--input_w", "128"]


def _build(args):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet"] + SMALL + list(args))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what=""):
    """two lists of per-image results, bit for bit"""
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb)
        for j in ra:
            x, y = np.asarray(ra[j], np.float32), np.asarray(rb[j], np.float32)
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i, j)


@pytest.fixture(scope="module")
def det300(dev):
    return _build(["--K", "300", "--max_per_image", "300"])


def test_run_returns_all_rows(dev, det300):
    assert det300.max_per_image == 300 and det300.model.deferred_names() == ()
    res = det300.run(_img(100, 140, 1))["results"]
    assert sorted(res) == list(range(1, 81))
    assert all(v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == 5 for v in res.values())
    assert sum(len(v) for v in res.values()) == 300
    assert all(np.isfinite(v).all() for v in res.values())


def test_pipes_give_what_run_gives(dev, det300):
    """run_frames, run_images and run_frames_stream against run per frame, bit for bit; the host tail serves them."""
    frames = [_img(100, 140, 1), _img(100, 140, 2)]
    want = [det300.run(f)["results"] for f in frames]
    pipe = det300._pipe_for(frames, 1)
    assert pipe.tail is None and det300._device_tail(pipe) is None          # K > 128: no device tail
    got = det300.run_frames(frames)
    assert sum(len(v) for v in got[0].values()) == 300
    for name, res in (("run_frames", got), ("run_images", det300.run_images(frames)),
                      ("run_frames_stream", list(det300.run_frames_stream(iter([frames, frames[::-1]])))[0])):
        worst = max(float(np.abs(np.asarray(a[j]) - np.asarray(b[j])).max()) if a[j].shape == b[j].shape and len(a[j])
                    else 0.0 for a, b in zip(res, want) for j in a)
        print("%s against run: max |diff| = %.3e" % (name, worst))
        _same(res, want, name)
    mixed = [_img(100, 140, 1), _img(64, 48, 3)]
    _same(det300.run_images(mixed), [det300.run(f)["results"] for f in mixed], "run_images, mixed sizes")
    assert det300.tail_fallbacks == 0


def test_first_rows_are_the_rows_of_k100(dev):
    """K = 100 runs the heads at the decoded cells, K = 300 the dense heads: same scores and classes bit for bit in
    the first 100 rows, boxes within the bar of the deferred-against-dense test (tests/test_gpu_heads_at_cells.py).
    Two fresh detectors: the f32s exponents of a network are calibrated on the first batch it sees, so both must
    see this batch first for `hm` to be the same bits."""
    det100, det300 = _build(["--K", "100"]), _build(["--K", "300", "--max_per_image", "300"])
    assert det100.model.deferred_names() == ("wh", "reg") and det300.model.deferred_names() == ()
    x = synth.images(2, 128, 128, seed=5).to(dev)
    big = det300.run_batch(x).clone()
    small = det100.run_batch(x).clone()
    torch.cuda.synchronize()
    assert det300.range_ok() and det100.range_ok()
    assert tuple(big.shape) == (2, 300, 6) and tuple(small.shape) == (2, 100, 6)
    got, want = big[:, :100].cpu(), small.cpu()
    for col in (4, 5):
        assert np.array_equal(_bits(got[..., col].numpy()), _bits(want[..., col].numpy()))
    err = ((got[..., :4] - want[..., :4]).abs() / (1 + want[..., :4].abs())).max()
    print("K = 300 dense against K = 100 deferred: max box |diff| / (1 + |value|) = %.3e" % float(err))
    assert float(err) < TOL, float(err)
    s = big[..., 4]
    assert bool((s[:, 1:] <= s[:, :-1]).all())


def test_flip_scales_nms(dev):
    det = _build(["--flip_test", "--test_scales", "0.5,1", "--nms", "--K", "200"])
    frames = [_img(100, 140, 4), _img(100, 140, 5)]
    pipe = det._pipe_for(frames, 1)
    assert pipe.tail is None
    batched = det.run_frames(frames)
    for f, rb in zip(frames, batched):
        _assert_close_multi(rb, det.run(f)["results"])
    _same(det.run_images(frames), batched, "run_images")


def test_fp16(dev):
    det = _build(["--fp16", "--K", "200"])
    x = synth.images(2, 128, 128, seed=6).to(dev)
    dets = det.run_batch(x).clone()
    torch.cuda.synchronize()
    assert tuple(dets.shape) == (2, 200, 6) and bool(torch.isfinite(dets).all())
    s = dets[..., 4]
    assert bool((s[:, 1:] <= s[:, :-1]).all()) and bool((s > 0).all()) and bool((s < 1).all())
    res = det.run(_img(100, 140, 7))["results"]
    assert sum(len(v) for v in res.values()) == 100                        # the default --max_per_image


def test_run_tiles(dev, det300):
    """Tiles at K = 300: the tile merge on the host (the device merge takes K <= 128), the pipe against the
    synchronous path."""
    frames = [_img(200, 260, 8)]
    args = det300._tiles_args(None, None, 32, None)
    pipe = det300._tile_pipe_for(frames, 1, *args, 'bgr')
    assert pipe.tail is None
    got = det300.run_tiles(frames)
    _same(got, det300._run_tiles_sync(frames, *args), "run_tiles")
    assert 0 < sum(len(v) for v in got[0].values()) <= 300


def test_k_above_the_limit_is_refused(dev):
    with pytest.raises((ValueError, RuntimeError), match="1024"):
        _build(["--K", "1025"]).run(_img(100, 140, 9))
    assert _build(["--K", "1024", "--max_per_image", "1024"]).run_batch(
        synth.images(1, 128, 128, seed=9).to(dev)).shape == (1, 1024, 6)
