"""The exdet frame pipe on the device: the tail kernels (cn_exdet_post_process_f32, cn_exdet_merge_f32) against
the host tail bit for bit, their refusal of bad arguments, run_batch against process(), and run_frames /
run_frames_stream against the loop of run(frame) -- with the path that produced each result asserted
(device tail, or the batch handed back to the host: ``tail_fallbacks``).  Measured agreement goes to
profiles/exdet_frame_pipe_parity.jsonl."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from centernet_amd.image import get_affine_transform
from centernet_amd.post_process import exdet_post_batch, exdet_results_batch
from oracle.parity import match_rows
from test_exdet_tail_host import CASES, NUM_CLASSES as NC, _bits, exdet_meta, exdet_rows

pytestmark = pytest.mark.gpu


def _note(name, **kw):
    try:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                            "exdet_frame_pipe_parity.jsonl")
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=name, **kw)) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------
# 1. the two kernels against the host tail on seeded rows
# ------------------------------------------------------------------------------------------------
def _device_tail(per_scale, nc=NC, max_per_image=100):
    """cn_exdet_post_process_f32 per scale + cn_exdet_merge_f32, one meta per scale for the whole batch"""
    lib = native.lib()
    S = len(per_scale)
    B, R, _ = per_scale[0][0].shape
    rows = torch.full((S, B, R, 5), float("nan"), device="cuda")
    bounds = torch.full((S, B, nc + 1), -7, dtype=torch.int32, device="cuda")
    for s, (dets, metas, scale) in enumerate(per_scale):
        m = metas[0]
        t = get_affine_transform(m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1)
        ts = torch.from_numpy(np.ascontiguousarray(t, np.float64).reshape(-1)).cuda()
        d = torch.from_numpy(np.ascontiguousarray(dets)).cuda()
        rc = lib.cn_exdet_post_process_f32(native.ptr(d), B, R, nc, int(m['out_width']), native.ptr(ts), 0, float(scale),
                                           native.ptr(rows[s]), native.ptr(bounds[s]), native.stream_ptr())
        assert rc == native.CN_OK
    cap = min(S * R, native.MERGE_MAX_ROWS)
    out_rows = torch.full((B, cap, 5), float("nan"), device="cuda")
    out_bounds = torch.full((B, nc + 1), -7, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = lib.cn_exdet_merge_f32(native.ptr(rows), native.ptr(bounds), S, B, R, nc, max_per_image, native.ptr(out_rows),
                                native.ptr(out_bounds), native.ptr(status), native.stream_ptr())
    assert rc == native.CN_OK
    torch.cuda.synchronize()
    return rows.cpu().numpy(), bounds.cpu().numpy(), out_rows.cpu().numpy(), out_bounds.cpu().numpy(), status.cpu().numpy()


def _host_grouped(dets, metas, scale, nc=NC):
    """per frame (rows (n, 5), bounds (nc + 1)): the host's post-process, filter and stable class grouping"""
    post = exdet_post_batch(dets, metas, scale)
    out = []
    for r in post:
        with np.errstate(invalid="ignore"):
            keep = (r[:, 4] > 0) & (r[:, 13] >= 0) & (r[:, 13] < nc) & (r[:, 13] == np.floor(r[:, 13]))
        r = r[keep]
        cls = r[:, 13].astype(np.int64)
        order = np.argsort(cls, kind="stable")
        out.append((r[order][:, 0:5], np.searchsorted(cls[order], np.arange(nc + 1))))
    return out


def _assert_frame(out_rows, out_bounds, want, nc=NC, what=""):
    bd = out_bounds
    assert bd[0] == 0 and bd[nc] == sum(len(v) for v in want.values()), what
    for j in range(nc):
        got = out_rows[bd[j]:bd[j + 1]]
        assert got.shape == want[j + 1].shape, (what, j)
        assert np.array_equal(_bits(got), _bits(want[j + 1])), (what, j)


DEVICE_CASES = dict(CASES)
# long class segments: most rows positive and in one class -- a segment spans every wave's rows and many steps
DEVICE_CASES["one_class"] = (2000, (1.0,), False, (300, 400), (1900, 1200, 2000))
DEVICE_CASES["two_scales_full"] = (1000, (0.5, 1.0), True, (200, 280), (1000, 1000))      # S * R rows present


@pytest.mark.parametrize("name", sorted(DEVICE_CASES))
def test_tail_kernels_equal_host_tail(dev, name):
    R, scales, keep_res, (h, w), positive = DEVICE_CASES[name]
    rng = np.random.RandomState(sorted(DEVICE_CASES).index(name) + 400)
    n = len(positive)
    per_scale = []
    for scale in scales:
        meta = exdet_meta(h, w, scale, keep_res)
        per_scale.append((exdet_rows(rng, n, R, meta['out_width'], meta['out_height'], positive,
                                     favoured=0.8 if name == "one_class" else 0.0,
                                     strays=name != "two_scales_full"), [meta] * n, scale))
    rows, bounds, out_rows, out_bounds, status = _device_tail(per_scale)
    for s, (dets, metas, scale) in enumerate(per_scale):             # the first kernel alone
        for b, (hr, hb) in enumerate(_host_grouped(dets, metas, scale)):
            assert np.array_equal(bounds[s, b], hb), (name, s, b)
            assert np.array_equal(_bits(rows[s, b, :len(hr)]), _bits(hr)), (name, s, b)
            assert not rows[s, b, len(hr):].any()                      # zeros behind the last bound
    want = exdet_results_batch(per_scale, NC)
    assert not status.any()
    for b in range(n):
        _assert_frame(out_rows[b], out_bounds[b], want[b], what=(name, b))


def test_merge_hands_back_the_frame_that_exceeds_the_cap(dev):
    """three scales, three frames; the middle one has 2400 positive rows over the scales (> CN_MERGE_MAX_ROWS):
    its status is set and its bounds are zero, its neighbours (1800 rows each) equal the host's"""
    rng = np.random.RandomState(77)
    per_scale = []
    for scale in (0.5, 1.0, 1.5):
        meta = exdet_meta(200, 280, scale, True)
        per_scale.append((exdet_rows(rng, 3, 2000, meta['out_width'], meta['out_height'], (600, 800, 600), strays=False),
                          [meta] * 3, scale))
    present = [sum(len(_host_grouped(d, m, s)[b][0]) for d, m, s in per_scale) for b in range(3)]
    assert present == [1800, 2400, 1800] and native.MERGE_MAX_ROWS == 2048
    _, _, out_rows, out_bounds, status = _device_tail(per_scale)
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    assert not out_bounds[1].any()
    want = exdet_results_batch(per_scale, NC)
    for b in (0, 2):
        _assert_frame(out_rows[b], out_bounds[b], want[b], what=b)


def test_tail_kernels_refuse_bad_arguments(dev):
    lib = native.lib()
    OK, SHAPE, NULL = native.CN_OK, -1, -5
    f = lambda *shape: torch.zeros(shape, device="cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    ts = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=torch.float64, device="cuda")
    st = native.stream_ptr()

    def post(R=10, nc=80, out_w=64, scale=1.0, B=1, dets="x", rows="x", bounds="x", t="x", alloc=10):
        d, r, b = f(1, alloc, 14), f(1, alloc, 5), i32(1, max(1, min(nc, 1024)) + 1)
        return lib.cn_exdet_post_process_f32(native.ptr(d) if dets else None, B, R, nc, out_w,
                                             native.ptr(ts) if t else None, 0, scale, native.ptr(r) if rows else None,
                                             native.ptr(b) if bounds else None, st)
    assert post() == OK
    assert post(dets=None) == NULL and post(rows=None) == NULL and post(bounds=None) == NULL and post(t=None) == NULL
    assert post(R=9) == SHAPE and post(R=0) == SHAPE and post(B=0) == SHAPE                    # odd, empty
    assert post(R=2050) == SHAPE and post(nc=1025) == SHAPE and post(nc=0) == SHAPE           # over the caps
    assert post(scale=0.0) == SHAPE and post(scale=-1.0) == SHAPE and post(scale=float("nan")) == SHAPE
    assert post(out_w=0) == SHAPE

    def merge(S=1, B=1, R=10, nc=80, mpi=100, rows="x", bounds="x", out="x", ob="x", status="x"):
        r, b = f(1, 1, 10, 5), i32(1, 1, max(1, min(nc, 1024)) + 1)
        o, o2, s = f(1, 10, 5), i32(1, max(1, min(nc, 1024)) + 1), i32(1)
        return lib.cn_exdet_merge_f32(native.ptr(r) if rows else None, native.ptr(b) if bounds else None, S, B, R, nc, mpi,
                                      native.ptr(o) if out else None, native.ptr(o2) if ob else None,
                                      native.ptr(s) if status else None, st)
    assert merge() == OK
    for k in ("rows", "bounds", "out", "ob", "status"):
        assert merge(**{k: None}) == NULL, k
    assert merge(R=9) == SHAPE and merge(R=2050) == SHAPE and merge(nc=1025) == SHAPE and merge(nc=0) == SHAPE
    assert merge(S=0) == SHAPE and merge(B=0) == SHAPE and merge(mpi=0) == SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. the detector: run_batch, run_frames, run_frames_stream
# ------------------------------------------------------------------------------------------------
def _favour_one_class(model, cls=17, by=3.0):
    """(tests/test_gpu_tasks.py) random heads never agree on a class: one class is favoured in the last layer
    of the five maps, as a trained net's dominant object would be"""
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.split(".")[0] in ("hm_t", "hm_l", "hm_b", "hm_r", "hm_c") and k.endswith("bias") and v.numel() == 80:
                v[cls] += by


def _build(extra):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["exdet", "--arch", "hourglass", "--input_res", "256", "--K", "40", "--scores_thresh", "0",
                           "--center_thresh", "0"] + extra)
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


@pytest.fixture(scope="module")
def hourglass(dev):
    det = _build(["--flip_test"])
    _favour_one_class(det.model)
    return det


@pytest.fixture(scope="module")
def hourglass_agnostic(dev):
    return _build(["--flip_test", "--agnostic_ex"])


def _configure(det, flip, scales=(1.0,), K=40):
    """one network serves every configuration: the options the pipe and run() read"""
    det.opt.flip_test = bool(flip)
    det.opt.test_scales = list(scales)
    det.scales = list(scales)
    det.opt.K = K
    det.tail_fallbacks = 0
    return det


def _frames(seed, n, h=256, w=256):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


def _agreement(got, ref):
    """(rows of the run() side, rows of the pipe's side, run() rows with a nearest pipe row within 5e-3 in all
    five columns) -- the bar of test_exdet_detector_matches_the_oracle_pipeline"""
    n_ref = sum(len(v) for v in ref.values())
    n_got = sum(len(v) for v in got.values())
    same = 0
    for j in ref:
        assert got[j].dtype == np.float32 and got[j].ndim == 2 and got[j].shape[1] == 5
        if len(ref[j]) and len(got[j]):
            d = np.abs(got[j][:, None, :].astype(np.float64) - ref[j][None, :, :]).max(axis=2)
            same += int((d.min(axis=0) < 5e-3).sum())
    return n_ref, n_got, same


def _pipe_raw(det, frames):
    """the pipe's own raw rows of every test scale for these frames (its batch tensors still hold them)"""
    pipe = det._pipe_for(frames, 1)
    per_scale = []
    for lv in pipe.levels:
        raw = det._run_scale(lv.batch, pipe.flip).cpu().numpy()
        per_scale.append((raw, [lv.meta] * len(frames), lv.scale))
    assert det.range_ok()
    return per_scale


def _check_against_run(det, frames, name, device_tail):
    got = det.run_frames(frames)
    fallbacks = det.tail_fallbacks
    per_scale = _pipe_raw(det, frames)
    positive = [int(sum((d[b, :, 4] > 0).sum() for d, _, _ in per_scale)) for b in range(len(frames))]
    if device_tail:
        assert max(positive) <= native.MERGE_MAX_ROWS, positive
        assert fallbacks == 0 and det._pipe_for(frames, 1).tail is not None
        # the device tail against the host tail on the pipe's own raw rows: bit equal
        host = exdet_results_batch(per_scale, det.num_classes, det.max_per_image)
        for b in range(len(frames)):
            assert sorted(got[b]) == list(range(1, det.num_classes + 1))
            for j in host[b]:
                assert got[b][j].shape == host[b][j].shape and np.array_equal(_bits(got[b][j]), _bits(host[b][j])), (name, b, j)
    else:
        assert max(positive) > native.MERGE_MAX_ROWS, positive
        assert fallbacks > 0
    stats = []
    for b, f in enumerate(frames):
        ref = det.run(f)["results"]
        n_ref, n_got, same = _agreement(got[b], ref)
        stats.append(dict(rows_run=n_ref, rows_pipe=n_got, same=same, positive_rows=positive[b]))
    _note(name, frames=stats, tail_fallbacks=fallbacks)
    print(name, stats, "tail_fallbacks", fallbacks)
    for s in stats:
        assert s["rows_run"] > 0
        assert abs(s["rows_pipe"] - s["rows_run"]) <= max(2, s["rows_run"] // 20), s
        assert s["same"] >= 0.9 * s["rows_run"], s
    return got


def test_run_batch_matches_process(dev, hourglass):
    det = _configure(hourglass, True)
    images, _ = det.pre_process(_frames(12, 1)[0], 1.0)
    x = images.to(dev)
    assert tuple(x.shape) == (2, 3, 256, 256)
    raw = det.run_batch(x.clone()).cpu().numpy()
    assert raw.shape == (2, 1000, 14) and det.range_ok()
    _, dets = det.process(x.clone())
    ref = dets.cpu().numpy()
    tol = np.array([2e-3] * 4 + [1e-4] + [2e-3] * 8 + [0.0])
    fr = []
    for b in range(2):
        m = match_rows(raw[b][:320], ref[b][:320], list(range(14)), tol, window=20)
        fr.append(float((m[:300] >= 0).mean()))
    _note("run_batch_vs_process", paired=fr, valid_rows=int((ref[..., 4] > 0).sum()))
    assert min(fr) >= 0.95, fr
    assert tuple(det._run_scale(x.clone(), True).shape) == (1, 2000, 14)
    assert tuple(det._run_scale(x.clone(), False).shape) == (2, 1000, 14)
    assert det.range_ok()


def test_run_frames_flip_single_scale(dev, hourglass):
    det = _configure(hourglass, True)
    _check_against_run(det, _frames(21, 2), "flip_single_scale", device_tail=True)


def test_run_frames_without_flip(dev, hourglass):
    """--K 12: 20736 groupings per image, about one in a hundred valid with these weights, so a few hundred of the
    1000 rows are positive and their scores are spread.  At --K 40 the 1000 rows are the top of 2.56 million
    groupings: measured, their scores lie within 0.0044 of each other (980 distinct values, about 4e-6 apart),
    while the network's own rows for a frame differ by up to 1.2e-5 in score between a batch of one (run) and a
    batch of two (the pipe) -- which 100 rows soft-NMS and the cut leave is then decided by that rounding, not
    by the tail: the HOST tail on the two sets of raw rows agreed on 74 of 100 rows for one frame (100 of 100
    for the other), the device tail being bit equal to the host tail on both."""
    det = _configure(hourglass, False, K=12)
    _check_against_run(det, _frames(22, 2), "no_flip", device_tail=True)


def test_run_frames_agnostic(dev, hourglass_agnostic):
    det = _configure(hourglass_agnostic, True)
    _check_against_run(det, _frames(23, 2), "agnostic_ex", device_tail=True)


def test_run_frames_multi_scale_on_the_device(dev, hourglass):
    """two test scales with flip-test: S * R = 4000 rows per frame, of which the positive ones must fit the merge
    kernel.  --K 12 leaves 20736 groupings per image, about one in a hundred of them valid with these weights
    (the others carry the decode's rejections, score -1): a few hundred positive rows per image, four images per
    frame -- under the cap of 2048, which is asserted."""
    det = _configure(hourglass, True, scales=(0.5, 1.0), K=12)
    _check_against_run(det, _frames(24, 2), "multi_scale_device", device_tail=True)


def test_run_frames_multi_scale_overflow_goes_to_the_host(dev, hourglass):
    """thresholds at 0 and --K 40: every one of the 4000 rows of a frame is positive -- the merge kernel hands the
    batch back, the pipe runs it through _run_frames_sync: the same bits, and counted"""
    det = _configure(hourglass, True, scales=(0.5, 1.0), K=40)
    frames = _frames(25, 2)
    got = _check_against_run(det, frames, "multi_scale_overflow", device_tail=False)
    want = det._run_frames_sync(frames, det.scales)
    for b in range(len(frames)):
        for j in want[b]:
            assert got[b][j].shape == want[b][j].shape and np.array_equal(_bits(got[b][j]), _bits(want[b][j])), (b, j)


def test_stream_equals_run_frames_batch_by_batch(dev, hourglass):
    det = _configure(hourglass, True)
    batches = [_frames(30 + i, 2) for i in range(4)]
    streamed = list(det.run_frames_stream(iter(batches), depth=2))
    assert len(streamed) == len(batches) and det.tail_fallbacks == 0
    for batch, got in zip(batches, streamed):
        want = det.run_frames(batch)
        for b in range(len(batch)):
            for j in want[b]:
                assert got[b][j].shape == want[b][j].shape and np.array_equal(_bits(got[b][j]), _bits(want[b][j])), (b, j)
    assert det.tail_fallbacks == 0


def test_more_classes_than_the_kernels_take_keep_the_host_tail(dev, hourglass):
    det = _configure(hourglass, True)
    pipe = det._pipe_for(_frames(1, 2), 1)
    assert pipe.tail is not None and pipe.tail.R == 2000
    nc, det.num_classes = det.num_classes, native.MERGE_MAX_CLASSES + 1
    try:
        assert det._device_tail(pipe) is None
    finally:
        det.num_classes = nc
