"""The ddd frame pipe on the device: cn_warp_table_u8_f32_batch against the oracle's pre-process (bit for bit),
cn_ddd_post_process_f32 against the oracle's ddd_results + ddd_merge_outputs (every row; columns 1-10 and 12 bit
for bit, the two angle columns inside a bar derived from NumPy's own float32 arctan2 error), the depth flag of
cn_ddd_decode_f32, and run_frames / run_frames_stream built on them."""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from centernet_amd.decode import ddd_decode
from centernet_amd.image import invert_affine
from centernet_amd.post_process import ddd_norm_table, ddd_results_batch
from oracle import post_oracle, pre_oracle
from test_ddd_tail_host import KITTI, NUM_CLASSES, OUT_H, OUT_W, _bits, calib_like, ddd_meta, ddd_rows
from test_gpu_tasks import _paired_fraction

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]
ULP = 2.0 ** -22            # one ulp of a float32 in [2, 4)
TWO_PI = 2 * np.pi


def _note(**kw):
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ddd_frame_pipe_parity.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------
# 1. warp + table normalise
# ------------------------------------------------------------------------------------------------
def _host_detector(extra=()):
    from centernet_amd.detectors.ddd import DddDetector
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ddd"] + list(extra))
    det = DddDetector.__new__(DddDetector)
    det.opt, det.num_classes = opt, opt.num_classes
    det.mean = np.asarray(opt.mean, np.float32).reshape(1, 1, 3)
    det.std = np.asarray(opt.std, np.float32).reshape(1, 1, 3)
    return det, opt


WARP_CASES = [  # (frame (h, w), opts, N)
    ((375, 1242), (), 3),
    ((375, 1242), (), 1),
    ((188, 621), ("--keep_res",), 1),
    ((64, 96), ("--input_h", "64", "--input_w", "128"), 32),
    ((50, 70), ("--input_h", "64", "--input_w", "128", "--keep_res"), 3),
]


@pytest.mark.parametrize("case", range(len(WARP_CASES)))
def test_warp_table_kernel_equals_the_oracle_pre_process(dev, case):
    (h, w), extra, N = WARP_CASES[case]
    det, opt = _host_detector(extra)
    rng = np.random.RandomState(800 + case)
    frames = rng.randint(0, 256, (N, h, w, 3)).astype(np.uint8)
    _, _, to_input = det._frame_geometry(h, w)
    m = (ctypes.c_double * 6)(*invert_affine(to_input).reshape(-1))
    src = torch.from_numpy(frames).to(dev)
    table = torch.from_numpy(ddd_norm_table(det.mean, det.std)).to(dev)
    out = torch.full((N, 3, opt.input_h, opt.input_w), float("nan"), device=dev)
    rc = native.lib().cn_warp_table_u8_f32_batch(native.ptr(src), N, h * w * 3, h, w, w * 3, m, opt.input_h,
                                                 opt.input_w, native.ptr(table), native.ptr(out), native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == native.CN_OK
    got = out.cpu().numpy()
    assert torch.equal(src.cpu(), torch.from_numpy(frames))
    for n in range(N):
        want, _ = pre_oracle.ddd_pre_process(frames[n], opt.mean, opt.std, opt.input_h, opt.input_w,
                                             keep_res=bool(opt.keep_res))
        assert want.shape == (1, 3, opt.input_h, opt.input_w)
        assert np.array_equal(_bits(got[n]), _bits(want[0])), (case, n)


def test_warp_table_kernel_refuses_bad_arguments(dev):
    t = torch.zeros((3, 256), device=dev)
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros((1, 3, 8, 8), device=dev)
    m = (ctypes.c_double * 6)(1, 0, 0, 0, 1, 0)
    call = native.lib().cn_warp_table_u8_f32_batch
    assert call(native.ptr(src), 1, 0, 8, 8, 24, m, 8, 8, None, native.ptr(out), native.stream_ptr()) == -5
    assert call(native.ptr(src), 0, 0, 8, 8, 24, m, 8, 8, native.ptr(t), native.ptr(out), native.stream_ptr()) == -1
    assert call(native.ptr(src), 1, 0, 8, 8, 23, m, 8, 8, native.ptr(t), native.ptr(out), native.stream_ptr()) == -1
    assert call(native.ptr(src), 2, 8, 8, 8, 24, m, 8, 8, native.ptr(t), native.ptr(out), native.stream_ptr()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. the tail kernel
# ------------------------------------------------------------------------------------------------
def _arctan2_gap(y, x):
    """largest |NumPy float32 arctan2 - float64 arctan2 rounded to float32| over the given arguments"""
    y, x = np.asarray(y, np.float32).ravel(), np.asarray(x, np.float32).ravel()
    if not len(y):
        return 0.0
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    return float(np.abs(np.arctan2(y, x).astype(np.float64) - ref.astype(np.float64)).max())


def angle_bars(dets, metas):
    """U over the arguments of both arctan2 of these rows, and the two bars of the issue: alpha = U + the
    device's own rounding + the float32 add of +-pi/2 (2 * 2^-22); rotation_y = that + U + 2 * 2^-22 for the
    second arctan2 and its add."""
    u = max(_arctan2_gap(dets[:, :, 5], dets[:, :, 6]), _arctan2_gap(dets[:, :, 9], dets[:, :, 10]))
    for b, m in enumerate(metas):
        cx = post_oracle.transform_preds(dets[b, :, 0:2], m['c'], m['s'], (m['out_width'], m['out_height']))
        cx = cx.astype(np.float32)[:, 0]
        u = max(u, _arctan2_gap(cx - m['calib'][0, 2], np.full(len(cx), m['calib'][0, 0], np.float32)))
    alpha = u + 2 * ULP
    return u, alpha, alpha + u + 2 * ULP


def _angle_diff(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.minimum(d, np.abs(TWO_PI - d))


def compare_rows(got, want, bars, seen, where):
    """one class of one image, every row: exact columns bit for bit, angles inside their bars"""
    assert got.shape == want.shape and got.dtype == np.float32, (where, got.shape, want.shape)
    if want.ndim == 1 or not len(want):
        return
    bad = np.argwhere(_bits(got[:, EXACT]) != _bits(want[:, EXACT]))
    assert not len(bad), (where, bad[:4], [(got[:, EXACT][tuple(i)], want[:, EXACT][tuple(i)]) for i in bad[:4]])
    da, dr = _angle_diff(got[:, 0], want[:, 0]).max(), _angle_diff(got[:, 11], want[:, 11]).max()
    seen[0], seen[1] = max(seen[0], float(da)), max(seen[1], float(dr))
    assert da <= bars[1] and dr <= bars[2], (where, da, dr, bars)


def _tail_call(dets, mats, per_image, calibs, thresh, cols=18, K=None):
    B, K0, _ = dets.shape
    K = K0 if K is None else K
    d = torch.from_numpy(dets).cuda()
    t = torch.from_numpy(np.ascontiguousarray(mats, np.float64).reshape(-1)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(calibs, np.float32)).cuda()
    rows = torch.full((B, K0, 13), float("nan"), device="cuda")
    bounds = torch.full((B, NUM_CLASSES + 1), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((B, NUM_CLASSES), -1, dtype=torch.int32, device="cuda")
    rc = native.lib().cn_ddd_post_process_f32(native.ptr(d), B, K, cols, NUM_CLASSES, native.ptr(t), int(per_image),
                                              native.ptr(p), float(thresh), native.ptr(rows), native.ptr(bounds),
                                              native.ptr(kept), native.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), torch.from_numpy(dets))          # the input is only read
    return rc, rows.cpu().numpy(), bounds.cpu().numpy(), kept.cpu().numpy()


TAIL_CASES = [(B, K, per_image, fill)
              for K, fill in ((1, "mixed"), (40, "empty"), (100, "stray"), (128, "mixed"))
              for B in (1, 3, 32) for per_image in (False, True)]


@pytest.mark.parametrize("case", range(len(TAIL_CASES)))
def test_tail_kernel_equals_the_oracle_row_by_row(dev, case):
    B, K, per_image, fill = TAIL_CASES[case]
    rng = np.random.RandomState(900 + case)
    thresh = 0.45
    dets = ddd_rows(rng, B, K, fill)
    metas = []
    for b in range(B):
        m = ddd_meta(calib=calib_like(rng) if per_image else KITTI)
        if per_image:           # other frame sizes: B different inverse maps
            m['c'] = (m['c'] + rng.uniform(-40, 40, 2)).astype(np.float32)
            m['s'] = (m['s'] * rng.uniform(0.8, 1.2)).astype(np.int32)
        metas.append(m)
    mats = np.stack([post_oracle.get_affine_transform(m['c'], m['s'], 0, (OUT_W, OUT_H), inv=1)
                     for m in (metas if per_image else metas[:1])])
    rc, rows, bounds, kept = _tail_call(dets, mats, per_image, np.stack([m['calib'] for m in metas]), thresh)
    assert rc == native.CN_OK
    bars, seen, n_rows = angle_bars(dets, metas), [0.0, 0.0], 0
    for b in range(B):
        full = post_oracle.ddd_results(dets[b][None], metas[b], NUM_CLASSES, OUT_W, OUT_H)
        cut = post_oracle.ddd_merge_outputs([dict(full)], NUM_CLASSES, thresh)
        want_bounds = np.cumsum([0] + [len(full[j]) for j in (1, 2, 3)])
        assert np.array_equal(bounds[b], want_bounds), (b, bounds[b], want_bounds)
        assert np.array_equal(kept[b], [len(cut[j]) for j in (1, 2, 3)]), (b, kept[b])
        for j in (1, 2, 3):
            lo, hi = bounds[b][j - 1], bounds[b][j]
            if hi > lo:
                compare_rows(rows[b, lo:hi], full[j], bars, seen, (case, b, j))
                compare_rows(rows[b, lo:lo + kept[b][j - 1]], cut[j], bars, seen, (case, b, j, "cut"))
            else:
                assert full[j].shape == (0,)
            n_rows += hi - lo
        # rows of no class lie behind the last bound, in their order: the oracle on them alone, as class 0
        stray = ~np.isin(dets[b, :, 17], [0.0, 1.0, 2.0])
        assert stray.sum() == K - bounds[b][3]
        if stray.any():
            relabelled = dets[b][stray].copy()
            relabelled[:, 17] = 0
            want = post_oracle.ddd_results(relabelled[None], metas[b], NUM_CLASSES, OUT_W, OUT_H)[1]
            compare_rows(rows[b, bounds[b][3]:], want, bars, seen, (case, b, "stray"))
            n_rows += int(stray.sum())
    assert n_rows == B * K                           # every row was compared
    _note(test="tail_kernel", B=B, K=K, per_image=per_image, fill=fill, U=bars[0], alpha_bar=bars[1],
          rotation_y_bar=bars[2], alpha_max=seen[0], rotation_y_max=seen[1])


def test_tail_kernel_refuses_what_it_does_not_take(dev):
    rng = np.random.RandomState(950)
    meta = ddd_meta()
    mats = post_oracle.get_affine_transform(meta['c'], meta['s'], 0, (OUT_W, OUT_H), inv=1)[None]
    calibs = np.stack([KITTI] * 2)
    wide = ddd_rows(rng, 2, 130)
    assert _tail_call(wide, mats, False, calibs, 0.2)[0] == -2                   # K > 128: CN_ERR_UNSUPPORTED
    narrow = np.ascontiguousarray(ddd_rows(rng, 2, 40)[:, :, :16])
    assert _tail_call(narrow, mats, False, calibs, 0.2, cols=16)[0] == -2        # no (w, h) columns
    assert _tail_call(ddd_rows(rng, 2, 40), mats, False, calibs, 0.2, cols=17)[0] == -1
    assert _tail_call(ddd_rows(rng, 2, 40), mats, False, calibs, 0.2, K=0)[0] == -1
    lib = native.lib()
    assert lib.cn_ddd_post_process_f32(None, 1, 1, 18, 3, None, 0, None, 0.2, None, None, None, None) == -5


# ------------------------------------------------------------------------------------------------
# 3. the depth flag of the decode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,K", [(1, 96, 320, 100), (3, 32, 96, 40), (32, 32, 96, 128)])
def test_decode_depth_flag_equals_the_torch_transform(dev, B, H, W, K):
    g = torch.Generator().manual_seed(B * 1000 + K)
    heat, rot, dep, dim, wh, reg = (torch.randn((B, c, H, W), generator=g).mul_(s).to(dev)
                                    for c, s in ((3, 2.0), (8, 1.0), (1, 3.0), (3, 1.0), (2, 4.0), (2, 0.3)))
    keep = dep.clone()
    got = ddd_decode(heat, rot, dep, dim, wh=wh, reg=reg, K=K, apply_sigmoid=True, raw_depth=True).cpu().numpy()
    ref = ddd_decode(heat, rot, 1. / (dep.sigmoid() + 1e-6) - 1., dim, wh=wh, reg=reg, K=K,
                     apply_sigmoid=True).cpu().numpy()
    plain = ddd_decode(heat, rot, dep, dim, wh=wh, reg=reg, K=K, apply_sigmoid=True).cpu().numpy()
    assert torch.equal(dep, keep)
    others = [c for c in range(18) if c != 11]
    assert np.array_equal(_bits(got[:, :, others]), _bits(ref[:, :, others]))
    err = np.abs(got[:, :, 11].astype(np.float64) - ref[:, :, 11])
    print("depth flag: max err %.3g, max err / bar %.3g" % (err.max(), (err / (2e-4 + 2e-3 * np.abs(ref[:, :, 11]))).max()))
    assert np.all(err <= 2e-4 + 2e-3 * np.abs(ref[:, :, 11]))
    # without the bit nothing changes: the map's values as they are
    assert np.array_equal(_bits(plain[:, :, others]), _bits(ref[:, :, others]))
    flat = dep.cpu().numpy().reshape(B, -1)
    assert all(np.isin(plain[b, :, 11], flat[b]).all() for b in range(B))


# ------------------------------------------------------------------------------------------------
# 4. the frame pipe
# ------------------------------------------------------------------------------------------------
def _detector(args=()):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ddd", "--input_h", "128", "--input_w", "384", "--K", "40"] + list(args))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


def _frames(seed, n, h=96, w=300):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


def _calibs(seed, n):
    rng = np.random.RandomState(seed)
    return [calib_like(rng) for _ in range(n)]


def _raw_rows(det, frames, calibs):
    """the pipe's own raw rows of a batch (the network is deterministic: the batch tensor run again)"""
    pipe = det._pipe_for(frames, 1)
    assert pipe.tail is not None
    pipe.submit(0, frames, det._calibs_for(frames, calibs))
    pipe.collect(0, frames)
    raw = det._run_scale(pipe.batch, False).detach().cpu().numpy()
    assert det.range_ok()
    return pipe, raw


def _threshold_inside(scores):
    """--peak_thresh in the middle of the widest gap between neighbouring scores of the central ranks"""
    sc = np.sort(np.asarray(scores).ravel())[::-1]
    lo, hi = len(sc) // 4, 3 * len(sc) // 4
    k = lo + int(np.argmax(sc[lo:hi] - sc[lo + 1:hi + 1]))
    return float((sc[k] + sc[k + 1]) / 2)


def _same_results(a, b):
    assert sorted(a) == sorted(b)
    for j in a:
        assert a[j].shape == b[j].shape and a[j].dtype == b[j].dtype == np.float32, (j, a[j].shape, b[j].shape)
        assert np.array_equal(_bits(a[j]), _bits(b[j])), j


def test_run_frames_equals_the_host_tail_on_its_own_raw_rows(dev):
    det, opt = _detector()
    frames, calibs = _frames(51, 4), _calibs(52, 4)
    calibs[2] = None                                              # the detector's default matrix
    pipe, raw = _raw_rows(det, frames, calibs)
    assert raw.shape == (4, 40, 18)
    opt.peak_thresh = _threshold_inside(raw[0, :, 2])
    got = det.run_frames(frames, calibs)
    side = det._calibs_for(frames, calibs)
    assert np.array_equal(side[2], det.calib)
    metas = [dict(pipe.meta, calib=p) for p in side]
    want = ddd_results_batch(raw, metas, opt.num_classes, opt.peak_thresh)
    bars, seen = angle_bars(raw, metas), [0.0, 0.0]
    assert len(got) == len(want) == 4
    kept = 0
    for b in range(4):
        assert sorted(got[b]) == [1, 2, 3]
        for j in (1, 2, 3):
            compare_rows(got[b][j], want[b][j], bars, seen, (b, j))
            kept += len(want[b][j])
    assert 0 < kept < 4 * 40                                       # a real cut
    _note(test="pipe_vs_host_tail", U=bars[0], alpha_bar=bars[1], rotation_y_bar=bars[2], alpha_max=seen[0],
          rotation_y_max=seen[1])
    pinned = pipe.tail.host('rows', 0).numpy()
    assert not any(np.shares_memory(r[j], pinned) for r in got for j in r)


def test_run_frames_stream_equals_run_frames_batch_by_batch(dev):
    det, opt = _detector()
    batches = [(_frames(60 + i, 3), _calibs(70 + i, 3)) for i in range(5)]
    _, raw = _raw_rows(det, *batches[0])
    opt.peak_thresh = _threshold_inside(raw[:, :, 2])
    alone = [det.run_frames(f, c) for f, c in batches]
    streamed = list(det.run_frames_stream(iter(batches), depth=2))
    assert len(streamed) == len(batches)
    for ra, rs in zip(alone, streamed):
        assert len(ra) == len(rs) == 3
        for a, b in zip(ra, rs):
            _same_results(a, b)
    assert any(len(r[j]) for ra in alone for r in ra for j in r)


def test_run_frames_against_run_frame_by_frame(dev):
    """Batch-size-dependent summation order rules out bit equality: the paired-row bars of
    test_ddd_detector_matches_the_oracle_pipeline."""
    det, opt = _detector()
    frames, calibs = _frames(81, 3), _calibs(82, 3)
    _, raw = _raw_rows(det, frames, calibs)
    opt.peak_thresh = _threshold_inside(raw[:, :, 2])
    batched = det.run_frames(frames, calibs)
    n_rows = 0
    for f, p, rb in zip(frames, calibs, batched):
        one = det.run(f, p)["results"]
        top = lambda r: np.sort(np.concatenate([r[j][:, 12] for j in r if len(r[j])]))[::-1]
        sa, sb = top(rb), top(one)
        n = min(len(sa), len(sb))
        assert abs(len(sa) - len(sb)) <= 1 and n > 0
        assert np.abs(sa[:n] - sb[:n]).max() < 1e-4                # scores
        for j in (1, 2, 3):
            assert abs(len(rb[j]) - len(one[j])) <= 1
            if len(one[j]) == 0:
                continue
            frac = _paired_fraction(rb[j], one[j], EXACT, 2e-2, 2e-3, window=8)
            ang = _paired_fraction(rb[j], one[j], [0, 11, 12], 2e-3, 1e-3, window=8)
            assert frac >= 0.95 and ang >= 0.9, (j, frac, ang)
            n_rows += len(one[j])
    assert n_rows > 10


def test_equal_pixels_with_different_matrices(dev):
    det, opt = _detector()
    frame = _frames(91, 1)[0]
    frames, calibs = [frame, frame.copy(), frame.copy()], [KITTI, calib_like(np.random.RandomState(92)), KITTI]
    _, raw = _raw_rows(det, frames, calibs)
    opt.peak_thresh = _threshold_inside(raw[0, :, 2])
    a, b, c = det.run_frames(frames, calibs)
    _same_results(a, c)
    flat = [0, 1, 2, 3, 4, 5, 6, 7, 12]              # alpha, the 2-D box, the dimensions, the score
    n = 0
    for j in (1, 2, 3):
        assert a[j].shape == b[j].shape
        if len(a[j]):
            assert np.array_equal(_bits(a[j][:, flat]), _bits(b[j][:, flat]))
            assert not np.array_equal(a[j][:, 8:11], b[j][:, 8:11])         # another camera: other locations
            n += len(a[j])
    assert n > 0


def test_one_matrix_serves_every_frame(dev):
    det, opt = _detector()
    frames = _frames(95, 3)
    _, raw = _raw_rows(det, frames, KITTI)
    opt.peak_thresh = _threshold_inside(raw[:, :, 2])
    for one, many in zip(det.run_frames(frames, KITTI), det.run_frames(frames, [KITTI] * 3)):
        _same_results(one, many)
    for one, many in zip(next(iter(det.run_frames_stream([(frames, KITTI.tolist())]))), det.run_frames(frames, [KITTI] * 3)):
        _same_results(one, many)


def test_pre_process_device_equals_the_host_form(dev):
    det, opt = _detector()
    frame = _frames(97, 1)[0]
    host, meta_h = det.pre_process(frame, 1.0, KITTI)
    got, meta_d = det.pre_process_device(frame, 1.0, KITTI)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(host.numpy()))
    assert sorted(meta_h) == sorted(meta_d) and all(np.array_equal(meta_h[k], meta_d[k]) for k in meta_h)
    uploaded, _ = det.pre_process_device(torch.from_numpy(frame).to(dev), 1.0)
    assert torch.equal(uploaded, got)
