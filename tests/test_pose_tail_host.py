"""The multi_pose device tail, the parts that need no GPU.

1. The form of soft-NMS that ``multi_pose_merge_kernel`` (cn_tail.hip) runs on 39-column rows, restated
   in numpy: only boxes and scores move during the greedy steps; which input row's joints sit at a position
   is tracked in ``jsrc`` (exchanged by the argmax swap and by every discard) and the joints are gathered
   once at the end.  Held equal to ``soft_nms_39`` (``cn_soft_nms_f32``, pinned to the reference's cython
   in test_oracle_ref.py) on seeded arrays: the whole in-place array, rows past the kept count included.
2. The C ABI of ``cn_multi_pose_post_process_f32`` / ``cn_multi_pose_merge_f32``: exported, declared,
   bound, and their argument checks, which return before any HIP call.
3. ``arrays=True`` of the frame pipeline on the host-tail path: the same bits as the list form."""
import ctypes
import inspect
import os
import re
import types

import numpy as np

from centernet_amd import native
from centernet_amd.soft_nms import soft_nms_39

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 8, 30, 90, 500)
SEEDS = range(20000, 21050)


def _decay(box, sc, i, N, sigma, threshold):
    """Decayed score and discard flag of every row p in (i, N), lane-parallel (cn_soft_nms_f32's terms)."""
    t = box[i]
    b = box[i + 1:N]
    x1, y1, x2, y2, s = b[:, 0], b[:, 1], b[:, 2], b[:, 3], sc[i + 1:N]
    area = ((np.float64(1.0) + (x2 - x1)) * (np.float64(1.0) + (y2 - y1))).astype(F32)
    iw = ((np.minimum(t[2], x2) - np.maximum(t[0], x1)).astype(np.float64) + 1.0).astype(F32)
    ih = ((np.minimum(t[3], y2) - np.maximum(t[1], y1)).astype(np.float64) + 1.0).astype(F32)
    touched = (iw > 0) & (ih > 0)
    inter = (iw * ih).astype(F32)
    ta = ((np.float64(t[2] - t[0]) + 1.0) * (np.float64(t[3] - t[1]) + 1.0))
    ua = ((ta + area.astype(np.float64)) - inter.astype(np.float64)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ov = (inter / ua).astype(F32)
        w = np.exp((-(ov * ov) / F32(sigma)).astype(F32).astype(np.float64)).astype(F32)
    ns = np.where(touched, (w * s).astype(F32), s)
    return ns, touched & (ns < F32(threshold))


def deferred_joint_form(rows, sigma=0.5, threshold=0.001):
    """Gaussian soft-NMS of (n, 39) rows as the device merge computes it.  Returns (the whole resulting
    array, the kept count, whether a row moved into a hole was itself discarded in the same step).
    ``rows`` is only read: it plays the kernel's global input."""
    n = rows.shape[0]
    box, sc = rows[:, :4].copy(), rows[:, 4].copy()      # the LDS copy
    jsrc = np.arange(n)
    N, chained = n, False
    for i in range(n):
        if i >= N:
            break
        live = sc[i:N]
        m = i + int(np.flatnonzero(live == live.max())[0])   # the first maximum
        box[[i, m]], sc[[i, m]], jsrc[[i, m]] = box[[m, i]], sc[[m, i]], jsrc[[m, i]]
        ns, disc = _decay(box, sc, i, N, sigma, threshold)
        ns = np.concatenate([np.zeros(i + 1, F32), ns])      # indexed by start-of-step position
        disc = np.concatenate([np.zeros(i + 1, bool), disc])
        orig = np.arange(N)
        pos = i + 1
        while pos < N:
            hits = np.flatnonzero(disc[pos:N])
            if not len(hits):
                break
            p = pos + int(hits[0])
            while True:
                if p == N - 1:
                    sc[p] = ns[orig[p]]
                    N = p
                    break
                last = N - 1
                box[p], sc[p] = box[last], sc[last]          # columns 0..4 copied
                jsrc[p], jsrc[last] = jsrc[last], jsrc[p]     # columns 5.. exchanged
                orig[p] = last
                N = last
                if not disc[last]:
                    break
                chained = True
            pos = p + 1
        q = np.arange(i + 1, N)
        sc[q] = ns[orig[q]]
    out = np.concatenate([box, sc[:, None], rows[jsrc, 5:]], axis=1)     # the gather
    return np.ascontiguousarray(out, F32), N, chained


def clustered(rng, n, stride=39):
    """Boxes in a few dense clusters (the discard path runs often), scores with repeats."""
    centres = rng.uniform(0, 200, (max(1, n // 6), 2))
    c = centres[rng.randint(0, len(centres), n)]
    wh = rng.uniform(4, 40, (n, 2))
    jitter = rng.normal(0, rng.choice([0.5, 3.0, 15.0]), (n, 2))
    xy1 = c + jitter - wh / 2
    rows = np.zeros((n, stride), F32)
    rows[:, 0:2] = xy1
    rows[:, 2:4] = xy1 + wh
    levels = rng.choice([4, 20, 1000])
    rows[:, 4] = (rng.randint(1, levels + 1, n) / levels) * rng.uniform(0.0005, 1.0)
    rows[:, 5:] = rng.uniform(-5, 300, (n, stride - 5))
    return rows


def test_deferred_joint_form_equals_soft_nms_39():
    n_disc = n_chain = 0
    assert len(SEEDS) >= 1000
    for seed in SEEDS:
        rng = np.random.RandomState(seed)
        rows = clustered(rng, SIZES[seed % len(SIZES)])
        want = rows.copy()
        kept = len(soft_nms_39(want, Nt=0.5, method=2))
        got, n_kept, chained = deferred_joint_form(rows)
        assert n_kept == kept, seed
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), seed
        n_disc += len(rows) - kept
        n_chain += int(chained)
    assert n_disc > 100          # the discard walk ran many times
    assert n_chain >= 20         # ... and a row moved into a hole was discarded there, in many arrays


def test_symbols_are_exported_declared_and_bound():
    lib = native.lib()
    header = open(os.path.join(ROOT, "include", "centernet_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("cn_multi_pose_post_process_f32", 8), ("cn_multi_pose_merge_f32", 7)):
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    assert lib.cn_version() == 313


def test_argument_checks_run_without_a_device():
    lib = native.lib()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data        # never dereferenced: every call below returns before a launch
    CN_ERR_SHAPE, CN_ERR_UNSUPPORTED, CN_ERR_NULL = -1, -2, -5
    post, merge = lib.cn_multi_pose_post_process_f32, lib.cn_multi_pose_merge_f32
    assert post(None, 1, 1, p, 0, 1.0, p, None) == CN_ERR_NULL
    assert post(p, 1, 1, None, 0, 1.0, p, None) == CN_ERR_NULL
    assert post(p, 1, 1, p, 0, 1.0, None, None) == CN_ERR_NULL
    assert post(p, 0, 1, p, 0, 1.0, p, None) == CN_ERR_SHAPE
    assert post(p, 1, 0, p, 0, 1.0, p, None) == CN_ERR_SHAPE
    assert post(p, 1, 1, p, 0, 0.0, p, None) == CN_ERR_SHAPE
    assert post(p, 1, 1, p, 0, -1.0, p, None) == CN_ERR_SHAPE
    assert post(p, 1, 129, p, 0, 1.0, p, None) == CN_ERR_UNSUPPORTED
    assert merge(None, 1, 1, 1, 0, p, None) == CN_ERR_NULL
    assert merge(p, 1, 1, 1, 0, None, None) == CN_ERR_NULL
    assert merge(p, 0, 1, 1, 0, p, None) == CN_ERR_SHAPE
    assert merge(p, 1, 0, 1, 0, p, None) == CN_ERR_SHAPE
    assert merge(p, 1, 1, 0, 0, p, None) == CN_ERR_SHAPE
    assert merge(p, 1, 1, 2049, 0, p, None) == CN_ERR_SHAPE          # S * K = 2049
    assert merge(p, 3, 1, 683, 1, p, None) == CN_ERR_SHAPE           # 3 x 683 = 2049
    assert native.MERGE_MAX_ROWS == 2048
    assert lib.cn_status_string(CN_ERR_NULL) != lib.cn_status_string(CN_ERR_SHAPE)


def _stub(scales, nms):
    from centernet_amd.detectors.multi_pose import MultiPoseDetector
    det = object.__new__(MultiPoseDetector)
    det.num_classes, det.max_per_image, det.scales = 1, 100, scales
    det.opt = types.SimpleNamespace(num_classes=1, nms=nms, test_scales=scales)
    return det


def test_arrays_keyword_on_the_host_tail():
    """run_frames(arrays=True) / run_frames_stream(arrays=True): the pose host tail returns {1: (n, 39)
    float32 array} with the bits of the list form; the default is the list form."""
    from centernet_amd.detectors.base_detector import BaseDetector
    from centernet_amd.frame_pipe import FramePipe
    from centernet_amd.detectors.ctdet import CtdetDetector
    for fn in (BaseDetector.run_frames, BaseDetector.run_frames_stream, FramePipe.collect):
        assert inspect.signature(fn).parameters["arrays"].default is False, fn
    assert object.__new__(CtdetDetector)._arrays_kw(True) == {}       # ctdet returns arrays as it is
    rng = np.random.RandomState(5)
    meta = {'c': np.array([250., 187.5], np.float32), 's': 500.0, 'out_height': 128, 'out_width': 128}
    n, K = 3, 40
    for scales, nms in (([1.0], False), ([1.0], True), ([1.0, 0.75], False)):
        det = _stub(scales, nms)
        kw = det._arrays_kw(True)
        assert kw == {"arrays": True} and det._arrays_kw(False) == {}
        per_scale = []
        for sc in scales:
            d = np.zeros((n, K, 40), F32)
            d[:, :, :4] = rng.uniform(20, 60, (n, K, 4))       # overlapping boxes: soft-NMS has work
            d[:, :, 2:4] += 30
            d[:, :, 4] = rng.uniform(0, 1, (n, K))
            d[:, :, 5:39] = rng.uniform(-4, 132, (n, K, 34))
            per_scale.append((d, [meta] * n, sc))
        if len(scales) == 1 and not nms:
            lists, arrs = det.results_batch(*per_scale[0]), det.results_batch(*per_scale[0], **kw)
        else:
            lists, arrs = det._results_merged(per_scale), det._results_merged(per_scale, **kw)
        assert len(lists) == len(arrs) == n
        for a, b in zip(lists, arrs):
            assert list(a) == list(b) == [1]
            assert isinstance(a[1], list) and isinstance(a[1][0], list) and isinstance(a[1][0][0], float)
            assert isinstance(b[1], np.ndarray) and b[1].dtype == np.float32
            assert b[1].shape == (len(scales) * K, 39)
            assert np.array_equal(np.array(a[1], np.float32).view(np.uint32), b[1].view(np.uint32))
