"""The multi_pose device tail of run_frames / run_frames_stream: cn_multi_pose_post_process_f32 against the
CPU oracle's multi_pose_results, cn_multi_pose_merge_f32 against np.concatenate + the reference soft-NMS on
the 39-column array (both bit for bit, through the C ABI), and the frame pipe built on them against the host
tail on the same raw detections and against run(frame)."""
import contextlib
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from oracle import post_oracle, ref as oracle_ref
from test_pose_tail_host import deferred_joint_form

pytestmark = pytest.mark.gpu

ROW = 39


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _detector(args):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["multi_pose", "--arch", "dla_34"] + list(args))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


def _frames(seed, n, h=96, w=120):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


# ------------------------------------------------------------------------------------------------
# 4. the post-process kernel against the oracle, bit for bit
# ------------------------------------------------------------------------------------------------
def _meta(h, w, keep_res, rng=None):
    """Meta of a (h, w) frame as BaseDetector builds it (fixed 512 x 512 input, or --keep_res), optionally
    with the centre moved a little (per-image matrices that differ)."""
    if keep_res:
        inp_h, inp_w = (h | 31) + 1, (w | 31) + 1
        c = np.array([w // 2, h // 2], np.float32)
        s = np.array([inp_w, inp_h], np.float32)
    else:
        inp_h, inp_w = 512, 512
        c = np.array([w / 2., h / 2.], np.float32)
        s = max(h, w) * 1.0
    if rng is not None:
        c = (c + rng.uniform(-20, 20, 2)).astype(np.float32)
        s = s * np.float32(rng.uniform(0.7, 1.4))
    return {'c': c, 's': s, 'out_height': inp_h // 4, 'out_width': inp_w // 4}


def _raw_dets(rng, B, K, meta):
    """multi_pose_decode-like rows; a part of the coordinates outside the grid and negative."""
    d = np.zeros((B, K, 40), np.float32)
    w, h = meta['out_width'], meta['out_height']
    pts = rng.uniform(-0.4, 1.4, (B, K, 19, 2)) * np.array([w, h])
    d[:, :, 0:4] = pts[:, :, :2].reshape(B, K, 4)
    d[:, :, 5:39] = pts[:, :, 2:].reshape(B, K, 34)
    d[:, :, 4] = np.sort(rng.uniform(0, 1, (B, K)), axis=1)[:, ::-1]
    return d


POST_CASES = [  # (h, w, keep_res, scale, B, K, per_image)
    (512, 512, False, 1.0, 1, 100, False),
    (512, 512, False, 0.5, 3, 100, False),
    (375, 500, False, 0.75, 3, 128, False),         # non-square, fixed input
    (375, 500, True, 1.25, 3, 100, False),          # non-square, --keep_res: s is an (inp_w, inp_h) pair
    (96, 120, True, 1.0, 32, 100, False),
    (480, 640, False, 0.75, 32, 128, False),
    (333, 517, True, 0.5, 1, 1, False),
    (512, 512, False, 1.25, 3, 1, False),
    (375, 500, False, 1.0, 3, 100, True),           # B different matrices
    (375, 500, True, 0.75, 32, 128, True),
    (600, 400, True, 1.25, 3, 128, True),
]


@pytest.mark.parametrize("case", range(len(POST_CASES)))
def test_post_process_kernel_equals_oracle(dev, case):
    h, w, keep_res, scale, B, K, per_image = POST_CASES[case]
    rng = np.random.RandomState(300 + case)
    metas = [_meta(int(h * scale), int(w * scale), keep_res, rng if per_image else None) for _ in range(B)]
    if not per_image:
        metas = [metas[0]] * B
    dets = _raw_dets(rng, B, K, metas[0])
    mats = np.stack([post_oracle.get_affine_transform(m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1)
                     for m in (metas if per_image else metas[:1])]).astype(np.float64)
    if per_image:
        assert len({m.tobytes() for m in mats}) == B
    d, t = torch.from_numpy(dets).to(dev), torch.from_numpy(np.ascontiguousarray(mats.reshape(-1))).to(dev)
    rows = torch.full((B, K, ROW), float("nan"), device=dev)
    rc = native.lib().cn_multi_pose_post_process_f32(native.ptr(d), B, K, native.ptr(t), int(per_image),
                                                     float(scale), native.ptr(rows), native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == native.CN_OK
    got = rows.cpu().numpy()
    assert torch.equal(d.cpu(), torch.from_numpy(dets))          # the input is only read
    for b in range(B):
        want = np.array(post_oracle.multi_pose_results(dets[b:b + 1], metas[b], scale)[1], np.float32)
        assert want.shape == (K, ROW)
        bad = np.argwhere(_bits(got[b]) != _bits(want))
        assert not len(bad), (b, bad[:4], [(got[b][tuple(i)], want[tuple(i)]) for i in bad[:4]])


# ------------------------------------------------------------------------------------------------
# 5. the merge kernel against np.concatenate + the reference soft-NMS, the whole array bit for bit
# ------------------------------------------------------------------------------------------------
def _ref_soft_nms_39(x):
    """The reference's own cython build where it was built, else the oracle's statement-by-statement
    restatement (never the product's soft_nms_39).  In place; returns the kept count."""
    if oracle_ref.available():
        return len(oracle_ref.soft_nms_39(x, Nt=0.5, method=2))
    return len(post_oracle.soft_nms(x, Nt=0.5, method=2))


def _scale_rows(rng, S, B, K, clusters, levels):
    """(S, B, K, 39) rows as the post-process kernel leaves them: boxes in a few dense clusters, scores on
    `levels` steps (ties), joints anywhere."""
    centres = rng.uniform(0, 300, (clusters, 2))
    c = centres[rng.randint(0, clusters, (S, B, K))] + rng.normal(0, rng.choice([0.7, 4.0]), (S, B, K, 2))
    wh = rng.uniform(8, 50, (S, B, K, 2))
    rows = np.zeros((S, B, K, ROW), np.float32)
    rows[..., 0:2] = c - wh / 2
    rows[..., 2:4] = c + wh / 2
    rows[..., 4] = rng.randint(1, levels + 1, (S, B, K)) / np.float32(levels) * np.float32(0.9)
    rows[..., 5:] = rng.uniform(-50, 600, (S, B, K, 34))
    return rows


def _merge_call(rows, nms):
    S, B, K, _ = rows.shape
    out = torch.full((B, S * K, ROW), float("nan"), dtype=torch.float32, device="cuda")
    r = torch.from_numpy(rows).cuda()
    rc = native.lib().cn_multi_pose_merge_f32(native.ptr(r), S, B, K, int(nms), native.ptr(out),
                                              native.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


MERGE_CASES = [  # (S, K, nms, clusters, score levels)
    (1, 100, True, 6, 1000),
    (2, 100, False, 3, 1000),           # dense: the discard walk runs again and again
    (3, 100, False, 10, 7),             # ties at the argmax
    (5, 100, False, 4, 20),             # flip + 5 scales
    (5, 128, True, 40, 3),
    (2, 1024, False, 30, 50),           # S * K at the cap
    (4, 3, False, 2, 5),
    (1, 3, True, 1, 5),                 # K = 3
]


def _merge_batch(S, K):
    """Images per case; the oracle's restatement is O(n^2) Python, so one image at the cap without the cython."""
    if S * K < 1024:
        return 6
    return 3 if oracle_ref.available() else 1


def test_merge_kernel_equals_reference_merge(dev):
    n_disc = n_chain = 0
    for case, (S, K, nms, clusters, levels) in enumerate(MERGE_CASES):
        rng = np.random.RandomState(400 + case)
        B = _merge_batch(S, K)
        rows = _scale_rows(rng, S, B, K, clusters, levels)
        rc, out = _merge_call(rows, nms)
        assert rc == native.CN_OK
        for b in range(B):
            cat = np.concatenate([rows[s, b] for s in range(S)], axis=0).astype(np.float32)
            want = cat.copy()
            kept = _ref_soft_nms_39(want) if S > 1 or nms else S * K
            n_disc += S * K - kept
            form, form_kept, chained = deferred_joint_form(cat)
            assert form_kept == kept and np.array_equal(_bits(form), _bits(want)), (case, b)
            n_chain += int(chained)        # (the form equals the reference run, so its walk is that run's)
            bad = np.argwhere(_bits(out[b]) != _bits(want))
            assert not len(bad), (case, b, kept, bad[:4],
                                  [(out[b][tuple(i)], want[tuple(i)]) for i in bad[:4]])
    assert n_disc > 100
    assert n_chain >= 20


def test_merge_kernel_single_scale_without_nms_is_a_copy(dev):
    rows = _scale_rows(np.random.RandomState(420), 1, 3, 100, 3, 7)
    rc, out = _merge_call(rows, False)
    assert rc == native.CN_OK
    assert np.array_equal(_bits(out), _bits(rows[0]))


def test_merge_kernel_refuses_rows_above_the_cap(dev):
    rc, _ = _merge_call(np.zeros((3, 1, 700, ROW), np.float32), False)
    assert rc == -1                                   # CN_ERR_SHAPE
    rc, _ = _merge_call(np.zeros((1, 1, 2049, ROW), np.float32), True)
    assert rc == -1


def test_merge_kernel_repeats_bit_for_bit_beside_a_busy_stream(dev):
    """Two launches of the flip + 5 scales shape, a second stream kept busy meanwhile: equal bits."""
    rows = _scale_rows(np.random.RandomState(430), 5, 8, 100, 4, 20)
    side = torch.cuda.Stream()
    a = torch.randn((2048, 2048), device=dev)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a) * 0.5
    rc1, out1 = _merge_call(rows, False)
    rc2, out2 = _merge_call(rows, False)
    side.synchronize()
    assert rc1 == rc2 == native.CN_OK
    assert np.array_equal(_bits(out1), _bits(out2))


# ------------------------------------------------------------------------------------------------
# 6 - 9. the frame pipe
# ------------------------------------------------------------------------------------------------
PIPE_ARGS = [["--input_h", "128", "--input_w", "128"],
             ["--nms", "--input_h", "128", "--input_w", "128"],
             ["--flip_test", "--test_scales", "1,0.75", "--keep_res"]]


@pytest.mark.parametrize("args", PIPE_ARGS)
def test_device_tail_equals_host_tail_on_the_same_detections(dev, args):
    """The pipe's device result == the host tail (results_batch / post_process + merge_outputs) on the same
    per-scale raw detections: the tail isolated from the network's last bits.  Lists by default, arrays on
    request, the same bits."""
    det, opt = _detector(args)
    frames = _frames(23, 4)
    pipe = det._pipe_for(frames, 1)
    assert pipe.tail is not None
    assert pipe.merge == ("--nms" in args or "--test_scales" in args)
    S = len(pipe.levels)
    pipe.submit(0, frames)
    got = pipe.collect(0, frames)
    got_arrays = pipe.collect(0, frames, arrays=True)           # (the slot's buffers hold the batch still)
    per_scale = [(det._run_scale(lv.batch, pipe.flip).detach().cpu().numpy(), [lv.meta] * 4, lv.scale)
                 for lv in pipe.levels]
    want = det._results_merged(per_scale) if pipe.merge else det.results_batch(*per_scale[0])
    assert len(got) == len(got_arrays) == len(want) == 4
    for a, arr, b in zip(got, got_arrays, want):
        assert list(a) == list(arr) == [1]
        assert isinstance(a[1], list) and len(a[1]) == S * opt.K
        assert all(isinstance(r, list) and len(r) == ROW and isinstance(r[0], float) for r in a[1])
        assert np.array_equal(_bits(np.array(a[1], np.float32)), _bits(np.array(b[1], np.float32)))
        assert isinstance(arr[1], np.ndarray) and arr[1].dtype == np.float32 and arr[1].shape == (S * opt.K, ROW)
        assert np.array_equal(_bits(arr[1]), _bits(np.array(a[1], np.float32)))
    pinned = pipe.tail.host('rows', 0).numpy()
    assert not any(np.shares_memory(arr[1], pinned) for arr in got_arrays)      # a copy, not a view
    assert det.run_frames(frames, arrays=True)[0][1].shape == (S * opt.K, ROW)


def test_run_frames_stream_equals_run_frames(dev):
    det, opt = _detector(["--flip_test", "--test_scales", "1,0.75", "--keep_res"])
    batches = [_frames(30 + i, 3) for i in range(4)]
    assert det._pipe_for(batches[0], 2).tail is not None
    alone = [det.run_frames(b) for b in batches]
    streamed = list(det.run_frames_stream(iter(batches), depth=2))
    arrays = list(det.run_frames_stream(iter(batches), depth=2, arrays=True))
    assert len(streamed) == len(arrays) == len(batches)
    for ra, rs, rr in zip(alone, streamed, arrays):
        assert len(ra) == len(rs) == len(rr) == 3
        for a, b, c in zip(ra, rs, rr):
            assert isinstance(b[1], list) and a[1] == b[1]               # exactly
            assert np.array_equal(_bits(c[1]), _bits(np.array(a[1], np.float32)))


def _assert_rows_paired(a, b):
    """The bars of the existing pose tests (test_gpu_frames_tta): soft-NMS / near-equal scores may order rows
    differently, so every row is paired with its nearest; scores 1e-4, pixels 5e-3, 95 % of the rows."""
    assert a.shape == b.shape
    d = np.abs(a[:, None, :].astype(np.float64) - b[None, :, :]).max(axis=2)
    near = d.argmin(axis=1)
    ok = (np.abs(a[:, 4] - b[near, 4]) < 1e-4) & (d.min(axis=1) < 5e-3)
    assert ok.mean() >= 0.95, ok.mean()


def test_more_rows_than_the_kernels_take_fall_back_to_the_host_tail(dev):
    """K > 128: no device tail.  cn_multi_pose_decode_f32 itself takes K <= 128, so at --K 130 there are no
    detections to compare on either surface: run_frames fails as run(frame) does, loudly, in the decode.
    The host tail behind a pipe without a device tail is compared where it can run: 17 test scales of
    K = 128, S * K = 2176 rows above the merge kernel's 2048."""
    det, opt = _detector(["--K", "130", "--input_h", "128", "--input_w", "128"])
    frames = _frames(26, 3)
    assert det._pipe_for(frames, 1).tail is None
    for call in (lambda: det.run_frames(frames), lambda: det.run(frames[0])):
        with pytest.raises(native.NativeError, match="cn_multi_pose_decode_f32"):
            call()
    torch.cuda.synchronize()
    scales = ",".join("%.2f" % (0.5 + 0.05 * i) for i in range(17))
    det, opt = _detector(["--K", "128", "--input_h", "128", "--input_w", "128", "--test_scales", scales])
    pipe = det._pipe_for(frames, 1)
    assert pipe.merge and pipe.tail is None and 17 * 128 > native.MERGE_MAX_ROWS
    batched = det.run_frames(frames)
    as_arrays = det.run_frames(frames, arrays=True)
    for f, rb, ra in zip(frames, batched, as_arrays):
        a, b = np.array(rb[1], np.float32), np.array(det.run(f)["results"][1], np.float32)
        assert a.shape == (17 * 128, ROW)
        _assert_rows_paired(a, b)
        assert isinstance(rb[1], list) and ra[1].dtype == np.float32 and np.array_equal(_bits(ra[1]), _bits(a))


def test_run_frames_single_scale_equals_run(dev):
    det, opt = _detector(["--input_h", "128", "--input_w", "128"])
    frames = _frames(27, 3)
    assert det._pipe_for(frames, 1).tail is not None
    for f, rb in zip(frames, det.run_frames(frames)):
        a, b = np.array(rb[1], np.float32), np.array(det.run(f)["results"][1], np.float32)
        assert a.shape == b.shape == (opt.K, ROW)
        assert np.abs(a[:, 4] - b[:, 4]).max() < 1e-4          # scores (test_gpu_detector's bars)
        assert np.abs(a - b).max() < 5e-3                      # pixels


def test_run_frames_flip_two_scales_equals_run(dev):
    det, opt = _detector(["--input_h", "128", "--input_w", "128", "--flip_test", "--test_scales", "1,0.75"])
    frames = _frames(28, 3)
    pipe = det._pipe_for(frames, 1)
    assert pipe.tail is not None and pipe.merge
    for f, rb in zip(frames, det.run_frames(frames)):
        a, b = np.array(rb[1], np.float32), np.array(det.run(f)["results"][1], np.float32)
        assert a.shape == (2 * opt.K, ROW)
        _assert_rows_paired(a, b)
