"""run_frames / run_frames_stream with flip-test, several test scales and --nms: the batched flip average
(cn_flip_average_f32_batch), the device scale merge (cn_ctdet_merge_f32) and the multi-scale frame pipe,
each against what run(frame) / merge_outputs / the CPU oracle compute."""
import contextlib
import ctypes
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from oracle import net_oracle, post_oracle, pre_oracle

pytestmark = pytest.mark.gpu

NC = 80
COCO_FLIP_IDX = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


def _detector(task, args):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task] + list(args))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


# ------------------------------------------------------------------------------------------------
# 1. the merge kernel against merge_outputs of the oracle, bit for bit
# ------------------------------------------------------------------------------------------------
def _tail_output(rng, S, B, K, classes, clusters, levels):
    """Rows / bounds as cn_ctdet_post_process_f32 leaves them for every scale: per image up to K rows
    grouped by class, boxes in a few dense clusters, scores on `levels` steps (ties)."""
    rows = np.full((S, B, K, 5), np.nan, np.float32)
    bounds = np.zeros((S, B, NC + 1), np.int32)
    per_scale = [[None] * B for _ in range(S)]
    centres = rng.uniform(0, 300, (clusters, 2))
    for s in range(S):
        for b in range(B):
            n = int(rng.randint(K - K // 4, K + 1))
            cls = np.sort(rng.choice(classes, n))
            c = centres[rng.randint(0, clusters, n)] + rng.normal(0, rng.choice([0.7, 4.0]), (n, 2))
            wh = rng.uniform(8, 50, (n, 2))
            r = np.zeros((n, 5), np.float32)
            r[:, 0:2] = c - wh / 2
            r[:, 2:4] = c + wh / 2
            r[:, 4] = rng.randint(1, levels + 1, n) / np.float32(levels) * np.float32(0.9)
            rows[s, b, :n] = r
            bounds[s, b] = np.searchsorted(cls, np.arange(NC + 1), side="left")
            per_scale[s][b] = {j + 1: r[bounds[s, b, j]:bounds[s, b, j + 1]].copy() for j in range(NC)}
    return rows, bounds, per_scale


def _merge_call(rows, bounds, nms, max_per_image=100):
    S, B, K, _ = rows.shape
    out_rows = torch.zeros((B, S * K, 5), dtype=torch.float32, device="cuda")
    out_bounds = torch.zeros((B, NC + 1), dtype=torch.int32, device="cuda")
    r, bd = torch.from_numpy(rows).cuda(), torch.from_numpy(bounds).cuda()
    rc = native.lib().cn_ctdet_merge_f32(native.ptr(r), native.ptr(bd), S, B, K, NC, int(nms), max_per_image,
                                         native.ptr(out_rows), native.ptr(out_bounds), native.stream_ptr())
    torch.cuda.synchronize()
    return rc, out_rows.cpu().numpy(), out_bounds.cpu().numpy()


CASES = [  # (S, K, nms, classes, clusters, score levels)
    (1, 100, True, np.arange(NC), 6, 1000),
    (2, 100, False, np.arange(5), 3, 1000),          # dense: the discard walk runs again and again
    (3, 100, False, np.arange(NC), 10, 7),           # ties at the argmax and at the top-100 threshold
    (5, 100, False, np.array([0, 3, 3, 3, 79]), 4, 20),   # empty classes next to long segments
    (5, 128, True, np.arange(0, NC, 7), 40, 3),
    (2, 1024, False, np.arange(NC), 30, 50),         # S * K at the cap
    (4, 3, False, np.arange(NC), 2, 5),              # one-row segments
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_merge_kernel_equals_oracle_merge(dev, case):
    S, K, nms, classes, clusters, levels = CASES[case]
    rng = np.random.RandomState(100 + case)
    B = 3
    rows, bounds, per_scale = _tail_output(rng, S, B, K, classes, clusters, levels)
    rc, out_rows, out_bounds = _merge_call(rows, bounds, nms)
    assert rc == native.CN_OK
    for b in range(B):
        want = post_oracle.ctdet_merge_outputs([per_scale[s][b] for s in range(S)], NC, S, nms=nms)
        bd = out_bounds[b]
        assert bd[0] == 0 and bd[NC] == sum(len(v) for v in want.values())
        for j in range(NC):
            got = out_rows[b, bd[j]:bd[j + 1]]
            assert got.shape == want[j + 1].shape, (b, j)
            assert np.array_equal(got.view(np.uint32), want[j + 1].view(np.uint32)), (b, j)


def test_merge_kernel_refuses_rows_above_the_cap(dev):
    rows = np.zeros((3, 1, 700, 5), np.float32)
    bounds = np.zeros((3, 1, NC + 1), np.int32)
    rc, _, _ = _merge_call(rows, bounds, False)
    assert rc == -1                                   # CN_ERR_SHAPE
    assert native.MERGE_MAX_ROWS == 2048


# ------------------------------------------------------------------------------------------------
# 2. the batched flip average == flip_average per pair
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["hm", "hps", "hm_hp"])
def test_flip_average_batch_equals_per_pair(dev, what):
    from centernet_amd.utils import flip_average, flip_average_batch
    P, H, W = 3, 24, 20
    C, kw = {"hm": (NC, dict(sigmoid=True)), "hps": (34, dict(flip_idx=COCO_FLIP_IDX, offsets=True)),
             "hm_hp": (17, dict(flip_idx=COCO_FLIP_IDX, sigmoid=True))}[what]
    g = torch.Generator().manual_seed(11)
    x = (torch.randn((2 * P, C, H, W), generator=g) * 4).to(dev)
    xb = x.clone()
    got = flip_average_batch(xb, **kw)
    assert tuple(got.shape) == (P, C, H, W)
    for p in range(P):
        pair = x[2 * p:2 * p + 2].clone()
        want = flip_average(pair, **kw)
        assert torch.equal(got[p:p + 1].view(torch.int32), want.view(torch.int32)), p
        if kw.get("sigmoid"):                       # both images hold the logistic afterwards, as sigmoid_()
            assert torch.equal(xb[2 * p:2 * p + 2], pair)
    first = flip_average_batch(x, first=True)
    assert torch.equal(first, x[0::2])


# ------------------------------------------------------------------------------------------------
# 3 - 7. the frame pipe
# ------------------------------------------------------------------------------------------------
def _frames(seed, n, h=100, w=140):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


def _paired(res, ref, box_tol=4e-3, score_tol=2e-4):
    """Rows of `res` that have a row of the same class in `ref` within tolerance, and the row counts."""
    matched = 0
    for j in ref:
        a, b = np.asarray(res[j], np.float64), np.asarray(ref[j], np.float64)
        if len(a) and len(b):
            d_box = np.abs(a[:, None, :4] - b[None, :, :4]).max(axis=2)
            d_sc = np.abs(a[:, None, 4] - b[None, :, 4])
            matched += int(((d_box < box_tol) & (d_sc < score_tol)).any(axis=1).sum())
    return matched, sum(len(v) for v in res.values()), sum(len(v) for v in ref.values())


def _assert_close_multi(res, ref):
    m, n_res, n_ref = _paired(res, ref)
    assert abs(n_res - n_ref) <= 2, (n_res, n_ref)
    assert m >= 0.95 * n_ref, (m, n_ref)


def test_ctdet_run_frames_flip_equals_run(dev):
    det, opt = _detector("ctdet", ["--arch", "resdcn_18", "--input_h", "128", "--input_w", "128", "--flip_test"])
    frames = _frames(21, 3)
    batched = det.run_frames(frames)
    for f, rb in zip(frames, batched):
        rs = det.run(f)["results"]
        for j in range(1, NC + 1):
            assert rb[j].shape == rs[j].shape
            if len(rb[j]):
                assert np.abs(rb[j] - rs[j]).max() < 2e-3


@pytest.mark.parametrize("args", [["--test_scales", "1,0.75", "--keep_res"],
                                  ["--test_scales", "0.5,1,1.5", "--flip_test", "--keep_res"]])
def test_ctdet_run_frames_multi_scale_equals_run(dev, args):
    det, opt = _detector("ctdet", ["--arch", "resdcn_18"] + args)
    frames = _frames(22, 3)
    pipe = det._pipe_for(frames, 1)
    assert pipe.tail is not None and pipe.merge       # served by the device merge
    batched = det.run_frames(frames)
    for f, rb in zip(frames, batched):
        _assert_close_multi(rb, det.run(f)["results"])


@pytest.mark.parametrize("args", [["--test_scales", "1,0.75", "--flip_test", "--keep_res"],
                                  ["--nms", "--input_h", "128", "--input_w", "128"]])
def test_device_merge_equals_host_merge_on_the_same_detections(dev, args):
    """The pipe's device result == the host tail + merge_outputs on the same per-scale raw detections:
    the merge isolated from the network's last bits."""
    det, opt = _detector("ctdet", ["--arch", "resdcn_18"] + args)
    frames = _frames(23, 4)
    pipe = det._pipe_for(frames, 1)
    assert pipe.tail is not None and pipe.merge
    pipe.submit(0, frames)
    got = pipe.collect(0, frames)
    per_scale = [(det._run_scale(lv.batch, pipe.flip).detach().cpu().numpy(), [lv.meta] * 4, lv.scale)
                 for lv in pipe.levels]
    want = det._results_merged(per_scale)
    for a, b in zip(got, want):
        for j in range(1, NC + 1):
            assert a[j].shape == b[j].shape and np.array_equal(a[j].view(np.int32), b[j].view(np.int32)), j


def test_run_frames_stream_flip_multi_scale_equals_run_frames(dev):
    det, opt = _detector("ctdet", ["--arch", "resdcn_18", "--flip_test", "--test_scales", "1,0.75", "--keep_res"])
    batches = [_frames(30 + i, 3) for i in range(4)]
    alone = [det.run_frames(b) for b in batches]
    streamed = list(det.run_frames_stream(iter(batches), depth=2))
    assert len(streamed) == len(batches)
    for ra, rs in zip(alone, streamed):
        assert len(ra) == len(rs) == 3
        for a, b in zip(ra, rs):
            for j in range(1, NC + 1):
                assert a[j].dtype == np.float32 and np.array_equal(a[j], b[j]), j


def test_multi_pose_run_frames_flip_multi_scale_equals_run(dev):
    det, opt = _detector("multi_pose", ["--arch", "dla_34", "--input_h", "128", "--input_w", "128",
                                        "--flip_test", "--test_scales", "1,0.75"])
    frames = _frames(24, 3, 96, 120)
    batched = det.run_frames(frames)
    assert len(batched) == 3
    for f, rb in zip(frames, batched):
        rs = det.run(f)["results"]
        a, b = np.array(rb[1], np.float32), np.array(rs[1], np.float32)
        assert a.shape == b.shape == (2 * opt.K, 39)
        # soft-NMS may order near-equal rows differently: pair every row with its nearest
        d = np.abs(a[:, None, :].astype(np.float64) - b[None, :, :]).max(axis=2)
        near = d.argmin(axis=1)
        ok = (np.abs(a[:, 4] - b[near, 4]) < 1e-4) & (d.min(axis=1) < 5e-3)
        assert ok.mean() >= 0.95, ok.mean()


def test_run_frames_flip_multi_scale_matches_oracle_pipeline(dev):
    det, opt = _detector("ctdet", ["--arch", "resdcn_18", "--flip_test", "--test_scales", "1,0.75", "--keep_res"])
    image = _frames(25, 1, 120, 152)[0]
    res = det.run_frames([image])[0]
    per_scale = []
    for scale in opt.test_scales:
        images, meta = pre_oracle.pre_process(image, scale, opt.mean, opt.std, fix_res=opt.fix_res,
                                              input_h=opt.input_h, input_w=opt.input_w, pad=opt.pad,
                                              flip_test=True, down_ratio=opt.down_ratio)
        _, dets = net_oracle.ctdet_process("resdcn_18", det.model.state_dict(), torch.from_numpy(images),
                                           list(opt.heads), K=opt.K, flip_test=True)
        per_scale.append(post_oracle.ctdet_post_process_scale(dets, meta, opt.num_classes, scale))
    ref = post_oracle.ctdet_merge_outputs(per_scale, opt.num_classes, len(opt.test_scales))
    m, n_res, n_ref = _paired(res, ref)
    assert abs(n_res - n_ref) <= 2, (n_res, n_ref)
    assert m >= 0.9 * n_ref, (m, n_ref)
