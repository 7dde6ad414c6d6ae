"""Host side of the ddd frame pipe: the normalisation table against the oracle's float32 chain, the vectorised
host tail ``post_process.ddd_results_batch`` against the oracle's statement-by-statement ``ddd_results`` +
``ddd_merge_outputs`` (bit for bit, angles included: both are NumPy), and the ``calibs`` argument of
``DddDetector.run_frames``.  ``ddd_rows`` builds the synthetic raw rows; tests/test_gpu_ddd_pipe.py uses the same."""
import types

import numpy as np
import pytest

from centernet_amd.detectors.ddd import DddDetector
from centernet_amd.post_process import ddd_norm_table, ddd_post_process, ddd_results_batch
from oracle import post_oracle, pre_oracle

KITTI = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
                  [0.0, 0.0, 1.0, 0.002745884]], np.float32)
DEFAULT = np.array([[707.0493, 0, 604.0814, 45.75831], [0, 707.0493, 180.5066, -0.3454157],
                    [0, 0, 1., 0.004981016]], np.float32)
OUT_W, OUT_H, NUM_CLASSES = 320, 96, 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ddd_meta(h=375, w=1242, calib=KITTI, keep_res=False):
    s = np.array([4 * OUT_W, 4 * OUT_H] if keep_res else [w, h], dtype=np.int32)
    return {'c': np.array([w / 2, h / 2], dtype=np.float32), 's': s, 'out_height': OUT_H, 'out_width': OUT_W,
            'calib': np.array(calib, dtype=np.float32)}


def calib_like(rng):
    """another camera: focal length, principal point and the translation column moved"""
    P = KITTI.copy()
    P[0, 0] = P[1, 1] = np.float32(rng.uniform(500, 1100))
    P[0, 2], P[1, 2] = rng.uniform(450, 750), rng.uniform(120, 240)
    P[:, 3] = rng.uniform(-60, 60, 3) * np.array([1, 0.05, 1e-4])
    return P.astype(np.float32)


def ddd_rows(rng, B, K, fill="mixed"):
    """(B, K, 18) rows as ddd_decode leaves them: scores descending; centres partly outside the grid; both
    orientation bins, the (sin, cos) pair in every quadrant; yaws that wrap at +-pi (alpha near the bin's
    far end and a viewing ray on the same side); class ids per ``fill``: 'mixed' = 0..2, 'empty' = class 1
    missing, 'stray' = some ids outside the range (and one that is no integer)."""
    d = np.zeros((B, K, 18), np.float32)
    d[:, :, 0] = rng.uniform(-0.3, 1.3, (B, K)) * OUT_W
    d[:, :, 1] = rng.uniform(-0.3, 1.3, (B, K)) * OUT_H
    d[:, :, 2] = np.sort(rng.uniform(0.02, 0.98, (B, K)), axis=1)[:, ::-1]
    d[:, :, 3:11] = rng.normal(0, 1, (B, K, 8))
    ang = rng.uniform(-np.pi, np.pi, (B, K, 2))                 # four quadrants for both bins
    edge = rng.uniform(0, 1, (B, K, 2)) < 0.3                   # ... and a share right at the far ends: wraps
    ang = np.where(edge, np.sign(ang) * (np.pi / 2 + rng.uniform(0, 0.4, (B, K, 2))), ang)
    mag = rng.uniform(0.2, 2.0, (B, K, 2))
    d[:, :, 5], d[:, :, 6] = mag[..., 0] * np.sin(ang[..., 0]), mag[..., 0] * np.cos(ang[..., 0])
    d[:, :, 9], d[:, :, 10] = mag[..., 1] * np.sin(ang[..., 1]), mag[..., 1] * np.cos(ang[..., 1])
    d[:, :, 11] = rng.uniform(2, 80, (B, K))
    d[:, :, 12:15] = rng.uniform(0.5, 4.5, (B, K, 3))
    d[:, :, 15] = rng.uniform(0, 0.4, (B, K)) * OUT_W
    d[:, :, 16] = rng.uniform(0, 0.6, (B, K)) * OUT_H
    cls = rng.randint(0, NUM_CLASSES, (B, K)).astype(np.float32)
    if fill == "empty":
        cls[cls == 1] = 2
    if fill == "stray":
        stray = rng.uniform(0, 1, (B, K)) < 0.2
        cls = np.where(stray, rng.choice([-1.0, 3.0, 7.0, 1.5], (B, K)), cls).astype(np.float32)
    d[:, :, 17] = cls
    return d


def oracle_results(dets_b, meta, peak_thresh):
    res = post_oracle.ddd_results(dets_b[None], meta, NUM_CLASSES, OUT_W, OUT_H)
    return post_oracle.ddd_merge_outputs([res], NUM_CLASSES, peak_thresh)


def _assert_same(got, want, where):
    assert sorted(got) == sorted(want) == [1, 2, 3], where
    for j in want:
        assert got[j].dtype == np.float32 and got[j].shape == want[j].shape, (where, j, got[j].shape, want[j].shape)
        assert np.array_equal(_bits(got[j]), _bits(want[j])), (where, j)


# ------------------------------------------------------------------------------------------------
def test_norm_table_equals_the_oracle_chain_for_every_level():
    rng = np.random.RandomState(3)
    for mean, std in (([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]), (rng.uniform(0.2, 0.7, 3), rng.uniform(0.1, 0.4, 3))):
        table = ddd_norm_table(mean, std)
        assert table.shape == (3, 256) and table.dtype == np.float32 and table.flags.c_contiguous
        image = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2).reshape(16, 16, 3)
        # a 16 x 16 frame onto a 16 x 16 input under --keep_res: the identity warp, every level once
        images, _ = pre_oracle.ddd_pre_process(image, mean, std, input_h=16, input_w=16, keep_res=True)
        assert np.array_equal(_bits(images[0].reshape(3, 256)), _bits(table))


CASES = [  # (B, K, fill, per-image matrices, peak_thresh, keep_res)
    (1, 100, "mixed", False, 0.2, False),
    (3, 100, "mixed", True, 0.5, False),
    (3, 40, "empty", True, 0.2, True),
    (4, 128, "stray", True, 0.35, False),
    (2, 1, "mixed", False, 0.2, False),
    (3, 100, "mixed", True, 0.99, False),        # every class fully cut
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_results_batch_equals_the_oracle_per_image(case):
    B, K, fill, per_image, thresh, keep_res = CASES[case]
    rng = np.random.RandomState(700 + case)
    dets = ddd_rows(rng, B, K, fill)
    metas = [ddd_meta(calib=calib_like(rng) if per_image else KITTI, keep_res=keep_res) for _ in range(B)]
    if per_image and B > 1:
        assert len({m['calib'].tobytes() for m in metas}) == B
    before = dets.copy()
    got = ddd_results_batch(dets, metas, NUM_CLASSES, thresh)
    assert np.array_equal(_bits(dets), _bits(before))
    shapes = set()
    for b in range(B):
        want = oracle_results(before[b], metas[b], thresh)
        _assert_same(got[b], want, (case, b))
        shapes |= {want[j].shape for j in want}
    if fill == "empty":
        assert (0,) in shapes
    if thresh > 0.98:
        assert shapes == {(0, 13)}


def test_results_batch_equals_the_product_loop_too():
    """... and ddd_post_process + merge_outputs, the path run() takes."""
    rng = np.random.RandomState(41)
    dets = ddd_rows(rng, 3, 100, "stray")
    metas = [ddd_meta(calib=calib_like(rng)) for _ in range(3)]
    opt = types.SimpleNamespace(num_classes=NUM_CLASSES, output_w=OUT_W, output_h=OUT_H, peak_thresh=0.3)
    det = types.SimpleNamespace(opt=opt, num_classes=NUM_CLASSES)
    got = ddd_results_batch(dets, metas, NUM_CLASSES, 0.3)
    for b in range(3):
        m = metas[b]
        loop = ddd_post_process(dets[b:b + 1].copy(), [m['c']], [m['s']], [m['calib']], opt)[0]
        _assert_same(got[b], DddDetector.merge_outputs(det, [loop]), b)


def test_the_rows_cover_what_they_claim():
    """both bins, four quadrants, wraps on both sides, centres outside the grid"""
    rng = np.random.RandomState(700)
    dets = ddd_rows(rng, 3, 100)
    first = dets[:, :, 4] > dets[:, :, 8]
    assert 0.2 < first.mean() < 0.8
    for s, c in ((5, 6), (9, 10)):
        quadrants = {(bool(a), bool(b)) for a, b in zip((dets[:, :, s] > 0).ravel(), (dets[:, :, c] > 0).ravel())}
        assert len(quadrants) == 4
    assert (dets[:, :, 0] < 0).any() and (dets[:, :, 0] > OUT_W).any() and (dets[:, :, 1] > OUT_H).any()
    meta = ddd_meta()
    res = post_oracle.ddd_results(dets[0][None], meta, NUM_CLASSES, OUT_W, OUT_H)
    rows = np.concatenate([res[j] for j in res])
    unwrapped = rows[:, 0].astype(np.float64) + np.arctan2(rows[:, 1] / 2 + rows[:, 3] / 2 - KITTI[0, 2], KITTI[0, 0])
    assert (unwrapped > np.pi).sum() >= 2 and (unwrapped < -np.pi).sum() >= 2
    assert np.all(np.abs(rows[:, 11]) <= np.float32(np.pi))


def test_results_batch_refuses_rows_without_wh():
    with pytest.raises(ValueError):
        ddd_results_batch(np.zeros((1, 4, 16), np.float32), [ddd_meta()], NUM_CLASSES, 0.2)


# ------------------------------------------------------------------------------------------------
def _host_detector():
    """A DddDetector without its network (the constructor needs the device): host methods only."""
    from centernet_amd.opts import opts
    opt = opts().init(["ddd"])
    det = DddDetector.__new__(DddDetector)
    det.opt, det.num_classes, det.scales = opt, opt.num_classes, opt.test_scales
    det.mean = np.asarray(opt.mean, np.float32).reshape(1, 1, 3)
    det.std = np.asarray(opt.std, np.float32).reshape(1, 1, 3)
    det.calib = DEFAULT
    return det


def test_run_frames_without_calibs_still_raises_and_names_the_argument():
    det = _host_detector()
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    with pytest.raises(NotImplementedError, match="calibs"):
        det.run_frames(frames)
    with pytest.raises(NotImplementedError, match="calibs"):
        list(det.run_frames_stream([(frames, None)]))


def test_calibs_forms():
    det = _host_detector()
    frames = [np.zeros((8, 8, 3), np.uint8)] * 3
    one = det._calibs_for(frames, KITTI)
    assert one.shape == (3, 3, 4) and one.dtype == np.float32 and all(np.array_equal(m, KITTI) for m in one)
    assert np.array_equal(det._calibs_for(frames, KITTI.tolist()), one)
    mixed = det._calibs_for(frames, [KITTI, None, KITTI.tolist()])
    assert np.array_equal(mixed[0], KITTI) and np.array_equal(mixed[1], DEFAULT) and np.array_equal(mixed[2], KITTI)
    assert np.array_equal(det._calibs_for(frames, np.stack([KITTI, DEFAULT, KITTI])), mixed)


@pytest.mark.parametrize("bad", [np.zeros((3, 3)), np.zeros((4, 3)), [KITTI, KITTI], [KITTI] * 4, "calib",
                                 [KITTI, None, np.zeros((3, 3))], np.zeros((3, 4, 1)), 1.0])
def test_malformed_calibs_raise_value_error(bad):
    det = _host_detector()
    frames = [np.zeros((8, 8, 3), np.uint8)] * 3
    with pytest.raises(ValueError):
        det.run_frames(frames, bad)
    with pytest.raises(ValueError):
        list(det.run_frames_stream([(frames, bad)]))


def test_stream_batches_are_pairs():
    det = _host_detector()
    with pytest.raises(ValueError):
        list(det.run_frames_stream([[np.zeros((8, 8, 3), np.uint8)] * 3]))
