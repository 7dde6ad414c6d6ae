"""Host side of the exdet frame pipe: the vectorised host tail ``post_process.exdet_results_batch`` against the
oracle's statement-by-statement ``exdet_post_process`` + ``exdet_merge_outputs`` per frame, bit for bit over
every class key, on seeded raw rows.  ``exdet_rows`` / ``exdet_meta`` build the synthetic input;
tests/test_gpu_exdet_pipe.py uses the same for the device tail."""
import types

import numpy as np
import pytest

from centernet_amd.detectors.exdet import ExdetDetector
from centernet_amd.post_process import exdet_post_batch, exdet_results_batch
from centernet_amd.soft_nms import soft_nms
from oracle import post_oracle

NUM_CLASSES = 80


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exdet_meta(h, w, scale, keep_res, input_res=256, pad=31, down_ratio=4):
    """meta of one test scale, as ``BaseDetector.input_geometry`` + ``_meta`` give it"""
    sh, sw = int(h * scale), int(w * scale)
    if keep_res:
        inp_h, inp_w = (sh | pad) + 1, (sw | pad) + 1
        c, s = np.array([sw // 2, sh // 2], dtype=np.float32), np.array([inp_w, inp_h], dtype=np.float32)
    else:
        inp_h = inp_w = input_res
        c, s = np.array([sw / 2., sh / 2.], dtype=np.float32), max(h, w) * 1.0
    return {'c': c, 's': s, 'out_height': inp_h // down_ratio, 'out_width': inp_w // down_ratio}


def exdet_rows(rng, n, R, out_w, out_h, positive, num_classes=NUM_CLASSES, strays=True, favoured=0.0):
    """(n, R, 14) raw rows as the exdet decode leaves them: ``positive`` rows per frame (an int, or one per
    frame) carry a score > 0 out of a few levels (repeats: ties at the cut) down to values that soft-NMS
    decays under its threshold; the others carry the decode's rejections (-1), zeros and NaNs.  Boxes in dense
    clusters, partly outside the grid.  Classes: a few crowded ones (``favoured``: that share in class 17),
    and with ``strays`` ids outside [0, num_classes), fractional ids and NaN."""
    d = np.zeros((n, R, 14), np.float32)
    positive = np.broadcast_to(np.asarray(positive), (n,))
    crowded = rng.choice(num_classes, 6, replace=False)
    for i in range(n):
        centres = rng.uniform(-0.1, 1.1, (max(1, R // 120), 2)) * (out_w, out_h)
        c = centres[rng.randint(0, len(centres), R)]
        wh = rng.uniform(1, 0.3 * out_w, (R, 2))
        xy1 = c + rng.normal(0, rng.choice([0.3, 2.0]), (R, 2)) - wh / 2
        d[i, :, 0:2], d[i, :, 2:4] = xy1, xy1 + wh
        levels = rng.choice([4, 20, 1000])
        score = (rng.randint(1, levels + 1, R) / levels) * rng.choice([0.002, 0.05, 1.0], R)
        bad = rng.choice([-1.0, -1.0, 0.0, -0.0, np.nan, -3.5], R)
        pos = np.zeros(R, bool)
        pos[rng.permutation(R)[:positive[i]]] = True
        d[i, :, 4] = np.where(pos, score, bad)
        d[i, :, 5:13] = rng.uniform(-5, out_w + 5, (R, 8))
        cls = np.where(rng.uniform(0, 1, R) < 0.7, rng.choice(crowded, R), rng.randint(0, num_classes, R)).astype(np.float64)
        cls = np.where(rng.uniform(0, 1, R) < favoured, 17.0, cls)
        if strays:
            stray = rng.uniform(0, 1, R) < 0.08
            cls = np.where(stray, rng.choice([-1.0, float(num_classes), num_classes + 5.0, 1.5, np.nan, -0.5], R), cls)
        d[i, :, 13] = cls
    return d


def oracle_results(per_scale, i, num_classes=NUM_CLASSES, max_per_image=100):
    posts = [post_oracle.exdet_post_process(d[i], metas[i], scale) for d, metas, scale in per_scale]
    return posts, post_oracle.exdet_merge_outputs(posts, num_classes, max_per_image)


def _discards(posts, num_classes=NUM_CLASSES):
    """rows that soft-NMS drops from the frame's class segments (the library's routine, pinned to the oracle's)"""
    rows = np.concatenate(posts, axis=0).astype(np.float32)
    rows = rows[rows[:, 4] > 0]
    n = 0
    for j in range(num_classes):
        seg = np.ascontiguousarray(rows[rows[:, 13] == j][:, 0:5])
        n += len(seg) - len(soft_nms(seg, Nt=0.5, method=2))
    return n


def assert_same_results(got, want, num_classes=NUM_CLASSES, what=""):
    assert sorted(got) == sorted(want) == list(range(1, num_classes + 1)), what
    for j in want:
        assert got[j].dtype == np.float32 and got[j].ndim == 2 and got[j].shape == want[j].shape, (what, j, got[j].shape, want[j].shape)
        assert np.array_equal(_bits(got[j]), _bits(want[j])), (what, j)


CASES = {
    # name: (R, scales, keep_res, (h, w), positives per frame)
    "flip_single": (2000, (1.0,), False, (300, 400), (260, 0, 150, 40)),
    "noflip_single": (1000, (1.0,), False, (256, 256), (180, 3, 0, 101)),
    "flip_scaled": (2000, (0.75,), False, (375, 500), (220, 90)),
    "flip_keep_res": (2000, (1.0,), True, (300, 420), (200, 120)),
    "multi_keep_res": (2000, (0.5, 1.0, 1.5), True, (200, 280), (150, 60, 0)),
    "multi_fix_res": (1000, (0.75, 1.25), False, (256, 320), (130, 100)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_batch_equals_the_oracle_tail(name):
    R, scales, keep_res, (h, w), positive = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) + 40)
    n = len(positive)
    per_scale = []
    for scale in scales:
        meta = exdet_meta(h, w, scale, keep_res)
        per_scale.append((exdet_rows(rng, n, R, meta['out_width'], meta['out_height'], positive), [meta] * n, scale))
    if len(scales) > 1 and keep_res:
        assert len({m[0]['out_width'] for _, m, _ in per_scale}) == len(scales)     # another mirror axis per scale
    before = [d.copy() for d, _, _ in per_scale]
    got = exdet_results_batch(per_scale, NUM_CLASSES)
    assert all(np.array_equal(_bits(d), _bits(b)) for (d, _, _), b in zip(per_scale, before))     # input untouched
    assert len(got) == n
    discards = cut = empty = 0
    for i in range(n):
        posts, want = oracle_results(per_scale, i)
        assert_same_results(got[i], want, what=(name, i))
        discards += _discards(posts)
        rows = sum(len(v) for v in want.values())
        present = int(sum(np.sum((p[:, 4] > 0) & np.isin(p[:, 13], np.arange(NUM_CLASSES))) for p in posts))
        if present > 100:
            assert 100 <= rows < present                # the cut ran; `>=` keeps ties, so it may keep more than 100
            cut += 1
        empty += rows == 0
        # _post_batch + the detector's own merge_outputs (the pipe's multi-scale host route): the same
        ns = types.SimpleNamespace(num_classes=NUM_CLASSES, max_per_image=100)
        mine = [ExdetDetector._post_batch(ns, d, m, s)[i] for d, m, s in per_scale]
        for a, b in zip(mine, posts):
            assert np.array_equal(_bits(a[:, 0:5]), _bits(b[:, 0:5]))
        assert_same_results(ExdetDetector.merge_outputs(ns, mine), want, what=(name, i, "merge_outputs"))
    assert cut >= 1, name
    assert discards > 20, (name, discards)               # soft-NMS discarded rows: the order-dependent part ran
    if name in ("flip_single", "noflip_single", "multi_keep_res"):
        assert empty >= 1


def test_ties_at_the_cut_are_kept_and_strays_drop():
    """a frame whose 100-th score is shared: more than 100 rows come back; NaN / non-positive scores and class
    values outside [0, nc) (or no integers) never do"""
    rng = np.random.RandomState(7)
    meta = exdet_meta(256, 256, 1.0, False)
    d = exdet_rows(rng, 1, 2000, 64, 64, 0, strays=False)
    # 160 far-apart boxes (no overlap: soft-NMS leaves their scores), scores out of three values
    k = np.arange(160)
    d[0, k, 0], d[0, k, 1] = (k % 16) * 4.0, (k // 16) * 4.0
    d[0, k, 2], d[0, k, 3] = d[0, k, 0] + 1.0, d[0, k, 1] + 1.0
    d[0, k, 4] = np.where(k < 60, 0.9, np.where(k < 130, 0.5, 0.25))
    d[0, k, 13] = k % 5
    d[0, 160:170, 4] = 0.99
    d[0, 160:170, 13] = [-1, 80, 81, 1.5, np.nan, -0.5, 1e9, -1e9, 79.5, 80]
    d[0, 170:180, 13] = 3
    d[0, 170:180, 4] = [np.nan, 0.0, -0.0, -1, -1, np.nan, -5, 0, 0, -1]
    got = exdet_results_batch([(d, [meta], 1.0)], NUM_CLASSES)[0]
    _, want = oracle_results([(d, [meta], 1.0)], 0)
    assert_same_results(got, want)
    assert sum(len(v) for v in got.values()) == 130       # 60 + the 70 that tie at the threshold
    assert all(len(got[j]) == 0 for j in range(6, 81))


def test_post_batch_serves_frames_of_different_geometry():
    rng = np.random.RandomState(3)
    metas = [exdet_meta(300, 400, 1.0, True), exdet_meta(256, 256, 1.0, False), exdet_meta(300, 400, 1.0, True)]
    d = exdet_rows(rng, 3, 1000, 64, 64, 300)
    rows = exdet_post_batch(d, metas, 0.5)
    for i in range(3):
        want = post_oracle.exdet_post_process(d[i], metas[i], 0.5)
        assert np.array_equal(_bits(rows[i]), _bits(want), )
