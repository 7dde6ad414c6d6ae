"""The parallel form of soft-NMS that the device merge (cn_tail.hip) runs, restated in numpy and held
equal to the host soft-NMS ``cn_soft_nms_f32`` (pinned to the reference's cython, test_oracle_ref.py)
on seeded arrays: the whole in-place array, rows past the kept count included, bit for bit.

Per greedy step the form computes every live row's decayed score and discard flag at once, then walks
from discard to discard: a discarded row takes columns 0..4 of row N - 1 (columns 5.. are exchanged),
N shrinks and the moved row is looked at in the same place; the decayed scores are written last, where
their rows ended up."""
import numpy as np

from centernet_amd.soft_nms import soft_nms, soft_nms_39

F32 = np.float32


def _decay(boxes, i, N, sigma, threshold):
    """Decayed score and discard flag of every row p in (i, N), computed independently (lane-parallel)."""
    t = boxes[i, :4]
    b = boxes[i + 1:N]
    x1, y1, x2, y2, s = b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4]
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
    disc = touched & (ns < F32(threshold))
    return ns, disc


def soft_nms_parallel_form(boxes, sigma=0.5, threshold=0.001):
    """Gaussian soft-NMS in place, as the device form computes it; returns the kept count."""
    n = boxes.shape[0]
    N = n
    for i in range(n):
        if i >= N:
            break
        sc = boxes[i:N, 4]
        m = i + int(np.flatnonzero(sc == sc.max())[0])     # the first maximum
        tmp = boxes[i].copy()
        boxes[i] = boxes[m]
        boxes[m] = tmp
        ns, disc = _decay(boxes, i, N, sigma, threshold)
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
                    boxes[p, 4] = ns[orig[p]]
                    N = p
                    break
                last = N - 1
                boxes[p, :5] = boxes[last, :5]
                tail = boxes[p, 5:].copy()
                boxes[p, 5:] = boxes[last, 5:]
                boxes[last, 5:] = tail
                orig[p] = last
                N = last
                if not disc[last]:
                    break
            pos = p + 1
        q = np.arange(i + 1, N)
        boxes[q, 4] = ns[orig[q]]
    return N


def _clustered(rng, n, stride):
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
    if stride > 5:
        rows[:, 5:] = rng.uniform(-5, 300, (n, stride - 5))
    return rows


def _check(stride, seeds):
    ref_fn = soft_nms if stride == 5 else soft_nms_39
    n_disc = 0
    for seed in seeds:
        rng = np.random.RandomState(seed)
        rows = _clustered(rng, int(rng.choice([1, 2, 3, 8, 30, 90])), stride)
        want = rows.copy()
        kept = len(ref_fn(want, Nt=0.5, method=2))
        got = rows.copy()
        assert soft_nms_parallel_form(got) == kept, seed
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), seed
        n_disc += len(rows) - kept
    assert n_disc > 100          # the discard walk ran many times


def test_parallel_form_equals_host_soft_nms_stride5():
    _check(5, range(3000))


def test_parallel_form_equals_host_soft_nms_stride39():
    _check(39, range(10000, 11000))
