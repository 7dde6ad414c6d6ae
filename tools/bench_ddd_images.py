"""ddd dla_34 at the default 384 x 1280 input, B = 32: images/s of run_images_stream on KITTI-sized images, the
four sizes of the dataset mixed and every image with its own projection matrix, against, in the same process and
alternated, (1) the loop of run(image, calib) over the same images -- the only path mixed sizes had -- and (2)
run_frames_stream on frames of the single size 375 x 1242, the ceiling: mixed sizes only add the descriptor upload.
  python tools/bench_ddd_images.py [--batch 32] [--batches 12] [--repeats 3] [--timeout 500] [--out profiles/ddd_images_bench.txt]
Seeded images.  The pre-process launch of both warp kernels is timed on its own, on the device.  The first line is
the box calibration of tools/bench_images.py.  The whole measurement runs under its own time limit (SIGALRM): a hang
ends the tool with status 124."""
import argparse
import contextlib
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_images import box_line
from centernet_amd import native, synth
from centernet_amd.detectors.detector_factory import detector_factory
from centernet_amd.opts import opts

SIZES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]       # KITTI's image sizes


def calib_like(rng):
    """a KITTI-like projection matrix: focal length, principal point and the translation column moved"""
    P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
                  [0.0, 0.0, 1.0, 0.002745884]], np.float32)
    P[0, 0] = P[1, 1] = np.float32(rng.uniform(650, 800))
    P[0, 2], P[1, 2] = rng.uniform(580, 640), rng.uniform(160, 190)
    P[:, 3] = rng.uniform(-60, 60, 3) * np.array([1, 0.05, 1e-4])
    return P.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_ddd_images: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)

    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ddd"])
        det = detector_factory[opt.task](opt)
    assert opt.arch == "dla_34" and (opt.input_h, opt.input_w) == (384, 1280)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    box = box_line(opt.device)
    rng = np.random.RandomState(5)
    B, n = a.batch, a.batches
    pool = [(rng.randint(0, 256, SIZES[i % len(SIZES)] + (3,)).astype(np.uint8), calib_like(rng)) for i in range(2 * B)]
    order = rng.permutation(len(pool))
    mixed = []
    for i in range(n):
        items = [pool[order[(i * B + j) % len(pool)]] for j in range(B)]
        mixed.append(([im for im, _ in items], [P for _, P in items]))
    one = [rng.randint(0, 256, SIZES[0] + (3,)).astype(np.uint8) for _ in range(2 * B)]
    frames = [([one[(i * B + j) % len(one)] for j in range(B)], [pool[j][1] for j in range(B)]) for i in range(n)]

    def images_stream():
        return sum(len(r) for r in det.run_images_stream(iter(mixed), depth=3))

    def frames_stream():
        return sum(len(r) for r in det.run_frames_stream(iter(frames), depth=3))

    def loop():
        for images, calibs in mixed[:max(1, n // 4)]:      # (a quarter of the batches: the loop is the slow side)
            for f, P in zip(images, calibs):
                det.run(f, P)
        return max(1, n // 4) * B

    fns = [("loop of run(image, calib), mixed sizes", loop), ("run_images_stream, mixed sizes", images_stream),
           ("run_frames_stream, 375x1242 frames", frames_stream)]
    rates = {name: [] for name, _ in fns}
    for name, fn in fns:                       # warm-up: plans of both batch sizes, calibration, pinned buffers
        fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):                 # alternating, so that a drift of the machine meets all three
        for name, fn in fns:
            t0 = time.perf_counter()
            images = fn()
            torch.cuda.synchronize()
            rates[name].append(images / (time.perf_counter() - t0))

    # ---- the pre-process launch of a batch alone, on the device
    def pre_ms(pipe, batch, reps=50):
        side = det._calibs_for(*batch)
        pipe.submit(0, batch[0], side)
        pipe.collect(0, batch[0])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            pipe._pre_process(0, 0, native.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    pre_i = pre_ms(det._image_pipe_for(mixed[0][0], 3), mixed[0])
    pre_f = pre_ms(det._pipe_for(frames[0][0], 3), frames[0])
    signal.alarm(0)

    def line(name):
        r = rates[name]
        return "%-40s %8.1f images/s   (min %.1f, max %.1f over %d)" % (name + ":", max(r), min(r), max(r), len(r))
    lo, im, fr = (rates[name] for name, _ in fns)
    lines = [box,
             "ddd dla_34 384x1280, B=%d, %d batches, %d alternating repeats; mixed sizes: %d seeded images of the %d "
             "KITTI sizes, one projection matrix per image" % (B, n, a.repeats, len(pool), len(SIZES))]
    lines += [line(name) for name, _ in fns]
    lines += ["run_images_stream / loop: %.1fx; run_images_stream / run_frames_stream: %.2f (best over best)"
              % (max(im) / max(lo), max(im) / max(fr)),
              "one batch of the stream: %.2f ms mixed, %.2f ms one-size" % (1e3 * B / max(im), 1e3 * B / max(fr)),
              "pre-process launch of one batch on the device (50 back to back): cn_warp_table_u8_f32_ragged %.3f ms, "
              "cn_warp_table_u8_f32_batch %.3f ms" % (pre_i, pre_f)]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if max(im) > max(lo) else 1       # the one condition: the stream beats the loop


if __name__ == "__main__":
    sys.exit(main())
