"""ddd task, dla_34 at 384 x 1280 on 375 x 1242 frames: images/s of the frame pipe (run_frames_stream,
batches of B frames with their matrices) against a loop of run(frame, calib) -- the only path the task had
before the pipe (its pre-process on the host: --host_pre_process keeps that form) and as it is now.
  python tools/bench_ddd_frames.py [--batch 8] [--batches 12] [--timeout 240] [--out profiles/ddd_frame_pipe_bench.txt]
The whole measurement runs under its own time limit (SIGALRM): a hang ends the tool with status 124."""
import argparse
import contextlib
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from centernet_amd import synth
from centernet_amd.detectors.detector_factory import detector_factory
from centernet_amd.opts import opts

KITTI = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
                  [0.0, 0.0, 1.0, 0.002745884]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_ddd_frames: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)

    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ddd"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    rng = np.random.RandomState(5)
    B, n = a.batch, a.batches
    pool = [rng.randint(0, 256, (375, 1242, 3)).astype(np.uint8) for _ in range(2 * B)]
    batches = [([pool[(i * B + j) % len(pool)] for j in range(B)], [KITTI] * B) for i in range(n)]

    def stream():
        return sum(len(r) for r in det.run_frames_stream(iter(batches), depth=3))

    def loop(host_pre):
        opt.host_pre_process = host_pre
        for frames, calibs in batches:
            for f, p in zip(frames, calibs):
                det.run(f, p)
        opt.host_pre_process = False
        return n * B

    def rate(fn):
        fn()                                   # warm-up: plans, f32s calibration, pinned buffers
        torch.cuda.synchronize()
        best = 0.0
        for _ in range(3):
            t0 = time.perf_counter()
            images = fn()
            torch.cuda.synchronize()
            best = max(best, images / (time.perf_counter() - t0))
        return best

    pipe = rate(stream)
    parent = rate(lambda: loop(True))
    now = rate(lambda: loop(False))
    signal.alarm(0)
    lines = ["ddd dla_34 384x1280, 375x1242 uint8 frames, B=%d, %d batches, best of 3" % (B, n),
             "run_frames_stream (depth 3):                 %8.1f images/s" % pipe,
             "loop of run(frame, calib), host pre-process: %8.1f images/s   (the path before the pipe)" % parent,
             "loop of run(frame, calib), device pre-process: %6.1f images/s" % now,
             "pipe / loop (host pre-process): %.2fx" % (pipe / parent)]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if pipe > parent else 1


if __name__ == "__main__":
    sys.exit(main())
