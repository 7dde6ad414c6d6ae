"""exdet task, hourglass at the task's default 512 x 512 with --flip_test and --K 40: images/s of the frame
pipe (run_frames, run_frames_stream) against the loop of run(frame) -- the only path the task had before the
pipe -- and the tail alone, device (cn_exdet_post_process_f32 + cn_exdet_merge_f32 + the slicing) against host
(the copy of the raw rows + exdet_results_batch), on the same rows.
  python tools/bench_exdet_frames.py [--batch 4] [--batches 6] [--repeats 3] [--timeout 500] [--out profiles/exdet_frame_pipe_bench.txt]
Synthetic weights with one favoured class and the thresholds at 0, so that groupings survive: every one of a
frame's 2000 rows is positive and nearly all share a class -- the longest soft-NMS segment the tail can meet.
The tail is therefore timed a second time on seeded rows spread over the 80 classes.  The loop and the pipe
alternate, `repeats` times each; the lines give the best and the spread.  The whole measurement runs under its
own time limit (SIGALRM): a hang ends the tool with status 124."""
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


def seeded_rows(rng, B, R, out_w, out_h, positive, nc=80):
    """(B, R, 14) raw rows: `positive` of them with a score > 0, clustered boxes, classes spread over nc"""
    d = np.zeros((B, R, 14), np.float32)
    centres = rng.uniform(0, 1, (40, 2)) * (out_w, out_h)
    c = centres[rng.randint(0, 40, (B, R))]
    wh = rng.uniform(2, 0.3 * out_w, (B, R, 2))
    d[:, :, 0:2] = c + rng.normal(0, 2.0, (B, R, 2)) - wh / 2
    d[:, :, 2:4] = d[:, :, 0:2] + wh
    d[:, :, 4] = np.where(rng.uniform(0, 1, (B, R)) < positive / float(R), rng.uniform(0.01, 1, (B, R)), -1)
    d[:, :, 13] = rng.randint(0, nc, (B, R))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_exdet_frames: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)

    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["exdet", "--arch", "hourglass", "--flip_test", "--K", "40", "--scores_thresh", "0",
                           "--center_thresh", "0"])
        det = detector_factory[opt.task](opt)
    assert (opt.input_h, opt.input_w) == (512, 512)
    synth.fill_state_dict_(det.model, 317)
    with torch.no_grad():
        for k, v in det.model.state_dict().items():
            if k.split(".")[0] in ("hm_t", "hm_l", "hm_b", "hm_r", "hm_c") and k.endswith("bias") and v.numel() == 80:
                v[17] += 3.0
    det.model.invalidate_plans()
    rng = np.random.RandomState(5)
    B, n = a.batch, a.batches
    pool = [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(2 * B)]
    batches = [[pool[(i * B + j) % len(pool)] for j in range(B)] for i in range(n)]

    def stream():
        return sum(len(r) for r in det.run_frames_stream(iter(batches), depth=3))

    def frames():
        return sum(len(det.run_frames(b)) for b in batches)

    def loop():
        for b in batches:
            for f in b:
                det.run(f)
        return n * B

    fns = [("loop of run(frame)", loop), ("run_frames", frames), ("run_frames_stream (depth 3)", stream)]
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
    fallbacks = det.tail_fallbacks

    # ---- the tail alone, on the same rows
    pipe = det._pipe_for(batches[0], 1)
    pipe.submit(0, batches[0])
    pipe.collect(0, batches[0])
    lv = pipe.levels[0]
    net_rows = det._run_scale(lv.batch, pipe.flip).clone()
    det.range_ok()
    seeded = torch.from_numpy(seeded_rows(rng, B, 2000, lv.meta['out_width'], lv.meta['out_height'], 600)).to(net_rows.device)

    def device_tail(raw):
        pipe.tail.run(0, 0, raw)
        pipe.tail.finish(0)
        torch.cuda.synchronize()
        return pipe.tail.results(0, B)

    def host_tail(raw):
        return det.results_batch(raw.cpu().numpy(), [lv.meta] * B, lv.scale)

    def ms(fn, raw, reps=5):
        fn(raw)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(reps):
            t0 = time.perf_counter()
            fn(raw)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    tails = []
    for what, raw in (("the network's rows", net_rows), ("seeded rows, 80 classes", seeded)):
        positive = int((raw[:, :, 4] > 0).sum().item()) // B
        dv, hs = device_tail(raw), host_tail(raw)
        same = all(np.array_equal(dv[i][j].view(np.uint32), hs[i][j].view(np.uint32)) and dv[i][j].shape == hs[i][j].shape
                   for i in range(B) for j in hs[i])
        tails.append("tail alone, %-24s (%4d positive rows / frame): device %7.2f ms  host %7.2f ms per batch  (same bits: %s)"
                     % (what, positive, ms(device_tail, raw), ms(host_tail, raw), same))
    signal.alarm(0)

    def line(name):
        r = rates[name]
        return "%-28s %7.1f images/s   (min %.1f, max %.1f over %d)" % (name + ":", max(r), min(r), max(r), len(r))
    lo, st = rates["loop of run(frame)"], rates["run_frames_stream (depth 3)"]
    lines = ["exdet hourglass 512x512 --flip_test --K 40, 512x512 uint8 frames, B=%d, %d batches, %d alternating repeats"
             % (B, n, a.repeats)] + [line(name) for name, _ in fns] + [
        "run_frames_stream / loop: %.2fx (best over best); spread of the loop %.1f%%, of the stream %.1f%%; batches handed "
        "back to the host tail: %d" % (max(st) / max(lo), 100 * (max(lo) - min(lo)) / max(lo),
                                       100 * (max(st) - min(st)) / max(st), fallbacks)] + tails
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if max(st) >= min(lo) else 1          # not slower than the loop beyond the measured spread


if __name__ == "__main__":
    sys.exit(main())
