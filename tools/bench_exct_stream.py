"""exct_decode, stored against streaming grouping (cn_exct_decode_f32 / cn_exct_decode_stream_f32): milliseconds per
call and per image on the exdet maps of the hourglass at the task's default 512 x 512 -- (B, 80, 128, 128) for B = 2
(a frame and its mirror image) and B = 32 -- with the hourglass forward at the same batch for scale.
  python tools/bench_exct_stream.py [--batches 2,32] [--reps 5] [--timeout 500] [--out profiles/exct_stream.txt]
Both forms at K = 40, the streaming form alone at K = 72, 100, 128 (the stored form ends at K = 64).  Event timing on
the current stream, two warm-up calls, the median and the minimum of `reps`.  Synthetic weights with one favoured class
and the thresholds at 0, as tools/bench_exdet_frames.py: groupings survive, so the select works on spread scores.  The
whole measurement runs under its own time limit (SIGALRM): a hang ends the tool with status 124."""
import argparse
import contextlib
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from centernet_amd import decode as D, synth
from centernet_amd.detectors.detector_factory import detector_factory
from centernet_amd.opts import opts

MAPS = ("hm_t", "hm_l", "hm_b", "hm_r", "hm_c", "reg_t", "reg_l", "reg_b", "reg_r")


def timed(fn, reps):
    """(median, minimum) milliseconds of fn() by events, after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_exct_stream: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)

    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["exdet", "--arch", "hourglass", "--flip_test", "--K", "40", "--scores_thresh", "0",
                           "--center_thresh", "0"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    with torch.no_grad():
        for k, v in det.model.state_dict().items():
            if k.split(".")[0] in MAPS[:5] and k.endswith("bias") and v.numel() == 80:
                v[17] += 3.0
    det.model.invalidate_plans()
    dev = torch.device("cuda:0")
    lines = ["exct_decode on the exdet maps of the hourglass at 512 x 512: (B, 80, 128, 128), num_dets 1000, "
             "median (minimum) of %d calls, events" % a.reps]
    for B in [int(b) for b in a.batches.split(",")]:
        frames = np.random.RandomState(5).randint(0, 256, (B // 2 + B % 2, 512, 512, 3)).astype(np.uint8)
        x = torch.cat([det.pre_process(f, 1.0)[0] for f in frames])[:B].to(dev)
        with torch.no_grad():
            fwd = timed(lambda: det.model(x, borrow=True), a.reps)
            out = det.model(x, borrow=True)[-1]
            maps = [out[n].sigmoid().clone() if n.startswith("hm") else out[n].clone() for n in MAPS]
        assert tuple(maps[0].shape) == (B, 80, 128, 128)
        lines.append("B = %2d   hourglass forward                    %9.3f ms (%9.3f)   %8.3f ms / image"
                     % (B, fwd[0], fwd[1], fwd[0] / B))
        same = None
        for K, forms in ((40, (False, True)), (72, (True,)), (100, (True,)), (128, (True,))):
            rows = {}
            for stream in forms:
                def call():
                    return D.exct_decode(*maps, K=K, scores_thresh=0.0, center_thresh=0.0, stream=stream)
                med, best = timed(call, a.reps)
                rows[stream] = call()
                lines.append("B = %2d   K = %3d  %-9s grouping + top-K   %9.3f ms (%9.3f)   %8.3f ms / image   %5.2f x forward"
                             % (B, K, "streaming" if stream else "stored", med, best, med / B, med / fwd[0]))
            if len(rows) == 2:
                same = bool(torch.equal(rows[False], rows[True]))
        lines.append("B = %2d   K =  40  stored and streaming rows are the same bits: %s" % (B, same))
    signal.alarm(0)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
