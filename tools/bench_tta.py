"""Images/s of the test-time-augmentation settings of ctdet (the default) or multi_pose: run(frame), one
frame at a time, against run_frames_stream at batch B, for single scale, flip-test and flip-test + scales
0.5..1.5, on seeded 512 x 512 uint8 frames with --keep_res and synthetic weights.

    python tools/bench_tta.py [--task ctdet|multi_pose] [--archs resdcn_18,dla_34]
                              [--settings single,flip,flip5] [--batch 32] [--batches 6] [--frames 16]
                              [--skip-run] [--arrays]

--arrays: run_frames_stream(arrays=True) -- multi_pose rows as float32 arrays, not nested lists (ctdet
returns arrays either way).  Every shape is warmed up before its timed window.  Prints a table and one
JSON line (with "task" / "arrays" keys only when they are not the defaults)."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = {"single": [], "flip": ["--flip_test"],
            "flip5": ["--flip_test", "--test_scales", "0.5,0.75,1,1.25,1.5"]}


def detector(arch, extra, task="ctdet"):
    from centernet_amd import synth
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task, "--arch", arch, "--keep_res"] + extra)
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


def frames(n, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(n)]


def rate_run(det, n):
    fr = frames(n, 1)
    for f in fr[:2]:
        det.run(f)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in fr:
        det.run(f)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def rate_stream(det, B, nb, depth=3, arrays=False):
    kw = {"arrays": True} if arrays else {}
    pool = frames(B, 2)
    batches = [pool[i:] + pool[:i] for i in range(nb)]
    for _ in det.run_frames_stream(iter(batches[:depth + 1]), depth=depth, **kw):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for res in det.run_frames_stream(iter(batches), depth=depth, **kw):
        n += len(res)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--archs", default="resdcn_18,dla_34")
    p.add_argument("--settings", default="single,flip,flip5")
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--batches", type=int, default=6)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--skip-run", action="store_true", help="only run_frames_stream")
    p.add_argument("--task", default="ctdet", choices=["ctdet", "multi_pose"])
    p.add_argument("--arrays", action="store_true", help="run_frames_stream(arrays=True)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta needs a HIP device")
    rows = []
    for arch in a.archs.split(","):
        for name in a.settings.split(","):
            det = detector(arch, SETTINGS[name], a.task)
            r = {"arch": arch, "setting": name, "batch": a.batch}
            if a.task != "ctdet":
                r["task"] = a.task
            if a.arrays:
                r["arrays"] = True
            r["run_img_s"] = None if a.skip_run else round(rate_run(det, a.frames), 1)
            r["stream_img_s"] = round(rate_stream(det, a.batch, a.batches, arrays=a.arrays), 1)
            rows.append(r)
            print("%-10s %-7s run(frame) %8s img/s   run_frames_stream B=%d %8.1f img/s"
                  % (arch, name, r["run_img_s"], a.batch, r["stream_img_s"]), flush=True)
            del det
            torch.cuda.empty_cache()
    print(json.dumps({"bench_tta": rows}))


if __name__ == "__main__":
    main()
