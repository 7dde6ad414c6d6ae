"""--keep_res batches of mixed sizes on a canvas in fp16 compute mode: images/s of ``run_images`` of one detector
  python tools/bench_canvas_half.py [--task ctdet] [--arch resdcn_18] [--batch 32] [--canvas H W] [--out FILE]
(1) with --fp16 against the f32s default on the same canvas batch, (2) with --fp16 on the canvas against --fp16 image
by image through ``run``, and (3) the share of a step of the ragged half plan that its mask launches take: the plan
replayed with one event per launch, the launches that ``meta`` calls "mask" summed (next to it the same for the f32s
plan).  One seeded batch of the six sizes of tools/bench_images.py --keep_res; every leg is warmed up, then timed
over whole calls for at least 0.5 s, three alternating repeats, best and range reported.  The first line is the box
calibration.  The whole measurement runs under its own time limit (SIGALRM): a hang ends the tool with status 124."""
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
from bench_images import KEEP_RES_SIZES, box_line


def detector(task, arch, extra):
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task, "--arch", arch, "--keep_res"] + list(extra))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    det.model.max_plans = 32
    return det, opt


def rate(fn, images, seconds=0.5):
    """images/s of whole calls of ``fn`` over at least ``seconds``"""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n * images / dt


def mask_share(det, batch, canvas, steps=10):
    """(ms per network step, ms of it in mask launches, launches, mask launches, mask bytes) of the ragged plan"""
    pipe = det._canvas_pipe_for(batch, 1, canvas, "bench_canvas_half")
    pipe.submit(0, batch)
    pipe.collect(0, batch)
    x, rects = pipe.levels[0].batch, pipe._rects(0, 0)
    total = masks = 0.0
    for step in range(steps + 2):
        ev = []
        with torch.no_grad():
            det.model(x, rects=rects, borrow=True, events=ev, check=False)
        torch.cuda.synchronize()
        meta = det.model.__dict__["_ran"].b.meta
        assert len(ev) == len(meta) + 1
        if step >= 2:
            dt = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(meta))]
            total += sum(dt)
            masks += sum(d for d, m in zip(dt, meta) if m["kind"] == "mask")
    b = det.model.__dict__["_ran"].b
    assert b.ragged
    nm = sum(m["kind"] == "mask" for m in b.meta)
    return total / steps, masks / steps, len(b.meta), nm, sum(m["bytes"] for m in b.meta if m["kind"] == "mask"), \
        tuple(x.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="ctdet", choices=["ctdet", "multi_pose"])
    ap.add_argument("--arch", default="resdcn_18")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--canvas", type=int, nargs=2, default=None, metavar=("H", "W"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_canvas_half: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)

    canvas = tuple(a.canvas) if a.canvas else None
    half, opt = detector(a.task, a.arch, ["--fp16"])
    f32s, _ = detector(a.task, a.arch, [])
    assert half.model.compute_dtype == torch.float16 and f32s.model.uses_f32s()
    box = box_line(opt.device)
    rng = np.random.RandomState(5)
    B = a.batch
    batch = [rng.randint(0, 256, KEEP_RES_SIZES[j % len(KEEP_RES_SIZES)] + (3,)).astype(np.uint8) for j in range(B)]

    def loop():
        for f in batch:
            half.run(f)
    fns = [("--fp16 run_images on the canvas", lambda: half.run_images(batch, canvas=canvas)),
           ("f32s  run_images on the canvas", lambda: f32s.run_images(batch, canvas=canvas)),
           ("--fp16 loop of run(image)", loop)]
    rates = {name: [] for name, _ in fns}
    for name, fn in fns:                       # warm-up: plans, calibration, pinned buffers
        fn()
        fn()
    for _ in range(a.repeats):                 # alternating, so that a drift of the machine meets all three
        for name, fn in fns:
            rates[name].append(rate(fn, B))
    assert f32s.range_ok()
    shares = [(name, mask_share(det, batch, canvas)) for name, det in (("--fp16", half), ("f32s", f32s))]
    signal.alarm(0)

    def line(name):
        r = rates[name]
        return "%-34s %8.1f images/s   (min %.1f, max %.1f over %d)" % (name + ":", max(r), min(r), max(r), len(r))
    hc, fc, hl = (rates[name] for name, _ in fns)
    shape = shares[0][1][5]
    lines = [box,
             "%s %s --keep_res, one seeded batch of B=%d images of the sizes %s; canvas %d x %d%s; timed regions of "
             "at least 0.5 s, %d alternating repeats"
             % (a.task, a.arch, B, ", ".join("%dx%d" % (w, h) for h, w in KEEP_RES_SIZES), shape[2], shape[3],
                " (pinned)" if canvas else " (the batch's own maxima)", a.repeats)] + [line(name) for name, _ in fns] + [
        "--fp16 / f32s on the canvas: %.2fx; --fp16 canvas / --fp16 loop of run(image): %.1fx (best over best)"
        % (max(hc) / max(fc), max(hc) / max(hl))]
    for name, (ms, mask_ms, n, nm, nbytes, _) in shares:
        lines.append("%s ragged plan, by one event per launch: %.3f ms per network step, %d launches, of them %d masks "
                     "taking %.3f ms = %.1f %% of the step (%.1f MB of tensors under the masks)"
                     % (name, ms, n, nm, mask_ms, 100.0 * mask_ms / ms, nbytes / 1e6))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
