"""ctdet resdcn_18 at 512 x 512, B = 32: images/s of run_images_stream on images of MIXED sizes against, in the
same process and alternated, (1) the loop of run(image) over the same images -- the only path mixed sizes had,
the same code at the parent commit -- and (2) run_frames_stream on one-size 512 x 512 frames, the ceiling.
  python tools/bench_images.py [--batch 32] [--batches 48] [--repeats 3] [--timeout 500] [--out profiles/run_images_bench.txt]
Seeded images, sizes drawn from a fixed list (both orientations, sides from about 300 to about 700).  The host
side of a batch (tables + packing into the pinned buffer: ImagePipe._stage) is timed on its own, next to
FramePipe._stage for the one-size frames, and so is the pre-process launch on the device, to say where the
difference to the ceiling lies.  The first line is
the box calibration: a register-only fp16 MFMA loop and a 512 MiB copy, what this box delivers at the moment.
The whole measurement runs under its own time limit (SIGALRM): a hang ends the tool with status 124.
  python tools/bench_images.py --keep_res [--batch 32] [--batches 24] [--out profiles/keep_res_images_bench.txt]
--keep_res: the same network with the input following the image; run_images_stream batches the mixed sizes on
a canvas and is measured against the two routes mixed sizes had before it: the loop of
run(image), and run_frames_stream over hand-made buckets of one size each (which compute no padding).  The exit
status is 0 when the stream beats the loop and 1 when not; the ratio to the buckets is reported.
  python tools/bench_images.py --keep_res --steps 20
the step of one canvas batch on its ragged plan and of the same batch on the ordinary plan of the canvas size,
back to back -- the run to put under ``rocprofv3 --kernel-trace --stats`` for the share of the mask launches."""
import argparse
import contextlib
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from centernet_amd import native, synth
from centernet_amd.detectors.detector_factory import detector_factory
from centernet_amd.opts import opts

SIZES = [(375, 500), (500, 375), (480, 640), (640, 480), (427, 640), (640, 427), (333, 500), (500, 333),
         (300, 400), (400, 300), (512, 512), (600, 700), (700, 525), (360, 640), (640, 360), (612, 612)]


def box_line(dev):
    lib, st = native.lib(), native.stream_ptr
    sink = torch.zeros(16, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib.cn_calib_mfma_f16(native.ptr(sink), 200, st())
    e0.record()
    fl = lib.cn_calib_mfma_f16(native.ptr(sink), 20000, st())
    e1.record()
    torch.cuda.synchronize()
    tf = fl / e0.elapsed_time(e1) / 1e9
    nbytes = 512 << 20
    src = torch.empty(nbytes // 4, device=dev).normal_()
    dst = torch.empty_like(src)
    native.check(lib.cn_calib_copy(native.ptr(src), native.ptr(dst), nbytes, st()), "cn_calib_copy")
    e0.record()
    for _ in range(8):
        native.check(lib.cn_calib_copy(native.ptr(src), native.ptr(dst), nbytes, st()), "cn_calib_copy")
    e1.record()
    torch.cuda.synchronize()
    return "box calibration: fp16 MFMA loop %.0f TFLOP/s, 512 MiB copy %.2f TB/s (read + write)" % (
        tf, 2.0 * nbytes * 8 / e0.elapsed_time(e1) / 1e9)


KEEP_RES_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (375, 500), (640, 640)]      # (rows, columns)


def keep_res_detector():
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet", "--arch", "resdcn_18", "--keep_res"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    det.model.max_plans = 32         # six bucket shapes, six single-image shapes and the canvas stay planned
    return det, opt


def keep_res_steps(a):
    """``--keep_res --steps N``: N steps of one canvas batch, ragged plan, then N on the ordinary plan."""
    det, opt = keep_res_detector()
    rng = np.random.RandomState(5)
    batch = [rng.randint(0, 256, KEEP_RES_SIZES[j % len(KEEP_RES_SIZES)] + (3,)).astype(np.uint8) for j in range(a.batch)]
    pipe = det._canvas_pipe_for(batch, 1, None, "bench_images")
    pipe.submit(0, batch)
    pipe.collect(0, batch)
    x, rects = pipe.levels[0].batch, pipe._rects(0, 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for name, kw in (("ragged plan", {"rects": rects}), ("ordinary plan of the canvas", {})):
        for _ in range(3):
            det.run_batch(x, **kw)
        e0.record()
        for _ in range(a.steps):
            det.run_batch(x, **kw)
        e1.record()
        torch.cuda.synchronize()
        out.append("%s: %.3f ms per step (network + decode, B=%d, canvas %d x %d, %d steps)"
                   % (name, e0.elapsed_time(e1) / a.steps, a.batch, x.shape[2], x.shape[3], a.steps))
    plan = det.model.__dict__["_ran"]
    ragged = [p for k, p in det.model.__dict__["_plans"].items() if "ragged" in k][0]
    out.append("launches per step: ragged %d (of them %d masks), ordinary %d"
               % (len(ragged.b.ops), sum(m["kind"] == "mask" for m in ragged.b.meta), len(plan.b.ops)))
    assert det.range_ok()
    print("\n".join(out))
    return 0


def keep_res_main(a):
    det, opt = keep_res_detector()
    box = box_line(opt.device)
    rng = np.random.RandomState(5)
    B, n = a.batch, a.batches
    pool = [rng.randint(0, 256, KEEP_RES_SIZES[rng.randint(len(KEEP_RES_SIZES))] + (3,)).astype(np.uint8)
            for _ in range(3 * B)]
    mixed = [[pool[(i * B + j) % len(pool)] for j in range(B)] for i in range(n)]
    # the same number of images, sorted by hand into batches of one size each (a size's last batch filled up)
    per = max(1, n // len(KEEP_RES_SIZES))
    buckets = []
    for size in KEEP_RES_SIZES:
        own = [f for f in pool if f.shape[:2] == size] or [rng.randint(0, 256, size + (3,)).astype(np.uint8)]
        buckets.append([[own[(i * B + j) % len(own)] for j in range(B)] for i in range(per)])

    seen = set()

    def images_stream():
        done = sum(len(r) for r in det.run_images_stream(iter(mixed), depth=3))
        # (the stream's pipe, before the six bucket pipes push it out of the detector's four)
        seen.update(det._canvas_pipe_for(mixed[0], 3, None, "bench_images").levels[0].batches)
        return done

    def bucket_streams():
        return sum(len(r) for bucket in buckets for r in det.run_frames_stream(iter(bucket), depth=3))

    def loop():
        for b in mixed[:max(1, n // 4)]:
            for f in b:
                det.run(f)
        return max(1, n // 4) * B

    fns = [("loop of run(image)", loop), ("run_images_stream on canvases", images_stream),
           ("run_frames_stream per size bucket", bucket_streams)]
    rates = {name: [] for name, _ in fns}
    for name, fn in fns:
        fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, fn in fns:
            t0 = time.perf_counter()
            images = fn()
            torch.cuda.synchronize()
            rates[name].append(images / (time.perf_counter() - t0))
    signal.alarm(0)
    canvases = sorted(seen)
    area = np.mean([((f.shape[0] | opt.pad) + 1) * ((f.shape[1] | opt.pad) + 1) for b in mixed for f in b])

    def line(name):
        r = rates[name]
        return "%-36s %8.1f images/s   (min %.1f, max %.1f over %d)" % (name + ":", max(r), min(r), max(r), len(r))
    lo, im, bu = (rates[name] for name, _ in fns)
    lines = [box,
             "ctdet resdcn_18 --keep_res, B=%d, %d batches, %d alternating repeats; %d seeded images of the sizes %s; "
             "canvases seen: %s; an image's own input is %.0f %% of its canvas on average"
             % (B, n, a.repeats, len(pool), ", ".join("%dx%d" % (w, h) for h, w in KEEP_RES_SIZES),
                ", ".join("%d x %d" % c for c in canvases), 100.0 * area / (canvases[-1][0] * canvases[-1][1]))] + \
        [line(name) for name, _ in fns] + [
        "run_images_stream / loop: %.1fx (the condition: > 1); run_images_stream / buckets: %.2f (reported; best "
        "over best)" % (max(im) / max(lo), max(im) / max(bu))]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if max(im) > max(lo) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep_res", action="store_true")
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_images: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)
    if a.keep_res:
        return keep_res_steps(a) if a.steps else keep_res_main(a)

    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet", "--arch", "resdcn_18"])
        det = detector_factory[opt.task](opt)
    assert (opt.input_h, opt.input_w) == (512, 512) and opt.fix_res
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    box = box_line(opt.device)
    rng = np.random.RandomState(5)
    B, n = a.batch, a.batches
    pool = [rng.randint(0, 256, SIZES[rng.randint(len(SIZES))] + (3,)).astype(np.uint8) for _ in range(3 * B)]
    mixed = [[pool[(i * B + j) % len(pool)] for j in range(B)] for i in range(n)]
    square = [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(2 * B)]
    frames = [[square[(i * B + j) % len(square)] for j in range(B)] for i in range(n)]
    mean_bytes = np.mean([f.nbytes for b in mixed for f in b])

    def images_stream():
        return sum(len(r) for r in det.run_images_stream(iter(mixed), depth=3))

    def frames_stream():
        return sum(len(r) for r in det.run_frames_stream(iter(frames), depth=3))

    def loop():
        for b in mixed[:max(1, n // 4)]:        # (a quarter of the batches: the loop is the slow side)
            for f in b:
                det.run(f)
        return max(1, n // 4) * B

    fns = [("loop of run(image), mixed sizes", loop), ("run_images_stream, mixed sizes", images_stream),
           ("run_frames_stream, 512x512 frames", frames_stream)]
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

    # ---- the host side of a batch alone
    def stage_ms(pipe, batches):
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            for i, b in enumerate(batches):
                pipe._stage(i % pipe.depth, b)
            best = min(best, (time.perf_counter() - t0) * 1e3 / len(batches))
        return best
    ipipe, fpipe = det._image_pipe_for(mixed[0], 3), det._pipe_for(frames[0], 3)
    st_i, st_f = stage_ms(ipipe, mixed), stage_ms(fpipe, frames)
    desc = np.zeros_like(ipipe.desc_host[0])
    ts = np.zeros((len(ipipe.scales), B, 6))
    shapes = [[(f.shape[0], f.shape[1]) for f in b] for b in mixed]
    t0 = time.perf_counter()
    for s in shapes:
        ipipe.tables.fill(s, desc, ts)
    tab = (time.perf_counter() - t0) * 1e3 / len(shapes)

    # ---- the pre-process launch of a batch alone, on the device
    def pre_ms(pipe, batch, reps=50):
        pipe.submit(0, batch)
        pipe.collect(0, batch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            pipe._pre_process(0, 0, native.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    pre_i, pre_f = pre_ms(ipipe, mixed[0]), pre_ms(fpipe, frames[0])
    signal.alarm(0)

    def line(name):
        r = rates[name]
        return "%-36s %8.1f images/s   (min %.1f, max %.1f over %d)" % (name + ":", max(r), min(r), max(r), len(r))
    lo, im, fr = (rates[name] for name, _ in fns)
    lines = [box,
             "ctdet resdcn_18 512x512, B=%d, %d batches, %d alternating repeats; mixed sizes: %d seeded images of %d "
             "sizes, sides 300 .. 700, %.2f MB per image on average (512x512: 0.79 MB)"
             % (B, n, a.repeats, len(pool), len(SIZES), mean_bytes / 1e6)] + [line(name) for name, _ in fns] + [
        "run_images_stream / loop: %.1fx; run_images_stream / run_frames_stream: %.2f (best over best)"
        % (max(im) / max(lo), max(im) / max(fr)),
        "host side of one batch: ImagePipe._stage %.2f ms (of it the tables: %.2f ms), FramePipe._stage %.2f ms; "
        "one batch of the stream: %.2f ms mixed, %.2f ms one-size" % (st_i, tab, st_f, 1e3 * B / max(im), 1e3 * B / max(fr)),
        "pre-process launch of one batch on the device (50 back to back): cn_warp_normalize_u8_f32_ragged %.3f ms, "
        "cn_warp_normalize_u8_f32_batch %.3f ms" % (pre_i, pre_f)]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
