"""ctdet resdcn_18 at 512 x 512, B = 32: images/s of run_images_stream on images of MIXED sizes against, in the
same process and alternated, (1) the loop of run(image) over the same images -- the only path mixed sizes had,
the same code at the parent commit -- and (2) run_frames_stream on one-size 512 x 512 frames, the ceiling.
  python tools/bench_images.py [--batch 32] [--batches 48] [--repeats 3] [--timeout 500] [--out profiles/run_images_bench.txt]
Seeded images, sizes drawn from a fixed list (both orientations, sides from about 300 to about 700).  The host
side of a batch (tables + packing into the pinned buffer: ImagePipe._stage) is timed on its own, next to
FramePipe._stage for the one-size frames, and so is the pre-process launch on the device, to say where the
difference to the ceiling lies.  The first line is
the box calibration: a register-only fp16 MFMA loop and a 512 MiB copy, what this box delivers at the moment.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def expired(*_):
        sys.stderr.write("bench_images: time limit of %d s reached\n" % a.timeout)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.timeout)

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
