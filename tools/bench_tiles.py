"""run_tiles on large frames against run_frames on the same tiles, and the tile merge against its host restatement.
python tools/bench_tiles.py [--frames 8] [--batches 24] [--K 100,32] [--out FILE]
ctdet resdcn_18 with seeded weights, 512 x 512 tiles at overlap 128 of 2160 x 3840 frames (10 x 6 = 60 tiles a frame),
once per value of --K (detections per tile):
  (a) run_tiles_stream, batches of --frames frames, tile_batch 32: frames/s and tiles/s, and how many batches the
      device tail handed back to the host (a class with more survivors than one soft-NMS holds);
  (b) run_frames_stream at B = 32 on the same tiles, cut on the host into 512 x 512 frames: img/s;
  (c) cn_ctdet_tiles_merge_f32 (its three launches, back to back between two device events) on the rows of one
      60-tile frame and of the whole batch, against post_process.ctdet_tiles_results on the same rows -- the rows
      as the stream left them, and the same rows with the classes dealt evenly (seeded weights on noise put most
      rows into one class, which at K = 100 is above the cap of a class segment).
Every window ends in a device synchronise; the box calibration (cn_calib_copy, 512 MiB) is taken in the same process."""
import argparse
import contextlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from centernet_amd import native, synth, tiles
from centernet_amd.post_process import ctdet_tiles_results

H, W, TILE, OVERLAP = 2160, 3840, 512, 128


def calibration():
    lib, st = native.lib(), native.stream_ptr
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nbytes = 512 << 20
    src = torch.empty(nbytes // 4, device="cuda").normal_()
    dst = torch.empty_like(src)
    native.check(lib.cn_calib_copy(native.ptr(src), native.ptr(dst), nbytes, st()), "cn_calib_copy")
    e0.record()
    for _ in range(8):
        native.check(lib.cn_calib_copy(native.ptr(src), native.ptr(dst), nbytes, st()), "cn_calib_copy")
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * 8 / e0.elapsed_time(e1) / 1e9


def windows(make_stream, batches, per_batch, n=3):
    """n timed windows of ``batches`` batches each -> items/s per window (the stream is drained inside the window)"""
    rates = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = sum(1 for _ in make_stream(batches))
        torch.cuda.synchronize()
        rates.append(count * per_batch / (time.perf_counter() - t0))
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8, help="frames per run_tiles batch")
    ap.add_argument("--batches", type=int, default=24, help="run_tiles batches per timed window")
    ap.add_argument("--K", default="100,32", help="detections per tile, one measurement per value")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tiles needs a HIP device"
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet", "--arch", "resdcn_18"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    lines = ["box calibration: 512 MiB copy %.2f TB/s (read + write)" % calibration()]
    B = a.frames
    rng = np.random.RandomState(5)
    frames = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(B)]
    grid = tiles.tile_grid(H, W, TILE, TILE, OVERLAP)
    for K in [int(v) for v in a.K.split(",")]:
        det.opt.K = K
        det.tail_fallbacks = 0
        for pipe in det.__dict__.pop("_pipes", {}).values():     # (their tails are sized by K)
            pipe.pool.shutdown(wait=False)
        measure(det, a, frames, grid, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def merge_times(det, pipe, grid, rows, bounds, nb, what, lines):
    """(c) for the first ``nb`` frames of host ``rows`` / ``bounds``: the three launches between two device events
    against the host restatement on the same rows"""
    lib, tail, T, K, nc = native.lib(), pipe.tail, grid.T, det.opt.K, det.opt.num_classes
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    r, bd = torch.from_numpy(rows).cuda(), torch.from_numpy(bounds).cuda()
    out_rows = torch.empty((nb, T * K, 5), device="cuda")
    out_bounds = torch.empty((nb, nc + 1), dtype=torch.int32, device="cuda")
    status = torch.empty((nb,), dtype=torch.int32, device="cuda")

    def run(reps):
        e0.record()
        for _ in range(reps):
            native.check(lib.cn_ctdet_tiles_merge_f32(
                native.ptr(r), native.ptr(bd), nb, T, K, nc, native.ptr(pipe.cores_dev), int(bool(det.opt.nms)),
                pipe.max_per_frame, native.ptr(out_rows), native.ptr(out_bounds), native.ptr(status),
                native.ptr(tail.ws), tail.ws_bytes, native.stream_ptr()), "tiles merge")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    run(5)
    dev_ms = min(run(50) for _ in range(3))
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps):
        for b in range(nb):
            dicts = [{j + 1: rows[b * T + t, bounds[b * T + t, j]:bounds[b * T + t, j + 1]] for j in range(nc)}
                     for t in range(T)]
            host = ctdet_tiles_results(dicts, grid.cores, nc, det.opt.nms, pipe.max_per_frame)
    host_ms = (time.perf_counter() - t0) / reps * 1e3
    seg = max(int(sum(bounds[b * T + t, j + 1] - bounds[b * T + t, j] for t in range(T)))
              for b in range(nb) for j in range(nc))
    lines.append("(c) %s: %d frame(s) x %d tiles x K %d, %d rows in, longest class %d rows before the core filter, "
                 "frames with status set %d: cn_ctdet_tiles_merge_f32 %.1f us for its 3 launches; ctdet_tiles_results "
                 "on the same rows %.2f ms (%d rows kept in the last frame)"
                 % (what, nb, T, K, int(bounds[:nb * T, nc].sum()), seg, int((status != 0).sum()), dev_ms * 1e3,
                    host_ms, sum(len(v) for v in host.values())))


def measure(det, a, frames, grid, lines):
    B, T = a.frames, grid.T
    lines.append("frames %d x %d, tiles %d x %d at overlap %d: %d x %d = %d tiles a frame, %d frames a batch, K = %d"
                 % (H, W, TILE, TILE, OVERLAP, grid.nx, grid.ny, T, B, det.opt.K))

    # (a) the tile stream
    def tile_stream(n):
        return det.run_tiles_stream((frames for _ in range(n)), depth=3, overlap=OVERLAP, tile_batch=32)
    list(tile_stream(3))
    rates = windows(tile_stream, a.batches, B)
    fps = float(np.median(rates))
    lines.append("(a) run_tiles_stream(B=%d, tile_batch=32, depth=3), %d batches a window: frames/s %s, median %.1f "
                 "= %.0f tiles/s; tail_fallbacks %d"
                 % (B, a.batches, " ".join("%.1f" % r for r in rates), fps, fps * T, det.tail_fallbacks))

    # (b) the same tiles as 512 x 512 frames through run_frames_stream at B = 32
    cut = [np.ascontiguousarray(f[y0:y0 + TILE, x0:x0 + TILE]) for f in frames for y0, x0 in grid.origins]
    cut = cut[:len(cut) // 32 * 32] if len(cut) >= 32 else cut * (32 // len(cut) + 1)
    groups = [cut[i:i + 32] for i in range(0, len(cut) - 31, 32)]
    per_window = max(1, a.batches * B * T // 32)

    def frame_stream(n):
        return det.run_frames_stream((groups[i % len(groups)] for i in range(n)), depth=3)
    list(frame_stream(3))
    rates_b = windows(frame_stream, per_window, 32)
    ips = float(np.median(rates_b))
    lines.append("(b) run_frames_stream(B=32, depth=3) on the same tiles, %d batches a window: img/s %s, median %.0f"
                 % (per_window, " ".join("%.0f" % r for r in rates_b), ips))
    lines.append("(a) / (b) in tiles: %.3f" % (fps * T / ips))

    # (c) the merge alone: on the rows the stream's last batch left in the tail, and on the same rows with the
    # classes dealt evenly (row k of a tile in class k * nc // K: no class above the soft-NMS cap)
    pipe = det._tile_pipe_for(frames, 3, *det._tiles_args(OVERLAP, None, 32, None), 'bgr')
    K, nc = det.opt.K, det.opt.num_classes
    rows, bounds = pipe.tail.tile_rows.cpu().numpy(), pipe.tail.tile_bounds.cpu().numpy()
    even = np.tile(np.searchsorted(np.arange(K) * nc // K, np.arange(nc + 1)).astype(np.int32), (B * T, 1))
    for nb in sorted({1, B}):
        merge_times(det, pipe, grid, rows, bounds, nb, "rows as run", lines)
        merge_times(det, pipe, grid, rows, even, nb, "the same rows, classes dealt evenly", lines)


if __name__ == "__main__":
    sys.exit(main())
