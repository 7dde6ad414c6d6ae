"""run_tiles on large frames against run_frames on the same tiles, and the tile merge against its host restatement.
python tools/bench_tiles.py [--task ctdet|multi_pose] [--frames 8] [--batches 24] [--K 100,32] [--out FILE]
ctdet resdcn_18 with seeded weights, 512 x 512 tiles at overlap 128 of 2160 x 3840 frames (10 x 6 = 60 tiles a frame),
once per value of --K (detections per tile):
  (a) run_tiles_stream, batches of --frames frames, tile_batch 32: frames/s and tiles/s, and how many batches the
      device tail handed back to the host (a class with more survivors than one soft-NMS holds);
  (b) run_frames_stream at B = 32 on the same tiles, cut on the host into 512 x 512 frames: img/s;
  (c) cn_ctdet_tiles_merge_f32 (its three launches, back to back between two device events) on the rows of one
      60-tile frame and of the whole batch, against post_process.ctdet_tiles_results on the same rows -- the rows
      as the stream left them, and the same rows with the classes dealt evenly (seeded weights on noise put most
      rows into one class, which at K = 100 is above the cap of a class segment).
--task multi_pose: dla_34 with seeded weights on the same frames, once per value of --K and of --min_score:
  (a) run_tiles_stream as above: frames/s, tiles/s and the batches handed back (a frame with more survivors than
      CN_POSE_TILES_MAX_ROWS);
  (c) cn_multi_pose_tiles_merge_f32 (one launch) between two device events on the rows of one frame and of the whole
      batch, against post_process.multi_pose_tiles_results on the same rows;
  (d) once: the workgroup-wide soft-NMS against the one-wave form it stands next to -- cn_multi_pose_tiles_merge_f32
      and cn_multi_pose_merge_f32 on the same seeded rows (infinite cores, no cut: both load, run soft-NMS and gather
      the same rows), segment lengths 64 ... 2048, the two calls alternating in one process (up to
      CN_POSE_TILES_ONE_WAVE_ROWS the new kernel runs its steps on one wave too: the crossover of the two forms).
--levels 0,1,2 (ctdet): the tile pyramid instead, once per value of --K:
  (p1) run_tiles_stream without levels and with them on the same frames, windows alternating in one process: frames/s,
       tiles/s, the tile counts per level and the batches handed back;
  (p2) cn_tile_box_normalize_u8_f32 alone per level -- all tiles of that level of two frames in one launch, between two
       device events -- with the bytes it must read and write per second, next to cn_warp_normalize_u8_f32_ragged on the
       same level-0 tiles.
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
from centernet_amd.post_process import ctdet_tiles_results, multi_pose_tiles_results

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
    ap.add_argument("--task", default="ctdet", choices=("ctdet", "multi_pose"))
    ap.add_argument("--min_score", default="none,0.1", help="multi_pose: score thresholds, one measurement per value")
    ap.add_argument("--levels", default=None, help="ctdet: pyramid levels, e.g. 0,1,2: measure the tile pyramid instead")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tiles needs a HIP device"
    if a.task == "multi_pose":
        return main_pose(a)
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
        if a.levels:
            measure_pyramid(det, a, frames, tuple(int(v) for v in a.levels.split(",")), lines)
        else:
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


# ------------------------------------------------------------------------------------------------
# --levels: the tile pyramid
# ------------------------------------------------------------------------------------------------
def measure_pyramid(det, a, frames, levels, lines):
    B, K = a.frames, det.opt.K
    pyr = tiles.pyramid_grid(H, W, TILE, TILE, OVERLAP, None, levels, None, 0.25, down_ratio=det.opt.down_ratio)
    T0 = tiles.tile_grid(H, W, TILE, TILE, OVERLAP).T
    lines.append("frames %d x %d, tiles %d x %d at overlap %d, %d frames a batch, K = %d; levels %s: %s = %d tiles a frame "
                 "(%d without levels), gates %s"
                 % (H, W, TILE, TILE, OVERLAP, B, K, levels, " + ".join(str(n) for n in pyr.level_T), pyr.T, T0,
                    pyr.bands.tolist()))

    # (p1) the two streams, windows alternating
    def stream(lv):
        return lambda n: det.run_tiles_stream((frames for _ in range(n)), depth=3, overlap=OVERLAP, tile_batch=32,
                                              levels=lv)
    rates, back = {None: [], levels: []}, {None: 0, levels: 0}
    for lv in (None, levels):
        list(stream(lv)(3))
    for _ in range(3):
        for lv in (None, levels):
            det.tail_fallbacks = 0
            rates[lv] += windows(stream(lv), a.batches, B, n=1)
            back[lv] += det.tail_fallbacks
    for lv, T in ((None, T0), (levels, pyr.T)):
        fps = float(np.median(rates[lv]))
        lines.append("(p1) run_tiles_stream(B=%d, tile_batch=32, depth=3, levels=%s), %d batches a window, alternating: "
                     "frames/s %s, median %.1f = %.0f tiles/s; tail_fallbacks %d of %d batches"
                     % (B, lv, a.batches, " ".join("%.1f" % r for r in rates[lv]), fps, fps * T, back[lv], 3 * a.batches))
    lines.append("(p1) frames/s with levels / without: %.3f; tiles with / without: %.3f"
                 % (np.median(rates[levels]) / np.median(rates[None]), pyr.T / float(T0)))

    # (p2) the box kernel alone per level, and the ragged warp on the level-0 tiles of the same two frames
    lib, nb = native.lib(), min(B, 2)
    src = torch.from_numpy(np.ascontiguousarray(np.stack(frames[:nb]))).cuda()
    pipe = det._tile_pipe_for(frames, 3, *det._tiles_args(OVERLAP, None, 32, None), 'bgr')
    mean, std = pipe.mean, pipe.std                      # (the detector's, as the C arrays the entries take)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f, reps=10):
        f()
        ts = []
        for _ in range(5):
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / reps * 1e3)
        return float(np.median(ts)), min(ts), max(ts)
    for l in (0, 1, 2, 3):
        g = tiles.tile_grid(-(-H // (1 << l)), -(-W // (1 << l)), TILE, TILE, OVERLAP)
        n = nb * g.T
        desc = np.zeros((n,), native.TILE_BOX_DESC)
        for b in range(nb):
            d = desc[b * g.T:(b + 1) * g.T]
            d['offset'], d['H'], d['W'], d['pitch'], d['level'] = b * H * W * 3, H, W, 3 * W, l
            d['y0'], d['x0'] = [o[0] for o in g.origins], [o[1] for o in g.origins]
        dd = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).cuda()
        out = torch.empty((n, 3, TILE, TILE), device="cuda")

        def box():
            native.check(lib.cn_tile_box_normalize_u8_f32(native.ptr(src), native.ptr(dd), n, TILE, TILE, mean, std,
                                                          native.ptr(out), native.stream_ptr()), "box")
        us, lo, hi = timed(box)
        nbytes = n * TILE * TILE * (3 * 4 ** l + 12)       # (tiles inside the frame; border tiles read less)
        lines.append("(p2) level %d: %d tiles (%d frames x %d): cn_tile_box_normalize_u8_f32 %.1f us (%.1f .. %.1f), "
                     "%.1f MB to read + write = %.2f TB/s" % (l, n, nb, g.T, us, lo, hi, nbytes / 1e6, nbytes / us / 1e6))
        if l == 0:
            idesc = np.zeros((n,), native.IMAGE_DESC)
            m = tiles.tile_maps(g, det.opt.down_ratio)[1]
            for b in range(nb):
                d = idesc[b * g.T:(b + 1) * g.T]
                d['offset'], d['H'], d['W'], d['pitch'], d['dst_to_src'] = b * H * W * 3, H, W, 3 * W, m
            idd = torch.from_numpy(idesc.view(np.uint8).reshape(-1).copy()).cuda()
            ref = torch.empty_like(out)

            def warp():
                native.check(lib.cn_warp_normalize_u8_f32_ragged(native.ptr(src), native.ptr(idd), n, TILE, TILE, mean,
                                                                 std, 0, native.ptr(ref), native.stream_ptr()), "warp")
            us, lo, hi = timed(warp)
            box()
            torch.cuda.synchronize()
            lines.append("(p2) level 0, the same tiles: cn_warp_normalize_u8_f32_ragged %.1f us (%.1f .. %.1f) = %.2f TB/s; "
                         "outputs bit-identical: %s"
                         % (us, lo, hi, nbytes / us / 1e6, torch.equal(out.view(torch.int32), ref.view(torch.int32))))
        del out


# ------------------------------------------------------------------------------------------------
# --task multi_pose
# ------------------------------------------------------------------------------------------------
def pose_rows(rng, n, clusters):
    """(n, 39) seeded rows: ``clusters`` > 0: boxes in that many dense clusters (the rows of tests/test_gpu_pose_tiles.py:
    most of them are discarded, few steps); 0: boxes spread over a 4K frame (few overlaps: as many steps as rows)"""
    if clusters:
        c = rng.uniform(0, 600, (clusters, 2))[rng.randint(0, clusters, n)] + rng.normal(0, 3.0, (n, 2))
    else:
        c = rng.uniform(0, 1, (n, 2)) * (W, H)
    wh = rng.uniform(8, 50, (n, 2))
    rows = np.empty((n, 39), np.float32)
    rows[:, 0:2], rows[:, 2:4] = c - wh / 2, c + wh / 2
    rows[:, 4] = rng.randint(1, 400, n) / np.float32(400)
    rows[:, 5:] = rng.uniform(-50, 700, (n, 34))
    return rows


def nms_forms(lines, rounds=15, reps=20):
    """(d): both kernels on the same rows, alternating; per call the median over the rounds and their spread"""
    lib = native.lib()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines.append("(d) soft-NMS forms, B = 2 frames of n rows (T = n / K tiles of K = min(n, 128)), infinite cores, no "
                 "cut; us per call, median of %d alternating rounds of %d calls (min .. max): "
                 "wg = cn_multi_pose_tiles_merge_f32 (16 waves), wave = cn_multi_pose_merge_f32 (1 wave)" % (rounds, reps))
    for clusters in (12, 0):
        for n in (64, 128, 256, 384, 512, 1024, 2048):
            B, K = 2, min(n, 128)
            T = n // K
            rows = pose_rows(np.random.RandomState(56 if (clusters, n) == (12, 2048) else 1000 + n), B * n, clusters)
            rows = rows.reshape(B * T, K, 39)
            host = rows[:T].reshape(n, 39).copy()
            kept = lib.cn_soft_nms_f32(host.ctypes.data, n, 39, 0.5, 0.5, 0.001, 2)
            tiles_in = torch.from_numpy(rows).cuda()
            scales_in = torch.from_numpy(np.ascontiguousarray(rows.reshape(B, T, K, 39).transpose(1, 0, 2, 3))).cuda()
            cores = torch.from_numpy(np.tile(np.array([-np.inf, -np.inf, np.inf, np.inf], np.float32), (T, 1))).cuda()
            out_a, out_b = torch.empty((B, n, 39), device="cuda"), torch.empty((B, n, 39), device="cuda")
            counts, status = torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
            ws = torch.empty((16,), dtype=torch.uint8, device="cuda")

            def wg():
                native.check(lib.cn_multi_pose_tiles_merge_f32(
                    native.ptr(tiles_in), B, T, K, native.ptr(cores), 1, n, float("nan"), native.ptr(out_a),
                    native.ptr(counts), native.ptr(status), native.ptr(ws), 16, native.stream_ptr()), "tiles merge")

            def wave():
                native.check(lib.cn_multi_pose_merge_f32(native.ptr(scales_in), T, B, K, 1, native.ptr(out_b),
                                                         native.stream_ptr()), "scale merge")

            def timed(f):
                e0.record()
                for _ in range(reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps * 1e3
            timed(wg), timed(wave)
            assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))      # the same bits
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(timed(wg))
                tb.append(timed(wave))
            lines.append("    %-9s n = %4d (%4d steps in frame 0): wg %8.1f (%.1f .. %.1f)   wave %8.1f (%.1f .. %.1f)   "
                         "wave / wg %.2f" % ("clustered" if clusters else "spread", n, min(kept, n), np.median(ta), min(ta),
                                             max(ta), np.median(tb), min(tb), max(tb), np.median(tb) / np.median(ta)))


def pose_merge_times(det, pipe, grid, rows, nb, min_score, lines):
    """(c) for the first ``nb`` frames of the host ``rows`` (B * T, K, 39): the launch between two device events
    against the host specification on the same rows"""
    lib, tail, T, K = native.lib(), pipe.tail, grid.T, det.opt.K
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    r = torch.from_numpy(rows).cuda()
    out_rows = torch.empty((nb, T * K, 39), device="cuda")
    counts = torch.empty((nb,), dtype=torch.int32, device="cuda")
    status = torch.empty((nb,), dtype=torch.int32, device="cuda")

    def run(reps):
        e0.record()
        for _ in range(reps):
            native.check(lib.cn_multi_pose_tiles_merge_f32(
                native.ptr(r), nb, T, K, native.ptr(pipe.cores_dev), int(bool(det.opt.nms)), pipe.max_per_frame,
                tail.min_score, native.ptr(out_rows), native.ptr(counts), native.ptr(status), native.ptr(tail.ws),
                tail.ws_bytes, native.stream_ptr()), "pose tiles merge")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    run(3)
    dev_ms = min(run(20) for _ in range(3))
    reps = 3
    survivors = []
    t0 = time.perf_counter()
    for _ in range(reps):
        for b in range(nb):
            host = multi_pose_tiles_results(list(rows[b * T:(b + 1) * T]), grid.cores, det.opt.nms, pipe.max_per_frame,
                                            min_score)
    host_ms = (time.perf_counter() - t0) / reps * 1e3
    from centernet_amd.tiles import in_core
    for b in range(nb):
        n = 0
        for t in range(T):
            keep = in_core(rows[b * T + t][:, :5], grid.cores[t])
            if min_score is not None:
                keep &= rows[b * T + t][:, 4] >= np.float32(min_score)
            n += int(keep.sum())
        survivors.append(n)
    lines.append("(c) %d frame(s) x %d tiles x K %d, min_score %s: survivors a frame %d .. %d, frames with status set %d: "
                 "cn_multi_pose_tiles_merge_f32 %.1f us for its 1 launch; multi_pose_tiles_results on the same rows "
                 "%.2f ms (%d rows kept in the last frame)"
                 % (nb, T, K, min_score, min(survivors), max(survivors), int((status != 0).sum()), dev_ms * 1e3, host_ms,
                    len(host[1])))


class Echo(list):
    """the report's lines, each shown on stderr as it is measured (the whole report is printed at the end)"""
    def append(self, line):
        print(line, file=sys.stderr, flush=True)
        list.append(self, line)


def main_pose(a):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["multi_pose", "--arch", "dla_34"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    lines = Echo(["box calibration: 512 MiB copy %.2f TB/s (read + write)" % calibration()])
    nms_forms(lines)
    B = a.frames
    rng = np.random.RandomState(5)
    frames = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(B)]
    grid = tiles.tile_grid(H, W, TILE, TILE, OVERLAP)
    for K in [int(v) for v in a.K.split(",")]:
        det.opt.K = K
        for pipe in det.__dict__.pop("_pipes", {}).values():     # (their tails are sized by K)
            pipe.pool.shutdown(wait=False)
        for ms in a.min_score.split(","):
            min_score = None if ms.lower() == "none" else float(ms)
            det.tail_fallbacks = 0
            lines.append("multi_pose dla_34: frames %d x %d, tiles %d x %d at overlap %d: %d x %d = %d tiles a frame, %d "
                         "frames a batch, K = %d, min_score %s, survivor cap %d"
                         % (H, W, TILE, TILE, OVERLAP, grid.nx, grid.ny, grid.T, B, K, min_score,
                            native.POSE_TILES_MAX_ROWS))

            def tile_stream(n):
                return det.run_tiles_stream((frames for _ in range(n)), depth=3, overlap=OVERLAP, tile_batch=32,
                                            arrays=True, min_score=min_score)
            list(tile_stream(3))
            det.tail_fallbacks = 0
            rates = windows(tile_stream, a.batches, B)
            fps = float(np.median(rates))
            lines.append("(a) run_tiles_stream(B=%d, tile_batch=32, depth=3, arrays=True), %d batches a window: frames/s %s, "
                         "median %.1f = %.0f tiles/s; tail_fallbacks %d of %d batches"
                         % (B, a.batches, " ".join("%.1f" % r for r in rates), fps, fps * grid.T, det.tail_fallbacks,
                            3 * a.batches))
            pipe = det._tile_pipe_for(frames, 3, *det._tiles_args(OVERLAP, None, 32, None), 'bgr', min_score=min_score)
            rows = pipe.tail.tile_rows.cpu().numpy()
            for nb in sorted({1, B}):
                pose_merge_times(det, pipe, grid, rows, nb, min_score, lines)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
