"""Host-boundary (PCIe-inclusive) rates of the task API: uint8 frames in host memory ->
result dicts in host memory.  python tools/bench_e2e.py [arch] [--pixel-format {bgr,nv12}] [--stream-only]
--pixel-format nv12: run_frames / run_frames_stream take the seeded frames as NV12 (converted once, outside
every timed region; run(frame) has no NV12 form and gets their BGR conversion).  The last lines split one
B = 32 batch of the stream: staging into pinned memory, the upload, and the whole synchronous run_frames
(staging + upload + device + results), the NV12 converter launch on its own.  --stream-only: the
run_frames_stream lines and that split only."""
import argparse, os, sys, time, contextlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from centernet_amd import native, synth
from centernet_amd.image import bgr_to_nv12, nv12_to_bgr
from centernet_amd.opts import opts
from centernet_amd.detectors.detector_factory import detector_factory
ap = argparse.ArgumentParser()
ap.add_argument("arch", nargs="?", default="resdcn_18")
ap.add_argument("--pixel-format", choices=("bgr", "nv12"), default="bgr")
ap.add_argument("--stream-only", action="store_true")
args = ap.parse_args()
arch, fmt = args.arch, args.pixel_format
kw = {} if fmt == "bgr" else {"pixel_format": fmt}
with contextlib.redirect_stdout(sys.stderr):
    opt = opts().init(["ctdet", "--arch", arch])
    det = detector_factory[opt.task](opt)
synth.fill_state_dict_(det.model, 317)
det.model.invalidate_plans()
rng = np.random.RandomState(0)
frames = [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(32)]
if fmt == "nv12":        # the same seeded pictures as NV12, and what a decoder's frames look like in BGR
    pipe_frames = [bgr_to_nv12(f) for f in frames]
    frames = [nv12_to_bgr(f) for f in pipe_frames]
else:
    pipe_frames = frames
for host_pre in (() if args.stream_only else (True, False)):
    opt.host_pre_process = host_pre
    for f in frames[:3]: det.run(f)
    keys = ("tot", "load", "pre", "net", "dec", "post", "merge")
    acc = dict.fromkeys(keys, 0.0)
    t = time.perf_counter()
    for f in frames:
        r = det.run(f)
        for k in keys: acc[k] += r[k]
    dt = time.perf_counter() - t
    print("%s run(frame) %-11s %.2f ms/img (%.0f img/s)  " % (arch, "host-pre" if host_pre else "device-pre", dt / 32 * 1e3, 32 / dt)
          + " ".join("%s %.2f" % (k, acc[k] / 32 * 1e3) for k in keys))
for B in (() if args.stream_only else (8, 32)):
    fr = pipe_frames[:B]
    det.run_frames(fr, **kw); det.run_frames(fr, **kw)
    t = time.perf_counter()
    n = 5
    for _ in range(n): det.run_frames(fr, **kw)
    dt = (time.perf_counter() - t) / n
    print("%s run_frames(B=%d, %s) %.2f ms/batch  %.0f img/s (uint8 H2D + device pre-process + net + decode + D2H + host post)" % (arch, B, fmt, dt * 1e3, B / dt))

# pipelined form: batches staged / uploaded / collected around the device work (run_frames_stream)
for B in (8, 32):
    nb = 24
    batches = [[pipe_frames[(i + j) % 32] for j in range(B)] for i in range(nb)]
    for _ in det.run_frames_stream(iter(batches[:4]), **kw): pass
    t = time.perf_counter()
    n = sum(len(r) for r in det.run_frames_stream(iter(batches), **kw))
    dt = time.perf_counter() - t
    print("%s run_frames_stream(B=%d, %s) %.2f ms/batch  %.0f img/s (pinned staging by 4 threads + async uint8 H2D on a copy "
          "stream + batched device pre-process + net + decode + device tail + D2H, pipelined 3 deep, %d batches)"
          % (arch, B, fmt, dt / nb * 1e3, n / dt, nb))

# where one B = 32 batch of the stream spends its time
pipe = det._pipe_for(pipe_frames, 3, **kw)
torch.cuda.synchronize()
reps = 20
t = time.perf_counter()
for i in range(reps): pipe._stage(i % 3, pipe_frames)
stage = (time.perf_counter() - t) / reps * 1e3
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
with torch.cuda.stream(pipe.copy_stream):
    pipe._upload(0)
    e0.record()
    for i in range(reps): pipe._upload(i % 3)
    e1.record()
torch.cuda.synchronize()
upload = e0.elapsed_time(e1) / reps
t = time.perf_counter()
for _ in range(reps): det.run_frames(pipe_frames, **kw)
whole = (time.perf_counter() - t) / reps * 1e3
line = ("%s one B=32 batch, %s, %.1f MB staged and uploaded: staging %.2f ms, upload %.2f ms (%.1f GB/s), synchronous "
        "run_frames (staging + upload + device + results) %.2f ms" % (arch, fmt, pipe.pinned_in[0].numel() / 1e6, stage, upload,
                                                                     pipe.pinned_in[0].numel() / upload / 1e6, whole))
if pipe.bgr is not None:
    e0.record()
    for _ in range(reps): det._nv12_to_bgr_device(pipe.dev_in[0], pipe.bgr)
    e1.record()
    torch.cuda.synchronize()
    line += ", cn_nv12_to_bgr_u8_batch %.3f ms" % (e0.elapsed_time(e1) / reps)
print(line)
