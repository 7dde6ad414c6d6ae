"""cn_nv12_to_bgr_u8_batch alone against its byte roofline: 1.5 bytes read and 3 bytes written per pixel, over the
copy bandwidth this box delivers at the moment (cn_calib_copy, 512 MiB, read + write bytes), at 32 x 512 x 512
(one batch of the frame stream) and 8 x 1080 x 1920.  python tools/bench_nv12.py [--out FILE]
Back-to-back launches between two device events; the 512 x 512 batch (13 + 25 MB) lives in the Infinity Cache
when it is converted again and again, so it is also timed on a ring of buffers larger than that cache."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from centernet_amd import native


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nv12 needs a HIP device"
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
    copy = 2.0 * nbytes * 8 / e0.elapsed_time(e1) / 1e9          # TB/s
    del src, dst
    lines = ["box calibration: 512 MiB copy %.2f TB/s (read + write)" % copy]
    for N, H, W in ((32, 512, 512), (8, 1080, 1920)):
        frame = H * 3 // 2 * W
        ring = max(1, -(-(1 << 30) // (N * frame * 3)))          # buffers of more than 1 GiB in all
        for name, k in (("one buffer", 1), ("ring of %d" % ring, ring)):
            ins = [torch.randint(0, 256, (N, H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(k)]
            outs = [torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(k)]

            def run(reps):
                e0.record()
                for i in range(reps):
                    native.check(lib.cn_nv12_to_bgr_u8_batch(native.ptr(ins[i % k]), N, frame, H, W, W,
                                                             native.ptr(outs[i % k]), st()), "cn_nv12_to_bgr_u8_batch")
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps
            run(3 * k)
            ms = min(run(50 * k if k == 1 else 4 * k) for _ in range(3))
            moved = 4.5 * N * H * W
            lines.append("cn_nv12_to_bgr_u8_batch %d x %d x %d, %s: %.1f us, %.2f TB/s of its 4.5 B/pixel (%.1f MB), "
                         "%.2f of the copy's rate; roofline at that rate %.1f us"
                         % (N, H, W, name, ms * 1e3, moved / ms / 1e9, moved / 1e6, moved / ms / 1e9 / copy,
                            moved / copy / 1e6))
            del ins, outs
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
