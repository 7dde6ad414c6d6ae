"""Decode kernel timing + phase ablation (GPU box only)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from centernet_amd import native
lib = native.lib()
SIG, CLEAN = native.DECODE_SIGMOID, native.DECODE_STATE_CLEAN
TWO, BAND = native.DECODE_TWO_LAUNCHES, native.DECODE_PER_BAND
dev = torch.device("cuda:0")
B, C, H, W, K = int(os.environ.get("B", 32)), 80, 128, 128, 100
g = torch.Generator().manual_seed(0)
wh = (40 * torch.rand((B, 2, H, W), generator=g)).to(dev)
reg = torch.rand((B, 2, H, W), generator=g).to(dev)


def heat_map(kind):
    """iid: independent Gaussian logits; net: the hm head of resdcn_18 on synthetic images
    (spatially smooth); floor: what a trained detector emits -- a smooth noise floor near
    sigmoid = 1e-3 with a few confident blobs, so the K-th peak lies INSIDE the floor."""
    if kind == "iid":
        return (2 * torch.randn((B, C, H, W), generator=g) - 2.19).to(dev)
    if kind == "net":
        from centernet_amd import synth
        from centernet_amd.model import create_model
        m = create_model("resdcn_18", {"hm": C, "wh": 2, "reg": 2}, 64)
        synth.fill_state_dict_(m, 317)
        m = m.to(dev).eval()
        with torch.no_grad():
            return m(synth.images(B, 4 * H, 4 * W, seed=0).to(dev))[-1]["hm"].clone()
    lo = torch.nn.functional.interpolate(torch.randn((B, C, H // 4, W // 4), generator=g), scale_factor=4,
                                         mode="bilinear", align_corners=False)
    x = -6.9 + 0.4 * lo + 0.05 * torch.randn((B, C, H, W), generator=g)
    for b in range(B):
        for _ in range(12):
            c, y, xx = (int(torch.randint(0, n_, (1,), generator=g)) for n_ in (C, H - 8, W - 8))
            yy, xg = torch.meshgrid(torch.arange(8.0), torch.arange(8.0), indexing="ij")
            x[b, c, y:y + 8, xx:xx + 8] += 8.0 * torch.exp(-((yy - 3.5) ** 2 + (xg - 3.5) ** 2) / 6.0)
    return x.to(dev)


def large_k(out_path):
    """LARGE_K=1: the large-K form (cn_ctdet_decode_large_f32) at K = 128, 256, 512 and 1024 beside the one-launch form
    at K = 128, on the three map kinds, in one run; logits in, the logistic fused; median (minimum) of 5 rounds of
    20 calls between two events.  Writes ``out_path`` (OUT=..., by default profiles/decode_large_k.txt) and ends."""
    lines = ["ctdet decode on (%d, %d, %d, %d) logits, the logistic fused: the large-K form (two launches, "
             "cn_ctdet_decode_large_f32) beside the one-launch form (cn_ctdet_decode_f32, owned workspace); "
             "median (minimum) of 5 rounds of 20 calls, events" % (B, C, H, W),
             "device: %s, %s, %d CUs" % (torch.cuda.get_device_name(0),
                                         getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"),
                                         torch.cuda.get_device_properties(0).multi_processor_count)]

    def timed(call, rounds=5, iters=20):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                call()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e) / iters)
        ms.sort()
        return ms[len(ms) // 2], ms[0]

    for kind in ("iid", "net", "floor"):
        x = heat_map(kind).contiguous()
        rows = {}
        for form, k in (("one launch", 128), ("large", 128), ("large", 256), ("large", 512), ("large", 1024)):
            large = form == "large"
            query = lib.cn_ctdet_decode_large_workspace_bytes if large else lib.cn_ctdet_decode_workspace_bytes
            entry = lib.cn_ctdet_decode_large_f32 if large else lib.cn_ctdet_decode_f32
            nb = query(B, C, H, W, k)
            w = torch.zeros(nb, device=dev, dtype=torch.uint8)
            d = torch.empty((B, k, 6), device=dev)
            i = torch.empty((B, k), device=dev, dtype=torch.int32)

            def call():
                rc = entry(native.ptr(x), native.ptr(wh), native.ptr(reg), B, C, H, W, k, 0, SIG | CLEAN,
                           native.ptr(d), native.ptr(i), native.ptr(w), nb, native.stream_ptr())
                assert rc == 0, rc
            med, low = timed(call)
            rows[(form, k)] = d.clone()
            lines.append("%-5s  %-10s  K = %4d   %8.3f ms (%8.3f)   workspace %6.1f MB" % (
                kind, form, k, med, low, nb / 1e6))
        same = torch.equal(rows[("one launch", 128)], rows[("large", 128)]) and all(
            torch.equal(rows[("large", k)][:, :128], rows[("large", 128)]) for k in (256, 512, 1024))
        lines.append("%-5s  K = 128 rows of both forms, and the first 128 rows at every K, are the same bits: %s" % (
            kind, same))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if os.environ.get("LARGE_K") == "1":
    large_k(os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                "profiles", "decode_large_k.txt")))
    sys.exit(0)

KIND = os.environ.get("HEAT", "iid")
logits = heat_map(KIND).contiguous()
# the reference-contract entry: ctdet_decode(heat) takes POST-sigmoid maps (models/decode.py:464).  (Round 4's
# "post-sigmoid in" line passed the raw logits with the sigmoid switched off -- negative "scores", every
# suppressed cell a zero ABOVE them: a plateau input, not a heat-map; its 0.125 / 0.487 ms were that.)
scores = torch.sigmoid(logits).contiguous()
print("heat map:", KIND)
dets = torch.empty((B, K, 6), device=dev)
inds = torch.empty((B, K), device=dev, dtype=torch.int32)
n = lib.cn_ctdet_decode_workspace_bytes(B, C, H, W, K)
ws = torch.empty(n, device=dev, dtype=torch.uint8)
alg = B * (C * H * W * 4 + 4 * H * W * 4 + K * 24)


def run(flags, iters=30):
    def call():
        rc = lib.cn_ctdet_decode_f32(native.ptr(logits), native.ptr(wh), native.ptr(reg), B, C, H, W, K, 0,
                                     flags, native.ptr(dets), native.ptr(inds), native.ptr(ws), n,
                                     native.stream_ptr())
        assert rc == 0, rc
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


zws = torch.zeros(n, device=dev, dtype=torch.uint8)     # owned + zeroed once: CN_DECODE_STATE_CLEAN


def check_forms():
    """all forms bit-identical on this map before anything is timed"""
    outs = []
    for flags, w in ((SIG | CLEAN, zws), (SIG, ws), (SIG | TWO, ws), (SIG | BAND, ws)):
        rc = lib.cn_ctdet_decode_f32(native.ptr(logits), native.ptr(wh), native.ptr(reg), B, C, H, W, K, 0,
                                     flags, native.ptr(dets), native.ptr(inds), native.ptr(w), n,
                                     native.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append((dets.clone(), inds.clone()))
    ok = all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    print("forms bit-identical:", ok)


check_forms()
for name, flags, w in (("one launch, owned workspace (default product path)", SIG | CLEAN, zws),
                       ("one launch + state fill (any caller)", SIG, ws),
                       ("one launch, post-sigmoid map in (reference contract)", CLEAN | (1 << 30), zws),
                       ("two launches (DECODE_TWO_LAUNCHES; round-4 first form)", SIG | TWO, ws),
                       ("per-band select of round 1 (DECODE_PER_BAND)", SIG | BAND, ws)):
    ws_cur = w

    def run_w(flags, iters=30, w=w):
        src = scores if flags & (1 << 30) else logits     # (bit 30: tool-side marker, not a library flag)
        flags &= ~(1 << 30)

        def call():
            rc = lib.cn_ctdet_decode_f32(native.ptr(src), native.ptr(wh), native.ptr(reg), B, C, H, W, K, 0,
                                         flags, native.ptr(dets), native.ptr(inds), native.ptr(w), n,
                                         native.stream_ptr())
            assert rc == 0, rc
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            call()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters

    ms = min(run_w(flags) for _ in range(3))
    print("%-52s %7.3f ms  %7.1f GB/s" % (name, ms, alg / ms / 1e6))

if os.environ.get("COLD") == "1":
    # the decode as the step sees it: between calls other kernels stream 2 GiB of other memory through
    # L2, the Infinity Cache and the address-translation caches (a copy), and the heat-map is REWRITTEN
    # (fresh lines, as behind the heads launch); only the decode is timed (events around it)
    big = torch.empty((1 << 30) // 4, device=dev)
    big2 = torch.empty_like(big)
    src = logits.clone()
    for cname, cflags in (("class-major (default)", SIG | CLEAN),):
        times = []
        for it in range(12):
            big2.copy_(big)
            logits.copy_(src)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rc = lib.cn_ctdet_decode_f32(native.ptr(logits), native.ptr(wh), native.ptr(reg), B, C, H, W, K, 0,
                                         cflags, native.ptr(dets), native.ptr(inds), native.ptr(zws), n,
                                         native.stream_ptr())
            assert rc == 0, rc
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        times = sorted(times[2:])
        print("one launch, COLD (2 GiB streamed + map rewritten before), %-22s %7.3f ms (median of %d; min %.3f)" % (
            cname, times[len(times) // 2], len(times), times[0]))
