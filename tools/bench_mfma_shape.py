"""The f32s step of the persistent 3x3 kernel as a bare loop, v_mfma_f32_32x32x16_f16 against
v_mfma_f32_16x16x32_f16 (cn_calib_mfma_shape, cn_misc.hip): same wave tile (64 pixels x 32 channels),
same three products per tile, same 12 operand fragments per step -- kept in registers, or read again from
LDS in every step as the kernel does -- at two waves per SIMD.  The chip lowers its clock under a dense
matrix loop by an amount that depends on the operand DATA, so the comparison runs on random values (split
into fp16 high / low parts like the kernel's operands, and full-range fp16 noise); all-zero operands are
the control that ranks the shapes by cycles alone.  GPU box only.

usage: python tools/bench_mfma_shape.py
       ROUNDS=9 ITERS=20000 WARM_S=2.0 DATA=split,noise,zeros python tools/bench_mfma_shape.py

Per (data, arrangement): the two shapes alternate launch by launch after WARM_S seconds of back-to-back
launches of both; reported are the median and the min .. max of TFLOP/s by wall (HIP events, un-stamped
build), the in-kernel clock of the stamped build (shader cycles / 100 MHz ticks of wave 0's loop, median over
workgroups), the SIMD cycles one wave's step costs by wall (wall time x clock / steps / 2 waves per SIMD: 384 =
the matrix pipe never idle.  Not the stamped wave's own cycle count: the older wave of a SIMD is served first, so
wave 0 finishes early and its count says little about the pair), and the ratio 16x16x32 / 32x32x16 of every round.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from centernet_amd import native

dev = torch.device("cuda:0")
lib = native.lib()
st = native.stream_ptr

ROUNDS = int(os.environ.get("ROUNDS", "9"))
ITERS = int(os.environ.get("ITERS", "20000"))
WARM_S = float(os.environ.get("WARM_S", "2.0"))
DATA = os.environ.get("DATA", "split,noise,zeros").split(",")
WAVES, FRAGS = 8, 12


def operands(kind, shape, seed=0):
    """(WAVES, FRAGS, 64 lanes, 8) fp16.  `split`: every (high, low) fragment pair is the fp16 split of
    fp32 normal noise, the low part in the fragment the shape multiplies as `low`."""
    g = torch.Generator().manual_seed(seed)
    if kind == "zeros":
        return torch.zeros((WAVES, FRAGS, 64, 8), dtype=torch.float16)
    if kind == "noise":
        return (torch.rand((WAVES, FRAGS, 64, 8), generator=g) * 2 - 1).to(torch.float16)
    v = torch.randn((WAVES, FRAGS // 2, 64, 8), generator=g)
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    out = torch.empty((WAVES, FRAGS, 64, 8), dtype=torch.float16)
    if shape == 16:      # fragments 2 b + part
        out[:, 0::2], out[:, 1::2] = hi, lo
    else:                # fragments 4 b + 2 part + kh
        hi, lo = hi.view(WAVES, 3, 2, 64, 8), lo.view(WAVES, 3, 2, 64, 8)
        o = out.view(WAVES, 3, 2, 2, 64, 8)
        o[:, :, 0], o[:, :, 1] = hi, lo
    return out


sink = torch.zeros(64, device=dev)
stamps = torch.zeros(2 * 256, device=dev, dtype=torch.int64)


def launch(ops, shape, from_lds, stamped):
    fl = lib.cn_calib_mfma_shape(native.ptr(ops), native.ptr(sink), native.ptr(stamps) if stamped else None,
                                 shape, from_lds, ITERS, st())
    assert fl > 0, "cn_calib_mfma_shape failed"
    return fl


def timed(ops, shape, from_lds, stamped):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fl = launch(ops, shape, from_lds, stamped)
    e.record()
    torch.cuda.synchronize()
    return fl / (s.elapsed_time(e) * 1e-3) / 1e12


def med(v):
    return sorted(v)[len(v) // 2]


print("cn_calib_mfma_shape: 256 workgroups x 8 waves, %d steps per wave, %d rounds, %.1f s warm-up per block"
      % (ITERS, ROUNDS, WARM_S))
for kind in DATA:
    ops = {sh: operands(kind, sh).to(dev) for sh in (32, 16)}
    for from_lds in (0, 1):
        t_end = time.time() + WARM_S
        while time.time() < t_end:
            for _ in range(4):
                for sh in (32, 16):
                    launch(ops[sh], sh, from_lds, False)
            torch.cuda.synchronize()
        tf = {32: [], 16: []}
        tfs = {32: [], 16: []}
        clk = {32: [], 16: []}
        for _ in range(ROUNDS):
            for sh in (32, 16):
                tf[sh].append(timed(ops[sh], sh, from_lds, False))
            for sh in (32, 16):
                stamps.zero_()
                tfs[sh].append(timed(ops[sh], sh, from_lds, True))
                s2 = stamps.view(256, 2).cpu().double()
                clk[sh].append(float((s2[:, 0] / s2[:, 1]).median()) * 0.1)      # GHz
        arr = "LDS reads every step" if from_lds else "operands in registers"
        print("== data %-5s | %s" % (kind, arr))
        flops = 256.0 * WAVES * ITERS * 3 * 2 * 64 * 32 * 32
        cyc = {sh: flops / (med(tf[sh]) * 1e12) * med(clk[sh]) * 1e9 / ITERS / 2 for sh in (32, 16)}
        for sh in (32, 16):
            name = "32x32x16" if sh == 32 else "16x16x32"
            print("   %s  wall %7.1f TFLOP/s (%7.1f .. %7.1f) | stamped build: wall %7.1f, clock %.3f GHz (%.3f .. %.3f), "
                  "%.1f SIMD cycles per step and wave" % (name, med(tf[sh]), min(tf[sh]), max(tf[sh]), med(tfs[sh]),
                                                          med(clk[sh]), min(clk[sh]), max(clk[sh]), cyc[sh]))
        ratio = [b / a for a, b in zip(tf[32], tf[16])]
        print("   16x16x32 / 32x32x16 by wall: median %.4f (rounds %.4f .. %.4f); repeat spread of 32x32x16 %.4f, of "
              "16x16x32 %.4f; clock ratio %.4f; cycle ratio %.4f"
              % (med(ratio), min(ratio), max(ratio), max(tf[32]) / min(tf[32]) - 1, max(tf[16]) / min(tf[16]) - 1,
                 med(clk[16]) / med(clk[32]), cyc[16] / cyc[32]))
