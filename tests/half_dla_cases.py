"""Case lists, operand builders and float64 references shared by tests/test_gpu_half_dla.py (GPU) and
tests/test_half_dla_host.py (CPU): the half forms dla_34 needs in a half plan.  Not a test module.

* CONV16: the 16-channel 3x3 layers of cn_conv16.hip's half form (conv16h_kernel), each run with key 65 on
  (the new form) and off (stride 1: the LDS-halo kernel, stride 2: the implicit GEMM).
* SLICE_CONV: a half 3x3 / s1 convolution with BN + ReLU + residual that writes a channel slice of a wider
  buffer and reads its residual from a slice of another one.
* DW: cn_dw_conv_transpose_f16, (B, H, W, C, f), with and without ``add``.

A1 operands are built as tests/half_cases.py builds them (integers in {-1, 0, 1}, scales in {1, 2, -1, 0.5},
integer shifts and residuals); the exactness condition is half_cases.exactness on the float64 reference."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_cases as hc   # noqa: E402

KEY = 65                  # cn_set_tuning: the half form of cn_conv16.hip


def _c16(id, B, H, W, Cout, s, bn=False, bias=False, relu=False, out_pitch=None, c_off=0):
    return dict(id=id, kind="conv", B=B, Cin=16, H=H, W=W, Cout=Cout, k=3, s=s, p=1, bn=bn, bias=bias, relu=relu,
                res=False, out_pitch=out_pitch or Cout, c_off=c_off)


CONV16 = [
    _c16("s1", 1, 3, 128, 16, 1, bn=True, relu=True),
    _c16("s2", 2, 5, 256, 32, 2, bn=True, relu=True),                 # 3 x 128 outputs
    _c16("ragged_cout", 1, 3, 128, 24, 1, bias=True),
    # 528 row tiles for 512 resident workgroups: the tile loop and the register prefetch only run here
    _c16("persistent_loop", 2, 264, 128, 16, 1, bn=True, relu=True),
    # channels 8 .. 23 of a 40-wide half buffer (the other channels keep a sentinel)
    _c16("slice_out", 1, 3, 128, 16, 1, bn=True, relu=True, out_pitch=40, c_off=8),
]
CONV16_RUNS = [(c, on) for c in CONV16 for on in (1, 0)]
CONV16_IDS = ["%s-k%d=%d" % (c["id"], KEY, on) for c, on in CONV16_RUNS]

# 64 -> 64 on a 9 x 20 map, B = 2; output: channels 64 .. 127 of a 192-wide buffer, residual: channels
# 32 .. 95 of a 128-wide one
SLICE_CONV = dict(id="slice_conv", kind="conv", B=2, Cin=64, H=9, W=20, Cout=64, k=3, s=1, p=1, bn=True, bias=False,
                  relu=True, res=True, out_pitch=192, c_off=64, res_pitch=128, res_off=32)
SLICE_VARIANTS = ({5: 1}, {})
# the builder's fallback in a half plan: 128 -> 64 on the same map wants split-K (KT = 18, 3 workgroups), so
# cn_conv2d_res_pitch_supported answers 0 for an output slice (pitch 192) with a residual at its own pitch (64, a
# private tensor): the layer writes a private tensor and the buffer's slice stays untouched
FALLBACK_CONV = dict(id="fallback_conv", kind="conv", B=1, Cin=128, H=9, W=20, Cout=64, k=3, s=1, p=1, bn=True,
                     bias=False, relu=True, res=True, out_pitch=192, c_off=64)
# not a case of the half form: 16 -> 27 with CN_CONV_Y_PLAIN (y plain fp32 at pitch 32, the offset convolution of a
# half plan) keeps the routes that store fp32, key 65 on or off
YPLAIN_CONV = dict(id="yplain_16_27", kind="conv", B=1, Cin=16, H=3, W=128, Cout=27, k=3, s=1, p=1, bn=False,
                   bias=True, relu=False, res=False, out_pitch=32, c_off=0)
OTHER_CONV = [SLICE_CONV, FALLBACK_CONV, YPLAIN_CONV]

DW = [(2, 5, 7, 24, 2), (1, 3, 4, 64, 4), (1, 2, 3, 8, 8)]
DW_RUNS = [(s, a) for s in DW for a in (True, False)]
DW_IDS = ["%dx%dx%dx%d_f%d_%s" % (s + ("add" if a else "noadd",)) for s, a in DW_RUNS]


def conv_case(cid):
    return next(c for c in CONV16 + OTHER_CONV if c["id"] == cid)


@functools.lru_cache(maxsize=None)
def int_case(cid):
    """A1 operands and float64 reference of a convolution case: dict(x, w, bn, bias, res, ref)."""
    c = conv_case(cid)
    rng = np.random.RandomState(2100 + [k["id"] for k in CONV16 + OTHER_CONV].index(cid))
    B, Cin, H, W, Cout, k, s, p = (c[n] for n in ("B", "Cin", "H", "W", "Cout", "k", "s", "p"))
    x = hc._ints(rng, (B, Cin, H, W), -1, 1)
    w = hc._ints(rng, (Cout, Cin, k, k), -1, 1)
    bn, bias = hc._int_epilogue(rng, Cout, Cin * k * k, 2.0 / 3.0, c["bn"], c["bias"], c["relu"])
    Ho, Wo = hc.out_hw(c)
    res = hc._ints(rng, (B, Cout, Ho, Wo), -4, 4) if c["res"] else None
    return dict(x=x, w=w, bn=bn, bias=bias, res=res, ref=hc.ref64(x, w, bias, bn, res, c["relu"], s, p).detach())


def conv_desc(c, dtype, flags=0):
    """The cn_conv_desc of a CONV16 case as PlanBuilder.conv fills it."""
    from centernet_amd.native import ConvDesc, LAYOUT_NHWC
    Ho, Wo = hc.out_hw(c)
    return ConvDesc(B=c["B"], H=c["H"], W=c["W"], Cin=c["Cin"], Ho=Ho, Wo=Wo, Cout=c["Cout"], KH=3, KW=3,
                    stride=c["s"], pad_h=1, pad_w=1, dil=1, in_layout=LAYOUT_NHWC, in_pitch=c["Cin"],
                    out_layout=LAYOUT_NHWC, out_pitch=c["out_pitch"], OH=Ho, OW=Wo, oy_mul=1, oy_add=0, ox_mul=1,
                    ox_add=0, relu=int(c["relu"]), dtype=dtype, flags=flags)


# ---- depthwise transposed convolution ---------------------------------------------------------------------
def dw_ref64(x, w, add, f):
    """(ref64, sum of |terms|): ConvTranspose2d(C, C, 2f, f, f // 2, groups=C) (+ add) in float64, and the
    same with every operand's magnitude (the <= 4 products and ``add`` of an output value)."""
    C = x.shape[1]
    y = F.conv_transpose2d(x.double(), w.double(), None, f, f // 2, groups=C)
    mag = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, f, f // 2, groups=C)
    if add is not None:
        y, mag = y + add.double(), mag + add.double().abs()
    return y, mag


def dw_bilinear_weight(C, f):
    """The taps the module's own initialisation gives IDAUp's up-sampling (bilinear_upsample_init_): (C, 1, 2f, 2f)."""
    from centernet_amd.networks.common import bilinear_upsample_init_
    up = torch.nn.ConvTranspose2d(C, C, 2 * f, stride=f, padding=f // 2, groups=C, bias=False)
    return bilinear_upsample_init_(up).weight.detach().clone()


@functools.lru_cache(maxsize=None)
def dw_int_case(shape, with_add):
    """A1: bilinear taps are odd multiples a * b / (4 f^2); inputs are integers in [-2, 2] times 4 f^2, so every
    product is an integer; ``add`` integers in [-8, 8].  dict(x, w, add, ref, mag)."""
    B, H, W, C, f = shape
    rng = np.random.RandomState(3000 + DW.index(shape))
    w = dw_bilinear_weight(C, f)
    x = hc._ints(rng, (B, C, H, W), -2, 2) * (4 * f * f)
    add = hc._ints(rng, (B, C, H * f, W * f), -8, 8) if with_add else None
    ref, mag = dw_ref64(x, w, add, f)
    return dict(x=x, w=w, add=add, ref=ref, mag=mag)


def dw_exact(d, f):
    """The A1 condition of a dw case: inputs and ``add`` are fp16 integers, the taps times 4 f^2 are integers
    (so every product is an integer), and the sum of the terms' magnitudes stays <= 2048: every product and
    every partial sum, in any order, is an integer of at most 2048 -- an fp16 number -- and so is the result."""
    ints = lambda t: t is None or (torch.equal(t, t.round()) and torch.equal(t.half().float(), t))
    taps = d["w"].double() * (4 * f * f)
    xs = d["x"].double() / (4 * f * f)
    ok = ints(d["x"]) and ints(d["add"]) and torch.equal(taps, taps.round()) and torch.equal(xs, xs.round())
    return bool(ok) and float(d["mag"].max()) <= 2048 and hc.exactness(d["ref"])[0]
