"""Case list, operand builders and float64 references of the fp16 compute mode's three new operations: the
deformable convolution (halves through cn_dcn_v2_forward_nhwc_f16), ConvTranspose 4x4/s2 and the max-pool.
Shared by tests/test_gpu_dcn_half.py (GPU) and tests/test_dcn_half_cases_host.py (CPU).  Not a test module.

The deformable reference builds the explicit columns (B, 9 * Cin, H * W) in float64 -- the modulated bilinear
samples of dcn_v2_im2col_cuda.cu:118-180, coordinates formed exactly from the fp32 offsets -- then contracts them
with the weight.  The kernels' arithmetic chain: corners read as halves, blend and mask multiply in fp32, ONE
rounding to fp16 as the sample enters the MFMA operand, fp32 accumulation, fp32 epilogue, one rounding to fp16 at
the store.

Forms (csrc/cn_dcn.hip dcn_route): the LDS-window form (csrc/cn_dcn_h.hip) takes H % 8 == 0, W % 16 == 0,
Cin % 64 == 0, Cout % 8 == 0 and > 32; by default only on grids of >= 192 workgroups, so the test-sized window
cases run it under cn_set_tuning key 23 = 2 (forced), the key the f32s register-sampling form is forced with.
Everything else is the gather form (igemm_kernel<_Float16, A_DCN / A_DCN_PAD>, csrc/cn_conv.hip), reached by
default routing; its tap split needs a workspace.
"""
import functools
import math

import numpy as np
import torch

WINDOW_KEYS = {23: 2}      # cn_set_tuning: force the LDS-window form on a grid below the chip-filling minimum
GATHER_KEYS = {23: 1}      # ... and the gather form on a shape the window form takes


def _c(id, shape, form, offsets="normal", pad=0, ws=False, relu=False, keys=None):
    B, Cin, H, W, Cout = shape
    return dict(id=id, B=B, Cin=Cin, H=H, W=W, Cout=Cout, form=form, offsets=offsets, pad=pad, ws=ws, relu=relu,
                keys=dict(keys if keys is not None else (WINDOW_KEYS if form == "window" else {})))


# form: what cn_dcn_v2_route must answer under ``keys``; offsets: "normal" N(0, 2) or "stress" (see stress_offsets);
# pad: out_pitch - Cout (the columns behind Cout keep the sentinel); ws: a workspace is given (the tap split runs)
CASES = [
    # ---- LDS-window form
    _c("win_one_tile", (2, 64, 8, 16, 64), "window"),                       # one tile per image, one chunk
    _c("win_2x2_two_chunks", (1, 128, 16, 32, 128), "window", relu=True),   # 2 x 2 tiles, every tile on a border
    _c("win_ragged_cout", (1, 64, 8, 16, 72), "window"),                    # 128-wide block, 72 channels stored
    _c("win_out_pitch", (1, 64, 8, 16, 64), "window", pad=16, relu=True),
    _c("win_stress", (1, 64, 8, 16, 64), "window", offsets="stress"),
    # ---- gather form
    _c("gat_cout24", (1, 64, 5, 7, 24), "gather"),                          # Cout <= 32: 128-pixel tiles
    _c("gat_pad", (1, 40, 6, 9, 64), "gather_pad", relu=True),              # Cin % 64 != 0: zero-filled last chunk
    _c("gat_split", (1, 128, 8, 8, 96), "gather", ws=True),                 # tap split: ksplit > 1
    _c("gat_nosplit", (1, 128, 8, 8, 96), "gather", ws=False),              # same layer, no workspace: ksplit 1
    _c("gat_stress", (1, 64, 5, 7, 24), "gather", offsets="stress"),
    # the window case's shape on the gather form (the two forms agree on it)
    _c("gat_on_window_shape", (2, 64, 8, 16, 64), "gather", keys=GATHER_KEYS),
    _c("gat_stress_window_shape", (1, 64, 8, 16, 64), "gather", offsets="stress", keys=GATHER_KEYS),
]
# integer-only offsets in the A1 form: K = 9 * Cin deep enough that eighths would leave the fp16 grid
DEEP_K = 9 * 128

DECONV_CASES = [(2, 64, 4, 6, 64), (1, 256, 4, 4, 128), (1, 96, 5, 7, 40)]      # (B, Cin, H, W, Cout)
POOL_CASES = [(2, 64, 17, 25, 3, 2, 1), (1, 24, 8, 8, 3, 2, 1), (2, 64, 17, 25, 2, 2, 0), (1, 24, 8, 8, 2, 2, 0)]


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


def _ints(rng, shape, lo, hi):
    return torch.from_numpy(rng.randint(lo, hi + 1, size=shape).astype(np.float32))


def stress_offsets(rng, B, H, W, half_steps=True):
    """(B, 18, H, W) offsets, multiples of 0.5: a base of small ones, and per pixel two taps from the stress
    set -- exactly -1 / H / W as the sample coordinate, integers, +-3.0 and +-3.5 (the window's reach on both
    sides), +-40 (far outside)."""
    step = 0.5 if half_steps else 1.0
    off = (_ints(rng, (B, 18, H, W), -4, 4) * step).numpy()
    special = np.array([3.0, -3.0, 3.5, -3.5, 40.0, -40.0, 2.0, -2.0, 0.0])
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(B):
        for tap in range(9):
            ki, kj = tap // 3, tap % 3
            pick = rng.randint(0, 14, size=(H, W))
            for ch, (o, k, n) in enumerate(((oy, ki, H), (ox, kj, W))):
                v = off[b, 2 * tap + ch]
                for i, s in enumerate(special):
                    v[pick == i] = s
                base = (o - 1 + k).astype(np.float64)
                v[pick == 9] = (-1.0 - base)[pick == 9]          # the sample coordinate is exactly -1: invalid
                v[pick == 10] = (float(n) - base)[pick == 10]    # ... exactly H (W): invalid
                v[pick == 11] = (float(n) - 1.0 - base)[pick == 11]   # ... the last row (column)
                v[pick == 12] = (-0.5 - base)[pick == 12]        # half a pixel outside: one corner row valid
                if not half_steps:
                    v[:] = np.round(v)
    return torch.from_numpy(off.astype(np.float32))


# ---- the float64 reference ------------------------------------------------------------------------------------
def cols64(x, off, mask):
    """Modulated deformable im2col, 3x3 / s1 / p1 / d1, in float64: (B, Cin * 9, H * W), row c * 9 + tap."""
    x, off, mask = x.double(), off.double(), mask.double()
    B, Cin, H, W = x.shape
    oy = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    ox = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    xf = x.reshape(B, Cin, H * W)
    out = torch.zeros(B, Cin, 9, H, W, dtype=torch.float64)
    for tap in range(9):
        ki, kj = tap // 3, tap % 3
        h_im = oy - 1 + ki + off[:, 2 * tap]
        w_im = ox - 1 + kj + off[:, 2 * tap + 1]
        valid = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)       # dcn_v2_im2col_cuda.cu:165
        hl, wl = torch.floor(h_im), torch.floor(w_im)
        lh, lw = h_im - hl, w_im - wl
        val = torch.zeros(B, Cin, H, W, dtype=torch.float64)
        for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            yy, xx = hl + dy, wl + dx
            ok = valid & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)         # :30-45
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(B, 1, H * W).expand(B, Cin, H * W)
            v = torch.gather(xf, 2, idx).view(B, Cin, H, W)
            val = val + v * (wt * ok.double()).unsqueeze(1)
        out[:, :, tap] = val * mask[:, tap].unsqueeze(1)
    return out.reshape(B, Cin * 9, H * W)


def dcn_ref64(x, off, mask, w, bias, scale, shift, relu):
    """-> (y (B, Cout, H, W) float64, cols): y = relu?((w . cols + bias) * scale + shift)."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    cols = cols64(x, off, mask)
    y = torch.einsum("ok,bkp->bop", w.double().reshape(Cout, Cin * 9), cols).view(B, Cout, H, W)
    v = lambda t: t.double().view(1, -1, 1, 1)
    y = (y + v(bias)) * v(scale) + v(shift)
    return (torch.relu(y) if relu else y), cols


def dcn_oracle32(x, off, mask, w, bias, scale, shift, relu):
    """The same through oracle's C deformable convolution (fp32, bit-identical to the reference kernel) and an fp32
    epilogue."""
    from oracle import cref
    y = cref.dcn_v2_forward(x.numpy(), off.numpy(), mask.numpy(), w.numpy(), bias.numpy())
    y = y * scale.numpy().reshape(1, -1, 1, 1).astype(np.float32) + shift.numpy().reshape(1, -1, 1, 1).astype(np.float32)
    return torch.from_numpy(np.maximum(y, 0) if relu else y)


def sample_term(w, cols, scale):
    """|scale| * 2^-11 * (|w| . |cols|): the one rounding of every sample to fp16, bounded term by term."""
    B = cols.shape[0]
    Cout = w.shape[0]
    s = torch.einsum("ok,bkp->bop", w.double().abs().reshape(Cout, -1), cols.abs())
    return (s * scale.double().abs().view(1, -1, 1)).reshape(B, Cout, -1) * 2.0 ** -11


# ---- A1: exact operands -----------------------------------------------------------------------------------------
def exactness(y):
    """The A1 condition on a float64 reference: every value an fp16 number.  -> (holds, max |y|, non-zero fraction)"""
    ok = bool((y.half().double() == y).all())
    return ok, float(y.abs().max()), float((y != 0).double().mean())


@functools.lru_cache(maxsize=None)
def int_case(cid):
    """Operands and reference of the A1 form of a deformable case: x integers in [-2, 2], w in {-1, 0, 1}, offsets
    multiples of 0.5 (integers on the deep-K cases), masks as probabilities in {0, 0.5, 1}, scales in
    {1, 2, -1, 0.5}, integer shifts and bias.  Every sample is then a multiple of 1/8 and every step exact."""
    c = case(cid)
    rng = np.random.RandomState(2000 + [k["id"] for k in CASES].index(cid))
    B, Cin, H, W, Cout = (c[n] for n in ("B", "Cin", "H", "W", "Cout"))
    deep = 9 * Cin >= DEEP_K
    x = _ints(rng, (B, Cin, H, W), -2, 2)
    w = _ints(rng, (Cout, Cin, 3, 3), -1, 1)
    if c["offsets"] == "stress":
        off = stress_offsets(rng, B, H, W, half_steps=not deep)
    else:
        off = _ints(rng, (B, 18, H, W), -4, 4) * (1.0 if deep else 0.5)
    mask = torch.tensor([0.0, 0.5, 1.0, 1.0])[torch.from_numpy(rng.randint(0, 4, size=(B, 9, H, W)))]
    scale = torch.tensor([1.0, 2.0, -1.0, 0.5])[torch.from_numpy(rng.randint(0, 4, size=(Cout,)))]
    bias = 2.0 * _ints(rng, (Cout,), -2, 2)
    # under ReLU: 1.7 standard deviations of the accumulator keep ~95 % of the outputs positive
    # (even, so that base * 0.5 stays an integer)
    base = 2 * int(math.ceil(0.85 * math.sqrt(9 * Cin * 2.0 * (2.0 / 3.0) * 0.4))) if c["relu"] else 0
    shift = base * scale.abs() + _ints(rng, (Cout,), -8, 8)
    ref, _ = dcn_ref64(x, off, mask, w, bias, scale, shift, c["relu"])
    return dict(x=x, w=w, off=off, mask=mask, bias=bias, scale=scale, shift=shift, ref=ref)


@functools.lru_cache(maxsize=None)
def normal_case(cid, logit_mask=False):
    """A2 operands: x and w rounded to fp16 first, offsets fp32 (N(0, 2) or the stress set), masks as
    probabilities.  -> dict with ref (float64), cols, e32 = max |C-oracle fp32 - ref64|."""
    from centernet_amd import synth
    c = case(cid)
    seed = 300 + 10 * [k["id"] for k in CASES].index(cid)
    B, Cin, H, W, Cout = (c[n] for n in ("B", "Cin", "H", "W", "Cout"))
    x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, seed)).half().float()
    w = torch.from_numpy(synth.normal((Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, seed + 1)).half().float()
    bias = torch.from_numpy(synth.normal((Cout,), 0.1, seed + 2))
    if c["offsets"] == "stress":
        off = stress_offsets(np.random.RandomState(seed), B, H, W)
    else:
        off = torch.from_numpy(synth.normal((B, 18, H, W), 2.0, seed + 3))
    mask = torch.from_numpy((1.0 / (1.0 + np.exp(-synth.normal((B, 9, H, W), 1.0, seed + 4)))).astype(np.float32))
    scale = torch.from_numpy(1.0 + 0.2 * synth.normal((Cout,), 1.0, seed + 5))
    shift = torch.from_numpy(synth.normal((Cout,), 0.3, seed + 6))
    ref, cols = dcn_ref64(x, off, mask, w, bias, scale, shift, c["relu"])
    o32 = dcn_oracle32(x, off, mask, w, bias, scale, shift, c["relu"])
    e32 = float((o32.double() - ref).abs().max())
    return dict(x=x, w=w, off=off, mask=mask, bias=bias, scale=scale, shift=shift, ref=ref, cols=cols, e32=e32, o32=o32)


def a2_bar(d):
    """The element-wise A2 bar of a normal case, split as (first three terms, 4 * E32):
    2^-11 |ref64| + 2^-25 + |scale| 2^-11 (|w| . |cols|)   and   4 E32."""
    ref = d["ref"]
    B, Cout, H, W = ref.shape
    three = ref.abs() * 2.0 ** -11 + 2.0 ** -25 + sample_term(d["w"], d["cols"], d["scale"]).view(B, Cout, H, W)
    return three, 4.0 * d["e32"]


# ---- the transposed convolution and the max-pool ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deconv_int_case(i):
    """A1 operands of DECONV_CASES[i]: x in {-1, 0, 1}, w in {-1, 0, 1} ((Cin, Cout, 4, 4): four taps per output),
    BatchNorm with scale in {1, 2, -1, 0.5} and integer shift, ReLU.  -> dict(x, w, bn, ref)"""
    import half_cases as hc
    import torch.nn.functional as F
    B, Cin, H, W, Cout = DECONV_CASES[i]
    rng = np.random.RandomState(4000 + i)
    x = _ints(rng, (B, Cin, H, W), -1, 1)
    w = _ints(rng, (Cin, Cout, 4, 4), -1, 1)
    bn, _ = hc._int_epilogue(rng, Cout, 4 * Cin, 2.0 / 3.0, True, False, True)
    ref = torch.relu(hc.bn64(F.conv_transpose2d(x.double(), w.double(), None, 2, 1), bn))
    return dict(x=x, w=w, bn=bn, ref=ref)


def pool_ref(x, k, s, p):
    import torch.nn.functional as F
    return F.max_pool2d(x.double(), k, s, p)
