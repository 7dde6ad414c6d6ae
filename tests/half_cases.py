"""Case list, input builders and float64 references shared by tests/test_gpu_half.py (GPU) and
tests/test_half_cases_host.py (CPU).  Not a test module.

A case is a dict: ``id``; ``kind`` ("conv", "stem" or "heads"); the shape (B, Cin, H, W, Cout, k, s, p);
the epilogue (``bn`` or ``bias``, ``relu``, ``res``); ``variants``: the cn_set_tuning settings the case
runs under (one run each); ``form``: the kernel form the fp16 run reaches, read off conv_route /
plan_ksplit (csrc/cn_conv.hip) and c3_dispatch (csrc/cn_conv3x3.hip).

Routing facts used below (fp16: 64-channel K chunks, KT = k * k * ceil(Cin / 64)): a dense layer whose
grid has fewer than 256 workgroups splits K as soon as KT >= 16, i.e. every 3x3 layer with Cin > 64 at
test-sized maps leaves the LDS-halo kernel for the split-K implicit GEMM.  Cases that must stay on the
halo kernel (or on the un-split implicit GEMM) with more than one K chunk therefore run with key 5 = 1
(never split K) -- the form the same layer takes at network-sized maps, where the grid is full.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

NOSPLIT = {5: 1}


def _c(id, kind, shape, bn=False, bias=False, relu=False, res=False, variants=({},), form=""):
    B, Cin, H, W, Cout, k, s, p = shape
    return dict(id=id, kind=kind, B=B, Cin=Cin, H=H, W=W, Cout=Cout, k=k, s=s, p=p, bn=bn, bias=bias,
                relu=relu, res=res, variants=tuple(variants), form=form)


CASES = [
    # KT = 9 < 16: no split.  Cout = 64: 64-wide N; W = 32: 4 x 32 tiles
    _c("halo64_4x32", "conv", (2, 64, 32, 32, 64, 3, 1, 1), bn=True, relu=True, res=True,
       form="conv3x3s1_kernel<_Float16, 32, 64, 2, 2>"),
    # KT = 18, 3 workgroups: would split in two -> key 5 = 1.  W = 20 < 32: 8 x 16 tiles, 13 rows and 20
    # columns leave ragged tiles; two full K chunks
    _c("halo64_8x16_ragged", "conv", (1, 128, 13, 20, 64, 3, 1, 1), bn=True, relu=True,
       variants=(NOSPLIT, {}),
       form="key 5 = 1: conv3x3s1_kernel<_Float16, 16, 64, 2, 2>; default: split-K implicit GEMM, 2 slices"),
    # Cout = 224: 128-wide N (padding 32 < 64), Cout % 64 != 0 keeps it there; KT = 9.  Key 15: 8 / 4 waves
    _c("halo128", "conv", (1, 64, 16, 32, 224, 3, 1, 1), bn=True, relu=True, res=True,
       variants=({15: 1}, {15: 0}),
       form="conv3x3s1_kernel<_Float16, 32, 128, 4, 2> (key 15 = 1) / <.., 2, 2> (key 15 = 0)"),
    # Cout = 24: 32-wide N, ragged; KT = 9; W = 40: 4 x 32 tiles, second tile column 8 wide, 9 rows
    _c("halo32_ragged_cout", "conv", (1, 64, 9, 40, 24, 3, 1, 1), bias=True,
       form="conv3x3s1_kernel<_Float16, 32, 32, 4, 1>"),
    # Cin = 96 / 72: second 64-channel chunk half / one-eighth full.  KT = 18 -> key 5 = 1 for the halo kernel
    _c("halo64_partial_chunk_96", "conv", (2, 96, 11, 17, 64, 3, 1, 1), bn=True, relu=True, res=True,
       variants=(NOSPLIT, {}),
       form="key 5 = 1: conv3x3s1_kernel<_Float16, 16, 64, 2, 2>, nchunk 2; default: split-K implicit GEMM"),
    _c("halo64_partial_chunk_72", "conv", (1, 72, 8, 16, 40, 3, 1, 1), bias=True, variants=(NOSPLIT, {}),
       form="key 5 = 1: conv3x3s1_kernel<_Float16, 16, 64, 2, 2>, nchunk 2; default: split-K implicit GEMM"),
    # stride 2: implicit GEMM, 128-wide N; key 4 picks the pixel tile.  KT = 18 would split in two: key 5 = 1
    # for the kernel's own epilogue, the default setting (64-pixel tiles, two K slices + reduce) as well
    _c("igemm_3x3s2", "conv", (2, 128, 32, 32, 256, 3, 2, 1), bn=True, relu=True,
       variants=({4: 64, 5: 1}, {4: 128, 5: 1}, {}),
       form="igemm_kernel<_Float16, 64 | 128, 128, 2, 2, A_DENSE>; default: BM = 64, 2 K slices + reduce"),
    # 1x1 / s1: KT = 4, implicit GEMM 128-wide N, 64-pixel tiles (3 x 2 workgroups); M = 323 ragged
    _c("igemm_1x1_res_relu", "conv", (1, 256, 17, 19, 256, 1, 1, 0), bn=True, relu=True, res=True,
       form="igemm_kernel<_Float16, 64, 128, 2, 2, A_DENSE>"),
    # 1x1 / s2 on an odd map (9 x 10 outputs), Cin = 96: partial second chunk, Cout = 72: 128-wide N
    _c("igemm_1x1s2_skip", "conv", (1, 96, 17, 19, 72, 1, 2, 0), bn=True,
       form="igemm_kernel<_Float16, 64, 128, 2, 2, A_DENSE>, stride 2"),
    # split-K: KT = 54, 2 workgroups -> 6 slices, Cout = 200 (cout_pad 224); KT = 72, 4 workgroups -> 9 slices
    _c("splitk_ragged_cout", "conv", (1, 384, 8, 8, 200, 3, 1, 1), bn=True, relu=True, res=True,
       form="igemm_kernel<_Float16, 64, 128> x 6 K slices + splitk_reduce_kernel<_Float16>"),
    _c("splitk_deep", "conv", (1, 512, 4, 4, 512, 3, 1, 1), bn=True, relu=True, res=True,
       form="igemm_kernel<_Float16, 64, 128> x 9 K slices + splitk_reduce_kernel<_Float16>"),
    # the un-fused heads of heads_from_convs: 3x3 64 -> 192 (64-wide N: 192 = 3 x 64; W = 20: 8 x 16 tiles),
    # then 1x1 convolutions on channel slices (pitch 192, offsets 0 / 64 / 128) writing fp32 NCHW
    _c("heads_sliced_nchw", "heads", (2, 64, 12, 20, 192, 3, 1, 1), bias=True, relu=True,
       form="conv3x3s1_kernel<_Float16, 16, 64, 2, 2>, then igemm_kernel<_Float16, 128, 128 | 32 | 32, OUT_NCHW>"),
    # the 7x7 / s2 stem on the fp32 NCHW image: K = 147 in three 64-wide chunks, 17 x 25 outputs
    _c("stem_ragged", "stem", (2, 3, 33, 50, 128, 7, 2, 3), bn=True, relu=True,
       form="igemm_kernel<_Float16, 128, 128, 2, 2, A_STEM>"),
]
HEAD_COUTS = (80, 2, 1)
HEAD_HIDDEN = 64


def runs():
    """(case, knobs) for every variant of every case, with a readable id."""
    out = []
    for c in CASES:
        for v in c["variants"]:
            tag = "-".join("k%d=%d" % kv for kv in sorted(v.items())) or "default"
            out.append((c, v, "%s-%s" % (c["id"], tag)))
    return out


def out_hw(c):
    return ((c["H"] + 2 * c["p"] - c["k"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["k"]) // c["s"] + 1)


def make_bn(scale, mean, beta):
    """BatchNorm2d(eval) with eps = 0 and unit variance: fold_bn gives scale and beta - mean * scale exactly."""
    C = scale.numel()
    bn = torch.nn.BatchNorm2d(C, eps=0.0)
    with torch.no_grad():
        bn.weight.copy_(scale)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(mean)
        bn.running_var.fill_(1.0)
    return bn.eval()


def bn64(y, bn):
    """BatchNorm2d(eval) in float64 from the module's parameters."""
    v = lambda t: t.detach().double().view(1, -1, 1, 1)
    return (y - v(bn.running_mean)) * (v(bn.weight) / torch.sqrt(v(bn.running_var) + bn.eps)) + v(bn.bias)


def ref64(x, w, bias, bn, res, relu, s, p):
    """conv2d (+ bias) (+ BatchNorm eval) (+ residual) (+ ReLU) in float64."""
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), s, p)
    if bn is not None:
        y = bn64(y, bn)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def ref32(x, w, bias, bn, res, relu, s, p):
    """The same in torch's fp32 CPU arithmetic."""
    y = F.conv2d(x.float(), w.float(), None if bias is None else bias.float(), s, p)
    if bn is not None:
        y = bn(y)
    if res is not None:
        y = y + res.float()
    return (F.relu(y) if relu else y).detach()


# ---- A1: exact-integer operands -------------------------------------------------------------------------
def _ints(rng, shape, lo, hi):
    return torch.from_numpy(rng.randint(lo, hi + 1, size=shape).astype(np.float32))


def _relu_base(K, var_x, relu):
    """Shift that keeps ~95 % of the outputs positive under ReLU: 1.7 standard deviations of the
    accumulator (K products of a weight in {-1, 0, 1} and an input of variance var_x)."""
    return int(math.ceil(1.7 * math.sqrt(K * var_x * 2.0 / 3.0))) if relu else 0


def _int_epilogue(rng, Cout, K, var_x, use_bn, use_bias, relu):
    """Per-channel scale in {1, 2, -1, 0.5} through a BatchNorm, or an integer bias: the epilogue's shift is
    base * |scale| + an integer in [-8, 8] (base > 0 only under ReLU, see _relu_base)."""
    base = _relu_base(K, var_x, relu)
    jitter = _ints(rng, (Cout,), -8, 8)
    if use_bn:
        scale = torch.tensor([1.0, 2.0, -1.0, 0.5])[torch.from_numpy(rng.randint(0, 4, size=(Cout,)))]
        mean = 2.0 * _ints(rng, (Cout,), -1, 1)            # even: mean * 0.5 stays an integer
        shift = base * scale.abs() + jitter
        return make_bn(scale, mean, shift + mean * scale), None
    if use_bias:
        return None, base + jitter
    return None, None


@functools.lru_cache(maxsize=None)
def int_case(cid):
    """Operands and float64 reference(s) of the A1 form of case ``cid``:
    dict(x, w, bn, bias, res, ref) -- plus, for the heads case, ``lasts``: [(w2, b2, ref_map)]."""
    c = next(k for k in CASES if k["id"] == cid)
    rng = np.random.RandomState(1000 + [k["id"] for k in CASES].index(cid))
    B, Cin, H, W, Cout, k, s, p = (c[n] for n in ("B", "Cin", "H", "W", "Cout", "k", "s", "p"))
    amp = 2 if c["kind"] == "stem" else 1                  # integer image in [-2, 2]: variance 2
    var_x = 2.0 if c["kind"] == "stem" else 2.0 / 3.0
    x = _ints(rng, (B, Cin, H, W), -amp, amp)
    w = _ints(rng, (Cout, Cin, k, k), -1, 1)
    bn, bias = _int_epilogue(rng, Cout, Cin * k * k, var_x, c["bn"], c["bias"], c["relu"])
    Ho, Wo = out_hw(c)
    res = _ints(rng, (B, Cout, Ho, Wo), -4, 4) if c["res"] else None
    d = dict(x=x, w=w, bn=bn, bias=bias, res=res, ref=ref64(x, w, bias, bn, res, c["relu"], s, p))
    if c["kind"] == "heads":
        d["lasts"] = []
        for i, co in enumerate(HEAD_COUTS):
            w2 = _ints(rng, (co, HEAD_HIDDEN, 1, 1), -1, 1)
            b2 = _ints(rng, (co,), -8, 8)
            mid = d["ref"][:, i * HEAD_HIDDEN:(i + 1) * HEAD_HIDDEN]
            d["lasts"].append((w2, b2, ref64(mid, w2, b2, None, None, False, 1, 0)))
    return d


def exactness(y):
    """The A1 condition on a float64 reference: every value an fp16 number with |y| <= 2048.
    Returns (holds, max |y|, fraction of non-zero values)."""
    ok = bool((y.abs() <= 2048).all()) and bool((y.half().double() == y).all())
    return ok, float(y.abs().max()), float((y != 0).double().mean())


def int_refs(cid):
    """Every reference tensor of the A1 form of a case, named."""
    d = int_case(cid)
    out = [("y", d["ref"])]
    for co, (_, _, r) in zip(HEAD_COUTS, d.get("lasts", ())):
        out.append(("map%d" % co, r))
    return out
