"""Case list, schedule mirror, operand builders and float64 references shared by
tests/test_gpu_c3p_items.py (GPU) and tests/test_c3p_cases_host.py (CPU).  Not a test module.

The persistent 3x3 kernel (csrc/cn_conv3x3p.hip) walks a list of items -- (pixel tile 8 x 16, parity, 64-channel
output block) -- per workgroup.  Its launchers size the grid as 8 * min(ceil(items / 8), key 47), so at the
default cap of 64 a launch of up to 512 items gives every workgroup ONE item and the code at an item boundary
(halo cursor, weight block, parity, halo buffer and ring slot parities, the strips that alias a halo buffer) is
never executed at a shape whose reference is cheap.  The cases below are run at caps 64, 3 and 1.

A case is a dict: ``id``; ``form`` ("s1", "s2", "deconv", "heads"); B, Cin, H, W (the INPUT map) and Cout, or
``heads``: [(name, outputs, has bias)] for the fused heads (hidden width 64); ``keys``: cn_set_tuning keys the
case needs besides 28 = 2 and 47 = cap.  The 3x3 / s1 cases run with key 5 = 1 (never split K): at these map
sizes conv_route (csrc/cn_conv.hip) would hand every layer of 18 or more (tap, chunk) steps to the split-K
implicit GEMM, and the persistent kernel would not run at all.

The mirror (``p3_args``, ``grid``, ``p3_decode``, ``workgroup_items``) restates the item arithmetic of
cn_conv3x3p.hip in plain Python: p3_args() of the launchers, the capped grid, and the kernel's per / lo / hi /
first / nit and p3_decode.
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from half_cases import bn64   # noqa: E402

TH, TW = 8, 16                     # P_TH, P_TW: output pixels per tile
NTAP = {"s1": 9, "s2": 9, "deconv": 4, "heads": 9}
CAPS = (64, 3, 1)
HIDDEN = 64
NOSPLIT = {5: 1}


def _c(id, form, shape, keys=None, heads=None):
    B, Cin, H, W, Cout = shape
    return dict(id=id, form=form, B=B, Cin=Cin, H=H, W=W, Cout=Cout, keys=dict(keys or {}), heads=heads)


CASES = [
    # 54 items, nchunk 3: cap 1 gives nit 7 and 5, 27 steps per item (ring phase 3), 96 = a half-empty second block
    _c("s1_96_20x40", "s1", (3, 96, 20, 40, 96), NOSPLIT),
    # 18 items, nchunk 1: nit 3, XCDs 6 and 7 empty; an item's strips and the next item's halo in ONE buffer
    _c("s1_32_17x33", "s1", (2, 32, 17, 33, 64), NOSPLIT),
    # 16 items, nchunk 2: consecutive items are the same tile with the next output block (four blocks)
    _c("s1_64_16x32", "s1", (1, 64, 16, 32, 256), NOSPLIT),
    # 15 items, nchunk 1: item pairs cross an image; 32 outputs = a half-empty single block
    _c("s1_32_24x16", "s1", (5, 32, 24, 16, 32), NOSPLIT),
    # 96 items, nchunk 3: nit 12; parity, block, tile row and image change inside a workgroup
    _c("deconv_96_9x20", "deconv", (3, 96, 9, 20, 96)),
    # 12 items, nchunk 1: four steps per item, the halo buffer alternates item by item
    _c("deconv_32_8x40", "deconv", (1, 32, 8, 40, 64)),
    # 36 items, nchunk 1, odd map (18 x 23 outputs): nit 5 ... 1 -- dla_34's 32 -> 64 form
    _c("s2_32_35x45", "s2", (3, 32, 35, 45, 96)),
    _c("s2_96_32x64", "s2", (3, 96, 32, 64, 128)),                      # 24 items, nchunk 3
    # 36 items, nchunk 2: the head changes item to item
    _c("heads_64_20x24", "heads", (2, 64, 20, 24, 0), heads=[("hm", 80, True), ("wh", 2, True), ("reg", 2, True)]),
    _c("heads_96_17x40", "heads", (1, 96, 17, 40, 0),                   # 45 items, nchunk 3
       heads=[("hm", 33, True), ("nobias", 96, False), ("a", 1, True), ("b", 64, True), ("c", 5, True)]),
    _c("heads_32_16x32", "heads", (3, 32, 16, 32, 0), heads=[("hm", 3, True), ("wh", 2, True)]),   # 24 items, nchunk 1
]
FORMS = ("s1", "deconv", "s2", "heads")


def case(cid):
    return next(c for c in CASES if c["id"] == cid)


def variants(c):
    """(residual format, plain output) of every instantiation a case runs: residual None / "f32s" / "plain"."""
    if c["form"] == "s1":
        return [(r, p) for r in (None, "f32s", "plain") for p in (False, True)]
    if c["form"] == "heads":
        return [(None, True)]          # fp32 NCHW maps
    return [(None, False), (None, True)]


# ---- the schedule mirror -------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def out_hw(c):
    if c["form"] == "s2":
        return (c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1
    if c["form"] == "deconv":
        return 2 * c["H"], 2 * c["W"]
    return c["H"], c["W"]


def p3_args(c):
    """items, nblk, npar, tiles_x, tiles_y, nchunk as p3_args / cn_heads3x3p fill them.  The tiles cover the
    output map; for the transposed form the input map (= the output in units of its four parity classes)."""
    H, W = (c["H"], c["W"]) if c["form"] == "deconv" else out_hw(c)
    npar = 4 if c["form"] == "deconv" else 1
    nblk = len(c["heads"]) if c["form"] == "heads" else cdiv(c["Cout"], 64)
    a = dict(H=H, W=W, npar=npar, nblk=nblk, nchunk=cdiv(c["Cin"], 32), tiles_x=cdiv(W, TW), tiles_y=cdiv(H, TH))
    a["items"] = c["B"] * a["tiles_y"] * a["tiles_x"] * npar * nblk
    return a


def grid(a, cap):
    """Workgroups of a launch: 8 * min(ceil(items / 8), cap) (p3_grid)."""
    return 8 * min(cdiv(a["items"], 8), cap)


def p3_decode(a, item):
    """item -> dict(b, ty, tx, nb, par): output block fastest, then parity, tile column, tile row, image."""
    nb = item % a["nblk"]
    t = item // a["nblk"]
    par = t % a["npar"]
    t //= a["npar"]
    tx = t % a["tiles_x"]
    t //= a["tiles_x"]
    return dict(b=t // a["tiles_y"], ty=t % a["tiles_y"], tx=tx, nb=nb, par=par)


def workgroup_items(a, cap):
    """The item list of every workgroup of a launch, in the order it walks them: XCD x = id % 8 owns the
    contiguous range [x * per, x * per + per), its workgroups take every nx-th item of it."""
    g = grid(a, cap)
    nx, per = g >> 3, (a["items"] + 7) >> 3
    out = []
    for wg in range(g):
        xcd, jx = wg & 7, wg >> 3
        lo = xcd * per
        hi = min(lo + per, a["items"])
        first = lo + jx
        nit = (hi - first + nx - 1) // nx if first < hi else 0
        out.append([first + k * nx for k in range(nit)])
    return out


def steps_per_item(c):
    return NTAP[c["form"]] * p3_args(c)["nchunk"]


def pitches(c, res, out_plain):
    """(in, out, residual) pixel pitches in elements: an f32s tensor is padded to whole 32-channel groups."""
    r32 = lambda n: cdiv(n, 32) * 32
    out = c["Cout"] if out_plain else r32(c["Cout"])
    return r32(c["Cin"]), out, {None: 0, "f32s": r32(c["Cout"]), "plain": c["Cout"]}[res]


def takes(c, res=None, out_plain=False):
    """The conditions of cn_conv3x3p_takes / cn_conv3x3s2p_takes / cn_deconv4x4s2p_takes / cn_heads3x3p_takes
    (with key 28 = 2: no lower bound on the items) and of the route that leads there."""
    B, H, W = c["B"], c["H"], c["W"]
    Ho, Wo = out_hw(c)
    ip, op, rp = pitches(c, res, out_plain)
    if c["form"] == "heads":
        return (ip % 32 == 0 and len(c["heads"]) <= 8 and all(co <= 96 for _, co, _ in c["heads"]) and
                B * H * W * ip * 4 < 2 ** 31 and all(B * co * H * W < 2 ** 31 for _, co, _ in c["heads"]))
    if ip % 32 or op % 32 or rp % 32 or c["Cout"] % 32:
        return False
    if c["form"] == "s1":       # conv_route: the halo route only without a K split (KT < 16 or key 5 = 1)
        return (B * H * W * max(ip, op, rp) * 4 < 2 ** 31 and
                (9 * p3_args(c)["nchunk"] < 16 or c["keys"].get(5) == 1))
    if c["form"] == "s2":
        return res is None and B * H * W * ip * 4 < 2 ** 31 and B * Ho * Wo * op * 4 < 2 ** 31
    return res is None and c["Cout"] > 32 and 4 * B * H * W * max(ip, op) * 4 < 2 ** 31


# ---- operands and float64 references -------------------------------------------------------------------------
def _ints(rng, shape, lo, hi):
    return torch.from_numpy(rng.randint(lo, hi + 1, size=shape).astype(np.float32))


def _ternary(rng, shape, p_plus=1.0 / 3):
    """Weights in {-1, 0, 1} (P(1) = p_plus, P(-1) = P(0)), no all-zero output row (dim 0)."""
    u = rng.random_sample(shape)
    q = (1.0 - p_plus) / 2
    w = torch.from_numpy(np.where(u < q, -1.0, np.where(u < 2 * q, 0.0, 1.0)).astype(np.float32))
    w.view(shape[0], -1)[:, 0] = 1.0
    return w


def _bias(rng, n, K):
    """Integer bias that keeps most outputs positive under ReLU: 1.7 standard deviations of the accumulator
    (K products of a weight in {-1, 0, 1} and an input in 0 ... 3: variance 3.5 * 2 / 3 each) + (-8 ... 8)."""
    return float(np.ceil(1.7 * np.sqrt(K * 7.0 / 3.0))) + _ints(rng, (n,), -8, 8)


def _head_modules(c, rng=None, seed=0):
    """name -> (Conv2d 3x3 Fc -> 64 with bias, Conv2d 1x1 64 -> outputs): integer weights from ``rng``, or the
    recipe of test_gpu_conv._heads_case from ``seed``."""
    from centernet_amd import synth
    Fc, pairs = c["Cin"], {}
    for i, (name, co, has_bias) in enumerate(c["heads"]):
        c1 = torch.nn.Conv2d(Fc, HIDDEN, 3, padding=1, bias=True)
        c2 = torch.nn.Conv2d(HIDDEN, co, 1, bias=has_bias)
        with torch.no_grad():
            if rng is not None:
                c1.weight.copy_(_ternary(rng, (HIDDEN, Fc, 3, 3)))
                c1.bias.copy_(_bias(rng, HIDDEN, Fc * 9))
                w2 = _ints(rng, (co, HIDDEN, 1, 1), -2, 2)
                w2[:, 0] = 1.0
                c2.weight.copy_(w2)
                if has_bias:
                    c2.bias.copy_(_ints(rng, (co,), -8, 8))
            else:
                c1.weight.copy_(torch.from_numpy(synth.normal(tuple(c1.weight.shape), (2.0 / (Fc * 9)) ** 0.5, seed + 20 + i)))
                c1.bias.copy_(torch.from_numpy(synth.normal((HIDDEN,), 0.2, seed + 30 + i)))
                c2.weight.copy_(torch.from_numpy(synth.normal(tuple(c2.weight.shape), 0.15, seed + 40 + i)))
                if has_bias:
                    c2.bias.copy_(torch.from_numpy(synth.normal((co,), 0.5, seed + 50 + i)))
        pairs[name] = (c1.eval(), c2.eval())
    return pairs


def _head_refs(x, pairs):
    """name -> (hidden, map) in float64."""
    out = {}
    for n, (c1, c2) in pairs.items():
        hid = F.relu(F.conv2d(x.double(), c1.weight.detach().double(), c1.bias.detach().double(), 1, 1))
        b2 = None if c2.bias is None else c2.bias.detach().double()
        out[n] = (hid, F.conv2d(hid, c2.weight.detach().double(), b2))
    return out


def _conv64(c, x, w):
    if c["form"] == "deconv":
        return F.conv_transpose2d(x.double(), w.double(), None, 2, 1, 0)
    return F.conv2d(x.double(), w.double(), None, 2 if c["form"] == "s2" else 1, 1)


def _finish(c, d, y):
    """ref[residual?]: ReLU(y (+ residual)) in float64, (B, Cout, Ho, Wo)."""
    d["ref"] = {False: F.relu(y)}
    if d["res"] is not None:
        d["ref"][True] = F.relu(y + d["res"].double())
    return d


@functools.lru_cache(maxsize=None)
def int_case(cid):
    """Exact-integer operands: x in 0 ... 3, weights in {-1, 0, 1}, integer bias (none for the transposed
    form, whose builder takes none: more of its weights are +1 instead), no BN, residual in -8 ... 8, ReLU.
    dict(x, w, bias, bn=None, res, ref) -- heads: dict(x, pairs, refs: name -> (hidden, map))."""
    c = case(cid)
    rng = np.random.RandomState(4700 + [k["id"] for k in CASES].index(cid))
    x = _ints(rng, (c["B"], c["Cin"], c["H"], c["W"]), 0, 3)
    if c["form"] == "heads":
        pairs = _head_modules(c, rng=rng)
        return dict(x=x, pairs=pairs, refs=_head_refs(x, pairs))
    Ho, Wo = out_hw(c)
    if c["form"] == "deconv":
        w = _ternary(rng, (c["Cout"], c["Cin"], 4, 4), p_plus=0.4).transpose(0, 1).contiguous()   # (Cin, Cout, 4, 4)
        bias = None
    else:
        w = _ternary(rng, (c["Cout"], c["Cin"], 3, 3))
        bias = _bias(rng, c["Cout"], c["Cin"] * 9)
    res = _ints(rng, (c["B"], c["Cout"], Ho, Wo), -8, 8) if c["form"] == "s1" else None
    d = dict(x=x, w=w, bias=bias, bn=None, res=res)
    y = _conv64(c, x, w)
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    return _finish(c, d, y)


@functools.lru_cache(maxsize=None)
def normal_case(cid):
    """Normal data with a folded BatchNorm, by the recipes of test_gpu_conv._conv_case / _deconv_case / the fused
    heads test: same keys as ``int_case``."""
    from centernet_amd import synth
    c = case(cid)
    B, Cin, H, W, Cout = (c[k] for k in ("B", "Cin", "H", "W", "Cout"))
    if c["form"] == "heads":
        x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 11)).relu_()
        pairs = _head_modules(c, seed=B + H)
        return dict(x=x, pairs=pairs, refs=_head_refs(x, pairs))
    x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 1))
    if c["form"] == "deconv":
        w = torch.from_numpy(synth.normal((Cin, Cout, 4, 4), (2.0 / (Cin * 4)) ** 0.5, 2))
    else:
        w = torch.from_numpy(synth.normal((Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, 2))
    bn = torch.nn.BatchNorm2d(Cout)
    synth.fill_state_dict_(bn, 3 if c["form"] == "deconv" else 4)
    bn = bn.eval()
    Ho, Wo = out_hw(c)
    res = torch.from_numpy(synth.normal((B, Cout, Ho, Wo), 1.0, 5)) if c["form"] == "s1" else None
    d = dict(x=x, w=w, bias=None, bn=bn, res=res)
    return _finish(c, d, bn64(_conv64(c, x, w), bn))


def data(cid, kind):
    return int_case(cid) if kind == "int" else normal_case(cid)


# ---- the exactness condition of the integer cases ----------------------------------------------------------------
def _fp16_exact(t):
    return bool(torch.equal(t.half().float(), t.float()))


def int_exactness(cid):
    """What the bit comparison of the integer cases rests on, from the case's own operands in float64:
    dict(sum_abs: largest sum |x * w| over K of any output (second layer of the heads included), top: largest
    stored magnitude (outputs with and without the residual, hidden layer), operands_exact: x, residual and every
    weight -- as given and after prescale_rows -- are fp16 numbers and the biases integers, rows_nonzero,
    nonzero: fraction of non-zero reference values)."""
    from centernet_amd.engine import prescale_rows
    c, d = case(cid), int_case(cid)
    x = d["x"]
    if c["form"] == "heads":
        sum_abs, top, exact, rows, nz = 0.0, 0.0, _fp16_exact(x), True, []
        for n, (c1, c2) in d["pairs"].items():
            hid, ref = d["refs"][n]
            w1, w2 = c1.weight.detach(), c2.weight.detach()
            s1 = F.conv2d(x.double().abs(), w1.double().abs(), None, 1, 1)
            s2 = F.conv2d(hid.abs(), w2.double().abs())
            sum_abs = max(sum_abs, float(s1.max()), float(s2.max()))
            top = max(top, float(hid.abs().max()), float(ref.abs().max()))
            biases = [c1.bias.detach()] + ([] if c2.bias is None else [c2.bias.detach()])
            exact = exact and all(_fp16_exact(t) and _fp16_exact(prescale_rows(t.flatten(1))[0]) for t in (w1, w2)) \
                and all(bool(torch.equal(b, b.round())) for b in biases)
            rows = rows and all(bool((t.flatten(1).abs().amax(1) > 0).all()) for t in (w1, w2))
            nz.append(float((ref != 0).double().mean()))
        return dict(sum_abs=sum_abs, top=top, operands_exact=exact, rows_nonzero=rows, nonzero=min(nz))
    w = d["w"]
    s = _conv64(c, x.abs(), w.abs())
    rows_first = w.transpose(0, 1).contiguous() if c["form"] == "deconv" else w       # (Cout, ...)
    exact = all(_fp16_exact(t) for t in (x, w, prescale_rows(rows_first)[0]))
    if d["res"] is not None:
        exact = exact and _fp16_exact(d["res"])
    if d["bias"] is not None:
        exact = exact and bool(torch.equal(d["bias"], d["bias"].round()))
        s = s + d["bias"].double().abs().view(1, -1, 1, 1)
    if d["res"] is not None:
        s = s + d["res"].double().abs()
    return dict(sum_abs=float(s.max()), top=max(float(r.abs().max()) for r in d["ref"].values()),
                operands_exact=exact, rows_nonzero=bool((rows_first.flatten(1).abs().amax(1) > 0).all()),
                nonzero=min(float((r != 0).double().mean()) for r in d["ref"].values()))
