"""cn_conv2d on the raw C ABI, one call per case of tests/conv_route_cases.py: ask cn_conv2d_route (the table's answer,
now with the real pointers), run cn_conv2d once, compare with a float64 reference, check where it wrote.

Reference: torch.nn.functional.conv2d on the CPU in float64 on the float32 operands (fp16 cases: rounded to half
first), then scale, shift, residual and ReLU in float64, then the scatter.  Bars, none of them new: fp32 and f32s
|diff| <= 2e-5 * (1 + |ref|) (tests/test_gpu_conv.py); fp16 the rounding bar of tests/test_gpu_half.py,
|diff| <= 2^-11 |ref| + 2^-25 + 4 E32 for a half output and 4 E32 for a float one, E32 being the largest error of
torch's own fp32 CPU evaluation of the same operands.

Buffers: y, the residual's tensor and the workspace are filled with the sentinel NaN of tests/dcn_cases.py and stand
between guards.  After the call every cell the call does not own is still sentinel: the channels outside
[c_off, c_off + Cout) -- outside the whole 32-channel groups where the kernel's contract is zeros behind Cout (f32s
output, cn_offconv) --, the cells of the (B, OH, OW) map the scatter does not address, the guards; the residual's
tensor is unchanged; exactly `ksplit` leading workspace slabs are written whole when ksplit > 1 and nothing
otherwise.  (What "zeros behind Cout" is in the code: the persistent kernels, cn_proj and unsplit cn_offconv store whole
groups, the tile kernels, the implicit GEMM and the split's second stage leave the channels behind Cout alone, and the
plan builder zero-fills an f32s tensor once when it makes it.  So those cells hold zeros or what they held.)  y is allocated as if the scatter reached (Ho-1)*|oy_mul| + |oy_add| + 1 rows and the workspace as if
every slab had B*OH*OW rows, while the call gets the true sizes: a scatter the library mis-handles shows as a
sentinel violation inside memory the test owns."""
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from centernet_amd import native, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_route_cases as cc   # noqa: E402
from dcn_cases import TOL   # noqa: E402
from route_buffers import Buf as _Buf, pack_f32s as _pack_f32s, unpack_f32s as _unpack_f32s   # noqa: E402

pytestmark = pytest.mark.gpu
POOLED = native.CONV_STEM_MAXPOOL


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    native.lib().cn_reset_tuning()


# ---- operands and references (CPU, shared between the cases of one layer) -------------------------------------------
def _layer_key(c):
    return tuple(c[k] for k in ("B", "Cin", "H", "W", "Cout", "KH", "KW", "s", "pad_h", "pad_w", "dil", "relu")) + \
        (c["dt"] == cc.F16, bool(c["res"]), bool(c["flags"] & POOLED)) + cc.scatter(c)[4:]


@functools.lru_cache(maxsize=None)
def _operands(key):
    B, Cin, H, W, Cout, KH, KW, s, ph, pw, dil, relu, half, has_res, pooled, OH, OW = key
    rnd = (lambda t: t.half().float()) if half else (lambda t: t)
    x = rnd(torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 11)))
    w = rnd(torch.from_numpy(synth.normal((Cout, Cin, KH, KW), (2.0 / (Cin * KH * KW)) ** 0.5, 12)))
    scale = torch.from_numpy(synth.normal((Cout,), 0.2, 13)) + 1.0
    shift = torch.from_numpy(synth.normal((Cout,), 0.3, 14))
    res = rnd(torch.from_numpy(synth.normal((B, Cout, OH, OW), 1.0, 15))) if has_res else None
    conv = {}
    for name, dt in (("ref", torch.float64), ("ref32", torch.float32)):
        y = F.conv2d(x.to(dt), w.to(dt), None, s, (ph, pw), dil)
        conv[name] = y * scale.to(dt).view(1, -1, 1, 1) + shift.to(dt).view(1, -1, 1, 1)
    return dict(x=x, w=w, scale=scale, shift=shift, res=res, conv=conv)


def _reference(c):
    """(ref (B, Cout, OH, OW) float64 with NaN where the scatter writes nothing, written-pixel mask (OH, OW), E32)"""
    o = _operands(_layer_key(c))
    ym, ya, xm, xa, OH, OW = cc.scatter(c)
    ho, wo = cc.out_hw(c)
    ys, xs = slice(ya, ya + ym * ho, ym), slice(xa, xa + xm * wo, xm)
    out = {}
    for name, y in o["conv"].items():
        if o["res"] is not None:
            y = y + o["res"].to(y.dtype)[:, :, ys, xs]
        if c["relu"]:
            y = F.relu(y)
        if c["flags"] & POOLED:
            y = F.max_pool2d(y, 3, 2, 1)
        out[name] = y
    if c["flags"] & POOLED:
        return out["ref"], torch.ones(out["ref"].shape[2:], dtype=torch.bool), 0.0
    ref = torch.full((c["B"], c["Cout"], OH, OW), float("nan"), dtype=torch.float64)
    ref[:, :, ys, xs] = out["ref"]
    mask = torch.zeros((OH, OW), dtype=torch.bool)
    mask[ys, xs] = True
    return ref, mask, float((out["ref32"].double() - out["ref"]).abs().max())


class _Call:
    """One case on the device: operands uploaded in the case's formats, y / residual / workspace as sentinel buffers"""

    def __init__(self, dev, c, y=None):
        self.dev, self.c, self.lib = dev, c, native.lib()
        o = _operands(_layer_key(c))
        B, Cout = c["B"], c["Cout"]
        self.ho, self.wo = cc.out_hw(c)
        ym, ya, xm, xa, OH, OW = cc.scatter(c)
        self.pooled = bool(c["flags"] & POOLED)
        if self.pooled:
            OH, OW = self.ho // 2, self.wo // 2
        self.OH, self.OW = OH, OW
        self.ip, self.op, self.rp = cc.pitches(c)
        half = c["dt"] == cc.F16
        # x
        if c["stem"]:
            self.x = o["x"].contiguous().to(dev)
        else:
            x = o["x"].permute(0, 2, 3, 1).contiguous()
            if cc.packed_in(c):
                x = _pack_f32s(F.pad(x, (0, self.ip - c["Cin"])))
            self.x = x.to(device=dev, dtype=torch.float16 if half else torch.float32)
        # weight, scale, shift
        w, scale = o["w"], o["scale"]
        cd = cc.DTYPES[c["dt"]]
        if c["dt"] == cc.F32S or c["flags"] & native.CONV_STEM_F32S:
            from centernet_amd.engine import prescale_rows
            w, factor = prescale_rows(w)
            scale = scale * factor
        w = w.contiguous().to(dev)
        n = self.lib.cn_packed_conv_weight_elems(Cout, c["Cin"], c["KH"], c["KW"], cd)
        self.wp = torch.zeros(n, device=dev, dtype=torch.float32)
        native.check(self.lib.cn_pack_conv_weight(native.ptr(w), native.ptr(self.wp), Cout, c["Cin"], c["KH"], c["KW"],
                                                  cd, native.stream_ptr()), "cn_pack_conv_weight")
        self.scale, self.shift = scale.contiguous().to(dev), o["shift"].to(dev)
        # y: as if the scatter reached where a wrong one could
        self.OHa = max(OH, (self.ho - 1) * abs(ym) + abs(ya) + 1) if not self.pooled else OH
        self.OWa = max(OW, (self.wo - 1) * abs(xm) + abs(xa) + 1) if not self.pooled else OW
        self.ye = cc.elem_bytes(c, "y")
        pix = B * self.OHa * self.OWa
        self.yn = pix * (Cout if c["nchw"] else self.op)
        self.y = y if y is not None else _Buf(dev, self.yn, self.ye, 2 * (self.OWa + 2) * max(self.op, Cout) + 1024)
        # residual: a (B, OH, OW, rp) tensor, the call's channels at res_off
        self.res = None
        if c["res"]:
            r = o["res"].permute(0, 2, 3, 1).contiguous()
            width = cc.r32(Cout) if cc.packed_res(c) else Cout
            assert c["res_off"] + width <= self.rp
            self.res = _Buf(dev, B * OH * OW * self.rp, cc.elem_bytes(c, "res"), 1024)
            if cc.packed_res(c):
                r = _pack_f32s(F.pad(r, (0, width - Cout)))
            r = r.to(device=dev, dtype=torch.float16 if half else torch.float32)
            rv = self.res.values("f16" if half else "f32").view(B, OH, OW, self.rp)
            rv[..., c["res_off"]:c["res_off"] + width] = r
            self.res_before = self.res.t.clone()
        # workspace: the queried bytes are passed, but it is owned as if every slab had B*OH*OW rows
        self.need = cc.workspace_bytes(c)
        self.cout_pad = cc.r32(Cout)
        self.slab = B * self.ho * self.wo * self.cout_pad
        self.ws = None
        if c["ws"]:
            slabs = max(self.need // (4 * self.slab), 16 if c["scatter"] else 1)
            self.ws = _Buf(dev, slabs * B * self.OHa * self.OWa * self.cout_pad, 4, 4096)
        torch.cuda.synchronize()

    def _args(self):
        c, vp = self.c, ctypes.c_void_p
        self.d = cc.desc(c)
        return (ctypes.byref(self.d), vp(self.x.data_ptr()), vp(self.wp.data_ptr()), vp(self.scale.data_ptr()),
                vp(self.shift.data_ptr()), vp(self.res.ptr(c["res_off"])) if self.res else None,
                vp(self.y.ptr(c["c_off"])), vp(self.ws.ptr()) if self.ws else None, self.need if self.ws else 0)

    def query(self):
        info = native.ConvRouteInfo()
        with native.tuning(self.c["keys"]):
            rc = self.lib.cn_conv2d_route(*self._args(), None, ctypes.byref(info))
        return rc, info

    def run(self):
        with native.tuning(self.c["keys"]):
            rc = self.lib.cn_conv2d(*self._args(), native.stream_ptr())
            torch.cuda.synchronize()
        return rc

    # ---- what the call owns in y.  Unit: an element of y -- for an f32s tensor a half, since a channel is one
    # fp16 high part and one low part, 32 halves apart in its group of 64
    def units(self, t=None):
        t = self.y.body if t is None else t
        return t.view(torch.int16) if cc.packed_out(self.c) else t

    def owned(self, pixel_mask):
        """(own, pad): masks over units() -- the channels [c_off, c_off + Cout) of the pixels the scatter addresses,
        and the channels behind Cout in the last 32-channel group where the output has such groups (an f32s tensor,
        cn_offconv's block): a kernel may fill those with zeros or leave them"""
        c = self.c
        B, Cout = c["B"], c["Cout"]
        packed = cc.packed_out(c)
        n = self.yn * (2 if packed else 1)
        own = torch.zeros(n, dtype=torch.bool, device=self.dev)
        pad = torch.zeros(n, dtype=torch.bool, device=self.dev)
        pm = pixel_mask.to(self.dev)
        if c["nchw"]:
            v = own.view(B, Cout, self.OHa, self.OWa)
            v[:, :, :self.OH, :self.OW] = pm
            return own, pad
        assert (self.OHa, self.OWa) == (self.OH, self.OW)
        # the kernel addresses pixel (b, oy, ox) at ((b*OH + oy)*OW + ox) * pitch from the pointer
        pm = pm.view(1, self.OH, self.OW, 1)
        if packed:
            assert c["c_off"] % 32 == 0
            vo = own.view(B, self.OH, self.OW, self.op // 32, 2, 32)
            vp = pad.view(B, self.OH, self.OW, self.op // 32, 2, 32)
            g0 = c["c_off"] // 32
            for g in range(cc.r32(Cout) // 32):
                k = min(Cout - 32 * g, 32)
                vo[..., g0 + g, :, :k] = pm.unsqueeze(-1)
                vp[..., g0 + g, :, k:] = pm.unsqueeze(-1)
            return own, pad
        vo = own.view(B, self.OH, self.OW, self.op)
        vo[..., c["c_off"]:c["c_off"] + Cout] = pm
        if c["route"] == "offconv":
            pad.view(B, self.OH, self.OW, self.op)[..., c["c_off"] + Cout:c["c_off"] + cc.r32(Cout)] = pm
        return own, pad

    def output(self):
        """values (B, Cout, OH, OW) float64 on the CPU"""
        c = self.c
        B, Cout = c["B"], c["Cout"]
        fmt = "f16" if self.ye == 2 else "f32"
        if c["nchw"]:
            return self.y.values(fmt).view(B, Cout, self.OHa, self.OWa)[:, :, :self.OH, :self.OW].double().cpu()
        v = self.y.values(fmt)[:B * self.OH * self.OW * self.op].view(B, self.OH, self.OW, self.op)
        if cc.packed_out(c):
            v = _unpack_f32s(v[..., c["c_off"]:c["c_off"] + cc.r32(Cout)].contiguous())[..., :Cout]
        else:
            v = v[..., c["c_off"]:c["c_off"] + Cout]
        return v.double().cpu().permute(0, 3, 1, 2)

    def slabs_written(self):
        """_Layer.slabs_written of tests/dcn_cases.py: leading slabs written whole, nothing else touched"""
        ws = self.ws.body
        n = ws.numel() // self.slab
        touched = [bool((~self.ws.is_sentinel(ws[k * self.slab:(k + 1) * self.slab])).any()) for k in range(n)]
        whole = [not bool(self.ws.is_sentinel(ws[k * self.slab:(k + 1) * self.slab]).any()) for k in range(n)]
        assert touched == whole, ("a partly written slab", touched, whole)
        k = sum(touched)
        assert touched == [True] * k + [False] * (n - k), touched
        assert bool(self.ws.is_sentinel(ws[n * self.slab:]).all())
        return k


def _compare(c, got, ref, mask, e32, fp16_out, what):
    sel = mask.view(1, 1, *mask.shape).expand_as(ref)
    g, r = got[sel], ref[sel]
    assert not bool(torch.isnan(r).any())
    err = (g - r).abs()
    if c["dt"] == cc.F16:
        bar = 4.0 * e32 + ((r.abs() * 2.0 ** -11 + 2.0 ** -25) if fp16_out else 0.0)
        assert e32 > 0
    else:
        bar = TOL * (1 + r.abs())
    over = ~(err <= bar)            # a NaN (an unwritten cell) is over the bar
    print("%s %s: max |err| %.3e, max err / bar %.3f" % (c["id"], what, float(err.max()), float((err / bar).max())))
    assert not bool(over.any()), "%s %s: %d of %d values beyond the bar, max |err| %.3e (NaN: %d)" % (
        c["id"], what, int(over.sum()), over.numel(), float(err[~torch.isnan(err)].max()), int(torch.isnan(g).sum()))


def _check_call(call, info, ref, mask, e32, before=None):
    """where the call wrote, then the values"""
    c = call.c
    own, pad = call.owned(mask)
    body = call.units()
    fresh = call.units(torch.full_like(call.y.body, call.y.sent))
    # outside its own cells the call changed nothing (before: a map shared by several calls) ...
    same = body == (fresh if before is None else call.units(before))
    assert bool(same[~own & ~pad].all()), "%s: %d cells outside the call's own were written" % (
        c["id"], int((~same[~own & ~pad]).sum()))
    # ... but for the channels behind Cout of a 32-channel group, which it may zero
    assert bool((same | (body == 0))[pad].all()), "%s: channels behind Cout hold neither zeros nor what they held" % c["id"]
    if not cc.packed_out(c):      # (halves of an f32s tensor: an unwritten cell fails the comparison below)
        assert not bool(call.y.is_sentinel(body)[own].any()), "%s: %d of the call's cells were not written" % (
            c["id"], int(call.y.is_sentinel(body)[own].sum()))
    assert call.y.guards_untouched(), c["id"]
    if call.res:
        assert torch.equal(call.res.t, call.res_before), c["id"]
    if call.ws:
        assert call.ws.guards_untouched(), c["id"]
        assert call.slabs_written() == (info.ksplit if info.ksplit > 1 else 0), c["id"]
    _compare(c, call.output(), ref, mask, e32, call.ye == 2, "y")


SINGLE = [c for c in cc.CASES if c["rc"] == cc.OK and not c["id"].startswith("scatter2_")]
PARITY = sorted({c["id"][:-4] for c in cc.CASES if c["id"].startswith("scatter2_")})
REFUSED = [c for c in cc.CASES if c["rc"] != cc.OK]


@pytest.mark.parametrize("cid", [c["id"] for c in SINGLE])
def test_the_routed_kernel_computes_the_reference(dev, cid):
    c = cc.BY_ID[cid]
    call = _Call(dev, c)
    rc, info = call.query()
    assert cc.said(rc, info) == cc.expected(c)
    ref, mask, e32 = _reference(c)
    assert call.run() == cc.OK
    _check_call(call, info, ref, mask, e32)


@pytest.mark.parametrize("group", PARITY)
def test_four_parity_scatters_fill_one_map(dev, group):
    """oy_mul = ox_mul = 2 with the four (oy_add, ox_add) into ONE (B, 2H, 2W) map: each call writes its parity class
    and nothing else, the four together every cell exactly once"""
    cases = [cc.BY_ID["%s_p%d%d" % (group, py, px)] for py in (0, 1) for px in (0, 1)]
    y, total = None, None
    for c in cases:
        call = _Call(dev, c, y=y)
        y = call.y
        rc, info = call.query()
        assert cc.said(rc, info) == cc.expected(c)
        ref, mask, e32 = _reference(c)
        before = y.body.clone()
        own = call.owned(mask)[0]
        fresh = call.units(torch.full_like(before, y.sent))
        assert bool((call.units(before) == fresh)[own].all()), "a cell would be written twice"
        assert call.run() == cc.OK
        _check_call(call, info, ref, mask, e32, before=before)
        total = mask if total is None else (total ^ mask)
    assert bool(total.all())


@pytest.mark.parametrize("cid", [c["id"] for c in REFUSED])
def test_a_scatter_that_leaves_the_map_is_refused(dev, cid):
    """CN_ERR_SHAPE from cn_conv2d, from cn_conv2d_route and (as 0 bytes) from the workspace query; nothing is
    launched: y and the workspace stay all sentinel"""
    c = cc.BY_ID[cid]
    call = _Call(dev, c)
    assert call.need == 0
    rc, info = call.query()
    assert (rc, info.route, info.ksplit) == (cc.ERR_SHAPE, native.ROUTE_NONE, 0)
    assert call.run() == cc.ERR_SHAPE
    assert bool(call.y.is_sentinel(call.y.t).all())
    assert bool(call.ws.is_sentinel(call.ws.t).all())


def test_a_wanted_split_given_or_not_is_the_same_layer(dev):
    """the same layer with and without the workspace its split wants: both within the bar of one reference (each in
    test_the_routed_kernel_computes_the_reference), and of each other by twice the bar"""
    got = {}
    for cid in ("igemm_split_given_s2_f32", "igemm_split_not_given_s2_f32"):
        call = _Call(dev, cc.BY_ID[cid])
        rc, info = call.query()
        assert rc == cc.OK and (info.ksplit > 1) == cc.BY_ID[cid]["ws"] and info.want > 1
        assert call.run() == cc.OK
        got[cid] = call.output()
    a, b = got.values()
    assert bool(((a - b).abs() <= 2 * TOL * (1 + a.abs())).all())
