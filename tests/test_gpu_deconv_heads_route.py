"""cn_conv_transpose4x4s2 and cn_heads3x3_1x1 on the raw C ABI, one call per case of tests/deconv_route_cases.py and
tests/heads_route_cases.py: ask the route query (the table's answer, now with the real pointers), run once, compare
with a float64 reference, check where the call wrote.

References (CPU, float64, on the float32 operands; fp16 cases: rounded to half first): the deconvolution is
F.conv_transpose2d(x, w, None, 2, 1), then scale, shift and ReLU; a head is conv1x1(relu(conv3x3(x) + b1)) + b2 with
F.conv2d.  The library gets its weights the way the engine prepares them (prescale_rows, the factors in the scale or
in oscale, cn_pack_head_w2_f32s); the reference sees the original weights only.

Bars, none of them new: fp32 and f32s |diff| <= 2e-5 * (1 + |ref|) (TOL of tests/dcn_cases.py); fp16 the rounding
bar of tests/test_gpu_half.py, |diff| <= 2^-11 |ref| + 2^-25 + 4 E32, E32 being the largest error of torch's own
fp32 CPU evaluation of the same operands (asserted positive).  The `exact` cases run a second time on small-integer
operands (tests/dcn_half_cases.py deconv_int_case, tests/c3p_cases.py) and must equal float64: a dropped tap, a
swapped parity class or a wrong K chunk cannot hide under a rounding bar.

Buffers: x, y (a tensor of out_pitch channels per pixel, the call's channels at c_off) and every head's map stand
between guards, y and the maps sentinel-filled.  Afterwards every cell outside the call's own is still sentinel, the
channels behind Cout of an f32s output's last 32-channel group hold zeros or what they held, every owned cell of a
plain or half output and of a head's map was written, the guards are untouched and x is unchanged.  The pad
channels of x (in_pitch > Cin) hold finite values of another tensor; x's guards hold NaN, so a read past the tensor
shows in the values."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centernet_amd import native, synth
from centernet_amd.engine import prescale_rows

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deconv_route_cases as dc   # noqa: E402
import heads_route_cases as hc    # noqa: E402
from dcn_cases import TOL   # noqa: E402
from route_buffers import Buf, pack_f32s, unpack_f32s   # noqa: E402

pytestmark = pytest.mark.gpu
FOREIGN = 3.0          # what the channels of x that belong to another tensor hold


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    native.lib().cn_reset_tuning()


def _ints(rng, shape, lo, hi):
    return torch.from_numpy(rng.randint(lo, hi + 1, size=shape).astype(np.float32))


def _upload_x(dev, x_nchw, Cin, ip, packed, half):
    """x as the (B, H, W, ip) tensor the call reads, between NaN guards -> (Buf, its content before the call)"""
    x = x_nchw.permute(0, 2, 3, 1).contiguous()
    full = torch.full(x.shape[:3] + (ip,), FOREIGN)
    full[..., :Cin] = x
    if packed and ip % 32 == 0:                   # (a pitch the call refuses: nothing reads the tensor)
        full[..., Cin:dc.r32(Cin)] = 0.0          # the format's own padding; whole foreign groups behind it
        full = pack_f32s(full)
    buf = Buf(dev, full.numel(), 2 if half else 4, 4096)
    buf.values("f16" if half else "f32").copy_(full.reshape(-1).to(torch.float16 if half else torch.float32))
    return buf, buf.t.clone()


def _padded(dev, t, n):
    """a per-channel vector in a buffer of n >= len floats (ones behind it)"""
    out = torch.ones(n, dtype=torch.float32)
    out[:t.numel()] = t
    return out.to(dev)


def _assert_close(cid, what, got, ref, half, e32):
    assert not bool(torch.isnan(ref).any())
    err = (got - ref).abs()
    if half:
        assert e32 > 0
        bar = 4.0 * e32 + ref.abs() * 2.0 ** -11 + 2.0 ** -25
    else:
        bar = TOL * (1 + ref.abs())
    over = ~(err <= bar)            # a NaN (an unwritten cell) is over the bar
    print("%s %s: max |err| %.3e, max err / bar %.3f" % (cid, what, float(err.max()), float((err / bar).max())))
    assert not bool(over.any()), "%s %s: %d of %d values beyond the bar, max |err| %.3e (NaN: %d)" % (
        cid, what, int(over.sum()), over.numel(), float(err[~torch.isnan(err)].max()), int(torch.isnan(got).sum()))


def _assert_exact(cid, what, got, ref):
    bad = ~(got == ref)
    assert not bool(bad.any()), "%s %s (integer operands): %d of %d values differ, first at %s: %r != %r" % (
        cid, what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(ref[bad][0]))


# ---- the deconvolution ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deconv_operands(B, Cin, H, W, Cout, half, relu, has_scale, ints, x_hi):
    """operands (float32, CPU) and references of one layer, shared by the cases on it"""
    if ints:
        rng = np.random.RandomState(B * 1000 + Cin + 7 * Cout)
        x = _ints(rng, (B, Cin, H, W), 0 if x_hi > 1 else -1, x_hi)
        w = _ints(rng, (Cin, Cout, 4, 4), -1, 1)
        scale = torch.tensor([1.0, 2.0, -1.0, 0.5])[torch.from_numpy(rng.randint(0, 4, size=Cout))]
        shift = _ints(rng, (Cout,), -3, 3)
    else:
        rnd = (lambda t: t.half().float()) if half else (lambda t: t)
        x = rnd(torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 21)))
        w = rnd(torch.from_numpy(synth.normal((Cin, Cout, 4, 4), (2.0 / (Cin * 4)) ** 0.5, 22)))
        scale = torch.from_numpy(synth.normal((Cout,), 0.2, 23)) + 1.0
        shift = torch.from_numpy(synth.normal((Cout,), 0.3, 24))
    if not has_scale:
        scale = torch.ones(Cout)
    out = {}
    for name, dt in (("ref", torch.float64), ("ref32", torch.float32)):
        y = F.conv_transpose2d(x.to(dt), w.to(dt), None, 2, 1)
        y = y * scale.to(dt).view(1, -1, 1, 1) + shift.to(dt).view(1, -1, 1, 1)
        out[name] = F.relu(y) if relu else y
    e32 = float((out["ref32"].double() - out["ref"]).abs().max())
    return dict(x=x, w=w, scale=scale, shift=shift, ref=out["ref"], e32=e32)


class _Deconv:
    """One case on the device: operands uploaded in the case's formats, y a sentinel tensor between guards"""

    def __init__(self, dev, c, ints=False):
        self.dev, self.c, self.lib = dev, c, native.lib()
        B, Cin, H, W, Cout = (c[k] for k in ("B", "Cin", "H", "W", "Cout"))
        self.half = c["dt"] == dc.F16
        x_hi = 3 if c["variant"] == native.C3_PERSIST else 1
        self.o = o = _deconv_operands(B, Cin, H, W, Cout, self.half, c["relu"], c["scale"], ints, x_hi)
        self.ip, self.op = dc.pitches(c)
        self.x, self.x_before = _upload_x(dev, o["x"], Cin, self.ip, dc.packed_in(c), self.half)
        w, scale = o["w"], o["scale"]
        if c["dt"] == dc.F32S and c["scale"]:   # prescale per OUTPUT channel (dim 1 of (Cin, Cout, 4, 4)), as the engine
            wt, factor = prescale_rows(w.transpose(0, 1).contiguous())
            w, scale = wt.transpose(0, 1), scale * factor
        w = w.contiguous().to(dev)
        self.wp = torch.zeros(self.lib.cn_packed_deconv4x4s2_weight_floats(Cin, Cout), device=dev, dtype=torch.float32)
        native.check(self.lib.cn_pack_deconv4x4s2_weight(native.ptr(w), native.ptr(self.wp), Cin, Cout,
                                                         dc.DTYPES[c["dt"]], native.stream_ptr()),
                     "cn_pack_deconv4x4s2_weight")
        n = dc.r32(Cout) + 128
        self.scale, self.shift = _padded(dev, scale, n), _padded(dev, o["shift"], n)
        self.OH, self.OW = 2 * H, 2 * W
        width = dc.r32(Cout) if dc.packed_out(c) else Cout
        assert c["rc"] != dc.OK or c["c_off"] + width <= self.op
        self.yn = B * self.OH * self.OW * self.op
        self.y = Buf(dev, self.yn, 2 if self.half else 4, 2 * (self.OW + 2) * self.op + 1024)
        torch.cuda.synchronize()

    def _args(self):
        c = self.c
        return dc.args(c, self.x.ptr() + c["x_off"], self.wp.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(),
                       self.y.ptr(c["c_off"]))

    def query(self):
        info = native.ConvRouteInfo()
        with native.tuning(self.c["keys"]):
            rc = self.lib.cn_conv_transpose4x4s2_route(*self._args(), None, ctypes.byref(info))
        return rc, info

    def run(self):
        with native.tuning(self.c["keys"]):
            rc = self.lib.cn_conv_transpose4x4s2(*self._args(), native.stream_ptr())
            torch.cuda.synchronize()
        return rc

    # unit: an element of y -- for an f32s tensor a half (a channel is a high and a low part, 32 halves apart)
    def units(self, t):
        return t.view(torch.int16) if dc.packed_out(self.c) else t

    def owned(self):
        """(own, pad) over units(): the channels [c_off, c_off + Cout) of every pixel, and the channels behind Cout
        of an f32s output's last 32-channel group, which a kernel may zero or leave"""
        c = self.c
        B, Cout, packed = c["B"], c["Cout"], dc.packed_out(c)
        n = self.yn * (2 if packed else 1)
        own = torch.zeros(n, dtype=torch.bool, device=self.dev)
        pad = torch.zeros(n, dtype=torch.bool, device=self.dev)
        if packed:
            assert c["c_off"] % 32 == 0
            vo = own.view(B, self.OH, self.OW, self.op // 32, 2, 32)
            vp = pad.view(B, self.OH, self.OW, self.op // 32, 2, 32)
            g0 = c["c_off"] // 32
            for g in range(dc.r32(Cout) // 32):
                k = min(Cout - 32 * g, 32)
                vo[..., g0 + g, :, :k] = True
                vp[..., g0 + g, :, k:] = True
        else:
            own.view(B, self.OH, self.OW, self.op)[..., c["c_off"]:c["c_off"] + Cout] = True
        return own, pad

    def output(self):
        """values (B, Cout, OH, OW) float64 on the CPU"""
        c = self.c
        v = self.y.values("f16" if self.half else "f32").view(c["B"], self.OH, self.OW, self.op)
        if dc.packed_out(c):
            v = unpack_f32s(v[..., c["c_off"]:c["c_off"] + dc.r32(c["Cout"])].contiguous())[..., :c["Cout"]]
        else:
            v = v[..., c["c_off"]:c["c_off"] + c["Cout"]]
        return v.double().cpu().permute(0, 3, 1, 2)

    def check_where_it_wrote(self):
        cid = self.c["id"]
        own, pad = self.owned()
        body = self.units(self.y.body)
        same = body == self.units(torch.full_like(self.y.body, self.y.sent))
        assert bool(same[~own & ~pad].all()), "%s: %d cells outside the call's own were written" % (
            cid, int((~same[~own & ~pad]).sum()))
        assert bool((same | (body == 0))[pad].all()), "%s: channels behind Cout hold neither zeros nor what they held" % cid
        if not dc.packed_out(self.c):      # (halves of an f32s tensor: an unwritten cell fails the comparison)
            assert not bool(self.y.is_sentinel(body)[own].any()), "%s: %d of the call's cells were not written" % (
                cid, int(self.y.is_sentinel(body)[own].sum()))
        assert self.y.guards_untouched(), cid
        assert torch.equal(self.x.t, self.x_before), cid


DECONV_OK = [c for c in dc.CASES if c["rc"] == dc.OK]


@pytest.mark.parametrize("cid", [c["id"] for c in DECONV_OK])
def test_the_routed_deconvolution_computes_the_reference(dev, cid):
    c = dc.BY_ID[cid]
    call = _Deconv(dev, c)
    rc, info = call.query()
    assert dc.said(rc, info) == dc.expected(c)
    assert call.run() == dc.OK
    call.check_where_it_wrote()
    _assert_close(cid, "y", call.output(), call.o["ref"], call.half, call.o["e32"])


@pytest.mark.parametrize("cid", [c["id"] for c in DECONV_OK if c["exact"]])
def test_the_routed_deconvolution_is_exact_on_integers(dev, cid):
    c = dc.BY_ID[cid]
    call = _Deconv(dev, c, ints=True)
    rc, info = call.query()
    assert dc.said(rc, info) == dc.expected(c)
    assert call.run() == dc.OK
    call.check_where_it_wrote()
    _assert_exact(cid, "y", call.output(), call.o["ref"])


@pytest.mark.parametrize("cid", [c["id"] for c in dc.CASES if c["rc"] != dc.OK])
def test_a_refused_deconvolution_writes_nothing(dev, cid):
    c = dc.BY_ID[cid]
    call = _Deconv(dev, c)
    rc, info = call.query()
    assert (rc, info.route, info.variant, info.n_tile, info.grid_x) == (c["rc"], native.ROUTE_NONE, 0, 0, 0)
    assert call.run() == c["rc"]
    assert bool(call.y.is_sentinel(call.y.t).all())
    assert torch.equal(call.x.t, call.x_before)


# ---- the heads --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _heads_operands(B, Cin, H, W, hidden, couts, bias1, bias2, ints, x_hi):
    nh = len(couts)
    if ints:
        rng = np.random.RandomState(B * 1000 + Cin + 7 * hidden + sum(couts))
        x = _ints(rng, (B, Cin, H, W), 0 if x_hi > 1 else -1, x_hi)
        w1 = _ints(rng, (nh * hidden, Cin, 3, 3), -1, 1)
        b1 = _ints(rng, (nh * hidden,), -3, 3)
        w2 = [_ints(rng, (co, hidden), -1, 1) for co in couts]
        b2 = [_ints(rng, (co,), -3, 3) for co in couts]
    else:
        x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 31))
        w1 = torch.from_numpy(synth.normal((nh * hidden, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, 32))
        b1 = torch.from_numpy(synth.normal((nh * hidden,), 0.3, 33))
        w2 = [torch.from_numpy(synth.normal((co, hidden), (2.0 / hidden) ** 0.5, 40 + h)) for h, co in enumerate(couts)]
        b2 = [torch.from_numpy(synth.normal((co,), 0.3, 50 + h)) for h, co in enumerate(couts)]
    if not bias1:
        b1 = torch.zeros_like(b1)
    b2 = [b if has else torch.zeros_like(b) for b, has in zip(b2, bias2)]
    refs = []
    for h, co in enumerate(couts):
        rows = slice(h * hidden, (h + 1) * hidden)
        hid = F.relu(F.conv2d(x.double(), w1[rows].double(), b1[rows].double(), 1, 1))
        refs.append(F.conv2d(hid, w2[h].double().view(co, hidden, 1, 1), b2[h].double()))
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, refs=refs)


class _Heads:
    """One case on the device: every head's map its own sentinel buffer of exactly B * cout * H * W floats"""

    def __init__(self, dev, c, ints=False):
        self.dev, self.c, self.lib = dev, c, native.lib()
        B, Cin, H, W, hidden, couts = (c[k] for k in ("B", "Cin", "H", "W", "hc", "couts"))
        x_hi = 3 if c["variant"] == native.C3_PERSIST else 1
        self.o = o = _heads_operands(B, Cin, H, W, hidden, couts, c["bias1"], c["bias2"], ints, x_hi)
        f32s = c["dt"] == hc.F32S
        self.ip = hc.in_pitch(c)
        self.x, self.x_before = _upload_x(dev, o["x"], Cin, self.ip, hc.packed_in(c), False)
        w1, self.scale1 = o["w1"], None
        if f32s:
            w1, factor1 = prescale_rows(w1)
            self.scale1 = factor1.contiguous().to(dev)
        w1 = w1.contiguous().to(dev)
        cd = hc.DTYPES[c["dt"]]
        n = self.lib.cn_packed_conv_weight_elems(len(couts) * hidden, Cin, 3, 3, cd)
        self.wp = torch.zeros(n, device=dev, dtype=torch.float32)
        native.check(self.lib.cn_pack_conv_weight(native.ptr(w1), native.ptr(self.wp), len(couts) * hidden, Cin, 3, 3,
                                                  cd, native.stream_ptr()), "cn_pack_conv_weight")
        self.b1 = o["b1"].to(dev)
        self.keep, self.y = [], []
        w, bias, osc, frag = [], [], [], []
        for h, co in enumerate(couts):
            w2, f2 = o["w2"][h], None
            if c["oscale"]:        # rows pre-scaled like every weight, undone by oscale
                w2, f2 = prescale_rows(w2)
                f2 = f2.contiguous().to(dev)
            w2 = w2.contiguous().to(dev)
            b2 = o["b2"][h].to(dev) if c["bias2"][h] else None
            wf = None
            if c["frag"]:
                wf = torch.zeros(self.lib.cn_packed_head_w2_bytes(co) + 16, device=dev, dtype=torch.uint8)
                off = 8 if c["frag"] == "misaligned" else 0
                if not off:
                    native.check(self.lib.cn_pack_head_w2_f32s(native.ptr(w2), native.ptr(wf), co,
                                                               native.stream_ptr()), "cn_pack_head_w2_f32s")
                frag.append(wf.data_ptr() + off)
            else:
                frag.append(None)
            self.y.append(Buf(dev, B * co * H * W, 4, 2 * W * co + 1024))
            self.keep += [w2, b2, f2, wf]
            w.append(w2.data_ptr())
            bias.append(b2.data_ptr() if b2 is not None else None)
            osc.append(f2.data_ptr() if f2 is not None else None)
        self.arr = hc.head_array(c, w, bias, [y.ptr() for y in self.y], osc, frag)
        torch.cuda.synchronize()

    def _args(self):
        return hc.args(self.c, self.x.ptr(), self.wp.data_ptr(),
                       self.scale1.data_ptr() if self.scale1 is not None else None, self.b1.data_ptr(), self.arr)

    def query(self):
        info = native.ConvRouteInfo()
        with native.tuning(self.c["keys"]):
            rc = self.lib.cn_heads3x3_1x1_route(*self._args(), None, ctypes.byref(info))
        return rc, info

    def run(self):
        with native.tuning(self.c["keys"]):
            rc = self.lib.cn_heads3x3_1x1(*self._args(), native.stream_ptr())
            torch.cuda.synchronize()
        return rc

    def check(self, compare):
        c = self.c
        for h, co in enumerate(c["couts"]):
            what = "head %d (%d outputs)" % (h, co)
            y = self.y[h]
            assert y.guards_untouched(), (c["id"], what)
            unwritten = int(y.is_sentinel(y.body).sum())
            assert unwritten == 0, "%s %s: %d cells were not written" % (c["id"], what, unwritten)
            compare(c["id"], what, y.values("f32").view(c["B"], co, c["H"], c["W"]).double().cpu(), self.o["refs"][h])
        assert torch.equal(self.x.t, self.x_before), c["id"]


HEADS_OK = [c for c in hc.CASES if c["rc"] == hc.OK]


def _heads_said(c, rc, info):
    assert hc.said(rc, info) == hc.expected(c)
    if c["grid"]:
        assert (info.grid_x, info.grid_y) == c["grid"]


@pytest.mark.parametrize("cid", [c["id"] for c in HEADS_OK])
def test_the_routed_heads_compute_the_reference(dev, cid):
    c = hc.BY_ID[cid]
    call = _Heads(dev, c)
    _heads_said(c, *call.query())
    assert call.run() == hc.OK
    call.check(lambda *a: _assert_close(*a, False, 0.0))


@pytest.mark.parametrize("cid", [c["id"] for c in HEADS_OK if c["exact"]])
def test_the_routed_heads_are_exact_on_integers(dev, cid):
    c = hc.BY_ID[cid]
    call = _Heads(dev, c, ints=True)
    _heads_said(c, *call.query())
    assert call.run() == hc.OK
    call.check(_assert_exact)


@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES if c["rc"] != hc.OK])
def test_refused_heads_write_nothing(dev, cid):
    c = hc.BY_ID[cid]
    call = _Heads(dev, c)
    rc, info = call.query()
    assert (rc, info.route, info.variant, info.n_tile, info.grid_x) == (c["rc"], native.ROUTE_NONE, 0, 0, 0)
    assert call.run() == c["rc"]
    for y in call.y:
        assert bool(y.is_sentinel(y.t).all())
    assert torch.equal(call.x.t, call.x_before)
