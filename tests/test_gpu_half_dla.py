"""The half forms dla_34 needs in a half plan, at kernel level, against float64 references: the depthwise
transposed convolution, the channel-slice copy, the max-pool into a slice, a half convolution that writes a
slice and reads its residual from one, and the half form of the 16-channel 3x3 kernel (cn_conv16.hip).  Cases
and references: tests/half_dla_cases.py; the two-step discipline (A1 exact integers, A2 a derived bar) and
its helpers: tests/test_gpu_half.py / tests/half_cases.py.

Every output is pre-filled with NaN; every buffer wider than what a launch owns is pre-filled with a sentinel
that is checked afterwards."""
import ctypes
import os
import sys

import pytest
import torch

from centernet_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_cases as hc        # noqa: E402
import half_dla_cases as dc    # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 1234.0              # an fp16 number no case produces
NAN = float("nan")
UNSUPPORTED, ALIGN = -2, -6        # CN_ERR_UNSUPPORTED, CN_ERR_ALIGN


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _nhwc(t, dev, dtype=torch.float16):
    return t.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=dtype)


def _equal(tag, g, want):
    bad = g != want
    assert torch.equal(g, want), "%s: %d of %d values differ, first at %s: got %s, want %s" % (
        tag, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), g[bad][:4].tolist(), want[bad][:4].tolist())


# ---- cn_dw_conv_transpose_f16 -----------------------------------------------------------------------------
def _dw_launch(dev, x, w, add, f):
    """x (B, C, H, W), w (C, 1, 2f, 2f) fp32, add (B, C, fH, fW) or None -> (B, C, fH, fW) halves on the CPU."""
    from centernet_amd import native
    B, C, H, W = x.shape
    xa = _nhwc(x, dev)
    aa = _nhwc(add, dev) if add is not None else None
    taps = w[:, 0].permute(1, 2, 0).reshape(4 * f * f, C).contiguous().to(dev)     # as PlanBuilder.dw_deconv
    y = torch.full((B, H * f, W * f, C), NAN, device=dev, dtype=torch.float16)
    rc = native.lib().cn_dw_conv_transpose_f16(native.ptr(xa), native.ptr(taps), native.ptr(aa), native.ptr(y),
                                               B, H, W, C, f, native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == native.CN_OK, rc
    return y.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("run", dc.DW_RUNS, ids=dc.DW_IDS)
def test_dw_deconv_f16_bilinear_integers_exact(dev, run):
    shape, with_add = run
    d = dc.dw_int_case(shape, with_add)
    assert dc.dw_exact(d, shape[4])
    got = _dw_launch(dev, d["x"], d["w"], d["add"], shape[4])
    _equal("dw %s" % (shape,), got, d["ref"].half())


@pytest.mark.parametrize("run", dc.DW_RUNS, ids=dc.DW_IDS)
def test_dw_deconv_f16_normal_data_within_the_rounding_bar(dev, run):
    """|got - ref64| <= 2^-11 |ref64| + 2^-25 + 8 * 2^-24 * sum |terms|: the half-ulp of the one rounding plus fp32
    accumulation of at most five terms (the <= 4 products and ``add``) in any order."""
    (B, H, W, C, f), with_add = run
    x = torch.from_numpy(synth.normal((B, C, H, W), 1.0, 31)).half().float()
    w = dc.dw_bilinear_weight(C, f) * (1.0 + 0.25 * torch.from_numpy(synth.normal((C, 1, 2 * f, 2 * f), 1.0, 32)))
    add = torch.from_numpy(synth.normal((B, C, H * f, W * f), 1.0, 33)).half().float() if with_add else None
    ref, mag = dc.dw_ref64(x, w, add, f)
    got = _dw_launch(dev, x, w, add, f)
    err = (got.double() - ref).abs()
    bar = ref.abs() * 2.0 ** -11 + 2.0 ** -25 + 8 * 2.0 ** -24 * mag
    print("A2 dw %s add=%d: max |err| %.3e, max err / bar %.3f" % ((B, H, W, C, f), with_add, float(err.max()),
                                                                  float((err / bar).max())))
    assert not torch.isnan(got).any()
    assert not bool((err > bar).any()), int((err > bar).sum())


def test_dw_deconv_f16_refuses_twelve_channels(dev):
    from centernet_amd import native
    x = torch.zeros((1, 2, 2, 12), device=dev, dtype=torch.float16)
    taps = torch.zeros((16, 12), device=dev)
    y = torch.zeros((1, 4, 4, 12), device=dev, dtype=torch.float16)
    rc = native.lib().cn_dw_conv_transpose_f16(native.ptr(x), native.ptr(taps), None, native.ptr(y), 1, 2, 2, 12, 2,
                                               native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED


# ---- cn_copy_channels_f16, max-pool into a slice ---------------------------------------------------------
S_PITCH, S_OFF, D_PITCH, D_OFF, CW = 24, 8, 40, 16, 16


def _sentinel_kept(dst):
    assert bool((dst[..., :D_OFF] == SENTINEL).all()) and bool((dst[..., D_OFF + CW:] == SENTINEL).all())


def test_copy_channels_f16_between_slices(dev):
    from centernet_amd import native
    B, H, W = 2, 3, 5
    src = torch.from_numpy(synth.normal((B, H, W, S_PITCH), 1.0, 41)).to(dev, torch.float16)
    dst = torch.full((B, H, W, D_PITCH), SENTINEL, device=dev, dtype=torch.float16)
    dst[..., D_OFF:D_OFF + CW] = NAN
    rc = native.lib().cn_copy_channels_f16(ctypes.c_void_p(src.data_ptr() + 2 * S_OFF), S_PITCH,
                                           ctypes.c_void_p(dst.data_ptr() + 2 * D_OFF), D_PITCH, B * H * W, CW,
                                           native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == native.CN_OK
    assert torch.equal(dst[..., D_OFF:D_OFF + CW], src[..., S_OFF:S_OFF + CW])
    _sentinel_kept(dst)
    # C, pitches: multiples of 8; pointers: 16-byte aligned
    call = native.lib().cn_copy_channels_f16
    assert call(native.ptr(src), S_PITCH, native.ptr(dst), D_PITCH, 4, 12, native.stream_ptr()) == UNSUPPORTED
    assert call(native.ptr(src), 20, native.ptr(dst), D_PITCH, 4, 8, native.stream_ptr()) == UNSUPPORTED
    assert call(ctypes.c_void_p(src.data_ptr() + 8), S_PITCH, native.ptr(dst), D_PITCH, 4, 8,
                native.stream_ptr()) == ALIGN
    torch.cuda.synchronize()


def test_half_maxpool_into_a_slice(dev):
    """PlanBuilder(dtype=float16).maxpool(out=slice): MaxPool2d(2, 2) of a slice (pitch 24, offset 8) into a slice
    (pitch 40, offset 16), B * Ho * Wo = 2 * 3 * 5; ``to_s`` is ignored in a half plan."""
    from centernet_amd.engine import PlanBuilder, Act
    B, Ho, Wo = 2, 3, 5
    src = torch.from_numpy(synth.normal((B, 2 * Ho, 2 * Wo, S_PITCH), 1.0, 42)).to(dev, torch.float16)
    dst = torch.full((B, Ho, Wo, D_PITCH), SENTINEL, device=dev, dtype=torch.float16)
    dst[..., D_OFF:D_OFF + CW] = NAN
    pb = PlanBuilder(dev, B, 2 * Ho, 2 * Wo, dtype=torch.float16)
    xa = Act(src, B, 2 * Ho, 2 * Wo, CW, pitch=S_PITCH, c_off=S_OFF, fmt="f16")
    oa = Act(dst, B, Ho, Wo, CW, pitch=D_PITCH, c_off=D_OFF, fmt="f16")
    y = pb.maxpool(xa, 2, 2, 0, out=oa, to_s=True)
    assert y is oa
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    want = torch.nn.functional.max_pool2d(src[..., S_OFF:S_OFF + CW].permute(0, 3, 1, 2).float(), 2, 2)
    assert torch.equal(dst[..., D_OFF:D_OFF + CW], want.permute(0, 2, 3, 1).half())
    _sentinel_kept(dst)


def test_half_concat_buffer_and_copying_concat(dev):
    """concat_buffer in a half plan hands out half slices (widths that are multiples of 8); a member in place is not
    copied, a private one is; the copying concat gives the same bytes."""
    from centernet_amd.engine import PlanBuilder, Act
    B, H, W = 1, 3, 5
    pb = PlanBuilder(dev, B, H, W, dtype=torch.float16)
    assert pb.concat_buffer(B, H, W, [16, 12]) == (None, None)
    buf, slots = pb.concat_buffer(B, H, W, [16, 8, 24])
    assert buf.fmt == "f16" and buf.t.dtype == torch.float16 and buf.pitch == 48
    assert [(s.c_off, s.C, s.pitch, s.fmt) for s in slots] == [(0, 16, 48, "f16"), (16, 8, 48, "f16"), (24, 24, 48, "f16")]
    parts = [torch.from_numpy(synth.normal((B, H, W, c), 1.0, 50 + c)).to(dev, torch.float16) for c in (16, 8, 24)]
    buf.t.fill_(NAN)
    slots[0].t[..., 0:16] = parts[0]                       # in place
    slots[2].t[..., 24:48] = parts[2]
    private = Act(parts[1], B, H, W, 8, fmt="f16")
    n0 = len(pb.ops)
    out = pb.concat([slots[0], private, slots[2]], into=buf)
    assert out is buf and len(pb.ops) == n0 + 1            # one copy: the private member
    copied = pb.concat([Act(p, B, H, W, p.shape[-1], fmt="f16") for p in parts])
    copied.t.fill_(NAN)
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    want = torch.cat(parts, dim=-1)
    assert torch.equal(buf.t, want) and torch.equal(copied.t, want)


# ---- a half convolution into a slice, residual from a slice ---------------------------------------------
@pytest.mark.parametrize("knobs", dc.SLICE_VARIANTS, ids=["k5=1", "default"])
def test_half_conv_into_a_slice_with_a_sliced_residual(dev, knobs):
    """3x3 / s1 64 -> 64 + BN + ReLU + residual, B = 2, 9 x 20: output into channels 64 .. 127 of a 192-wide half
    buffer, residual channels 32 .. 95 of a 128-wide one.  Key 5 = 1: the halo kernel takes the residual at its own
    pitch; default: whatever the route gives (KT = 9 wants no K split at this shape, so that is the halo kernel as
    well; the builder's fallback to a private tensor is test_half_conv_fallback_writes_a_private_tensor's).  A1: the
    result equals the float64 reference."""
    from centernet_amd import native
    from centernet_amd.engine import PlanBuilder, Act
    c = dc.SLICE_CONV
    d = dc.int_case(c["id"])
    ok, _, nonzero = hc.exactness(d["ref"])
    assert ok and nonzero >= 0.9
    B, H, W, Co = c["B"], c["H"], c["W"], c["Cout"]
    with native.tuning(dict(knobs)):
        pb = PlanBuilder(dev, B, H, W, dtype=torch.float16)
        xa = Act(_nhwc(d["x"], dev), B, H, W, c["Cin"], fmt="f16")
        rbuf = torch.full((B, H, W, c["res_pitch"]), SENTINEL, device=dev, dtype=torch.float16)
        rbuf[..., c["res_off"]:c["res_off"] + Co] = _nhwc(d["res"], dev)
        ra = Act(rbuf, B, H, W, Co, pitch=c["res_pitch"], c_off=c["res_off"], fmt="f16")
        obuf = torch.full((B, H, W, c["out_pitch"]), SENTINEL, device=dev, dtype=torch.float16)
        oa = Act(obuf, B, H, W, Co, pitch=c["out_pitch"], c_off=c["c_off"], fmt="f16")
        y = pb.conv(xa, d["w"], bn=d["bn"], relu=True, residual=ra, stride=1, padding=1, out=oa)
        in_place = y.t is obuf
        print("slice conv %s: written %s" % (dict(knobs), "in place" if in_place else "to a private tensor"))
        if dict(knobs).get(5) == 1:
            assert in_place and y.c_off == c["c_off"] and y.pitch == c["out_pitch"]
        y.t[..., y.c_off:y.c_off + Co] = NAN
        for op in pb.ops:
            op()
        torch.cuda.synchronize()
    got = y.t[..., y.c_off:y.c_off + Co].permute(0, 3, 1, 2).cpu()
    _equal("slice conv", got, d["ref"].half())
    lo, hi = c["c_off"], c["c_off"] + Co
    assert bool((obuf[..., :lo] == SENTINEL).all()) and bool((obuf[..., hi:] == SENTINEL).all())
    if not in_place:
        assert bool((obuf == SENTINEL).all())
    assert bool((rbuf[..., :c["res_off"]] == SENTINEL).all()) and bool((rbuf[..., c["res_off"] + Co:] == SENTINEL).all())


def test_half_conv_fallback_writes_a_private_tensor(dev):
    """The builder's fallback in a half plan, at kernel level: 128 -> 64 + BN + ReLU + residual on a 9 x 20 map wants
    split-K, so no kernel takes the residual (a private tensor, pitch 64) at a pitch of its own next to an output
    slice (pitch 192): cn_conv2d_res_pitch_supported answers 0, the layer writes a private tensor (A1: equal to the
    float64 reference), the buffer is untouched, and the concatenation copies the result into its slice."""
    from centernet_amd.engine import PlanBuilder, Act
    c = dc.FALLBACK_CONV
    d = dc.int_case(c["id"])
    ok, _, nonzero = hc.exactness(d["ref"])
    assert ok and nonzero >= 0.9
    B, H, W, Co = c["B"], c["H"], c["W"], c["Cout"]
    pb = PlanBuilder(dev, B, H, W, dtype=torch.float16)
    xa = Act(_nhwc(d["x"], dev), B, H, W, c["Cin"], fmt="f16")
    ra = Act(_nhwc(d["res"], dev), B, H, W, Co, fmt="f16")
    buf, slots = pb.concat_buffer(B, H, W, [Co, Co, Co])
    assert buf.pitch == c["out_pitch"] and slots[1].c_off == c["c_off"]
    y = pb.conv(xa, d["w"], bn=d["bn"], relu=True, residual=ra, stride=1, padding=1, out=slots[1])
    assert y.t is not buf.t and y.fmt == "f16" and y.pitch == Co and y.c_off == 0
    n_conv = len(pb.ops)
    y.t.fill_(NAN)
    buf.t.fill_(SENTINEL)
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    _equal("fallback conv", y.t.permute(0, 3, 1, 2).cpu(), d["ref"].half())
    assert bool((buf.t == SENTINEL).all())
    # the Root's concatenation: the private result is copied, the members in place are not
    out = pb.concat([slots[0], y, slots[2]], into=buf)
    assert out is buf and len(pb.ops) == n_conv + 1
    pb.ops[-1]()
    torch.cuda.synchronize()
    lo, hi = c["c_off"], c["c_off"] + Co
    assert torch.equal(buf.t[..., lo:hi], y.t)
    assert bool((buf.t[..., :lo] == SENTINEL).all()) and bool((buf.t[..., hi:] == SENTINEL).all())


@pytest.mark.parametrize("on", [1, 0], ids=["k65=1", "k65=0"])
def test_half_conv_16_to_27_with_a_plain_fp32_output_is_not_the_half_form(dev, on):
    """CN_DTYPE_F16 with CN_CONV_Y_PLAIN (the offset convolution of a half plan): y is plain fp32 at a pitch in
    floats.  With 16 input channels and W = 128 the descriptor has the half form's shape but not its store: the
    query answers 0 whatever key 65 says, and the result is the float64 reference in fp32 (A1), channels 27 .. 31
    of the pitch-32 tensor untouched."""
    from centernet_amd import native
    from centernet_amd.engine import PlanBuilder, Act
    c = dc.YPLAIN_CONV
    d = dc.int_case(c["id"])
    assert hc.exactness(d["ref"])[0]
    B, H, W, Co = c["B"], c["H"], c["W"], c["Cout"]
    with native.tuning({dc.KEY: on}):
        desc = dc.conv_desc(c, native.DTYPE_F16, native.CONV_Y_PLAIN)
        assert native.lib().cn_conv16_f16_supported(ctypes.byref(desc)) == 0
        pb = PlanBuilder(dev, B, H, W, dtype=torch.float16)
        xa = Act(_nhwc(d["x"], dev), B, H, W, 16, fmt="f16")
        om = pb._new(B, H, W, Co, pitch=c["out_pitch"], fmt="f32")        # as PlanBuilder.dcn allocates it
        y = pb.conv(xa, d["w"], bias=d["bias"], stride=1, padding=1, out=om)
        assert y is om and om.t.dtype == torch.float32
        om.t.fill_(SENTINEL)
        om.t[..., :Co] = NAN
        for op in pb.ops:
            op()
        torch.cuda.synchronize()
    _equal("16 -> 27, plain fp32 y", om.t[..., :Co].permute(0, 3, 1, 2).cpu(), d["ref"].float())
    assert bool((om.t[..., Co:] == SENTINEL).all())


# ---- conv16h ----------------------------------------------------------------------------------------------
def _conv16_launch(dev, c, on, x, w, bias, bn):
    """The case through PlanBuilder(dtype=float16).conv under key 65 = ``on`` -> (B, Cout, Ho, Wo) halves on the CPU."""
    from centernet_amd import native
    from centernet_amd.engine import PlanBuilder, Act
    lib = native.lib()
    Ho, Wo = hc.out_hw(c)
    with native.tuning({dc.KEY: on}):
        assert lib.cn_conv16_f16_supported(ctypes.byref(dc.conv_desc(c, native.DTYPE_F16))) == on
        pb = PlanBuilder(dev, c["B"], c["H"], c["W"], dtype=torch.float16)
        xa = Act(_nhwc(x, dev), c["B"], c["H"], c["W"], 16, fmt="f16")
        obuf = torch.full((c["B"], Ho, Wo, c["out_pitch"]), SENTINEL, device=dev, dtype=torch.float16)
        oa = Act(obuf, c["B"], Ho, Wo, c["Cout"], pitch=c["out_pitch"], c_off=c["c_off"], fmt="f16")
        y = pb.conv(xa, w, bias=bias, bn=bn, relu=c["relu"], stride=c["s"], padding=1, out=oa)
        assert y is oa
        lo, hi = c["c_off"], c["c_off"] + c["Cout"]
        obuf[..., lo:hi] = NAN
        for op in pb.ops:
            op()
        torch.cuda.synchronize()
    assert bool((obuf[..., :lo] == SENTINEL).all()) and bool((obuf[..., hi:] == SENTINEL).all()), "sentinel overwritten"
    return obuf[..., lo:hi].permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("run", dc.CONV16_RUNS, ids=dc.CONV16_IDS)
def test_conv16h_integer_operands_give_the_reference_exactly(dev, run):
    c, on = run
    d = dc.int_case(c["id"])
    ok, top, nonzero = hc.exactness(d["ref"])
    assert ok and nonzero >= 0.9, (c["id"], top, nonzero)
    got = _conv16_launch(dev, c, on, d["x"], d["w"], d["bias"], d["bn"])
    _equal("%s key %d = %d" % (c["id"], dc.KEY, on), got, d["ref"].half())


@pytest.mark.parametrize("run", dc.CONV16_RUNS, ids=dc.CONV16_IDS)
def test_conv16h_normal_operands_within_the_rounding_bar(dev, run):
    """The A2 bar of tests/test_gpu_half.py: |got - ref64| <= 2^-11 |ref64| + 2^-25 + 4 E32."""
    c, on = run
    B, Cin, H, W, Cout = (c[n] for n in ("B", "Cin", "H", "W", "Cout"))
    x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 1)).half().float()
    w = torch.from_numpy(synth.normal((Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, 2)).half().float()
    bn = bias = None
    if c["bn"]:
        bn = torch.nn.BatchNorm2d(Cout)
        synth.fill_state_dict_(bn, 4)
        bn.eval()
    elif c["bias"]:
        bias = torch.from_numpy(synth.normal((Cout,), 0.3, 3))
    got = _conv16_launch(dev, c, on, x, w, bias, bn)
    args = (x, w, bias, bn, None, c["relu"], c["s"], 1)
    ref = hc.ref64(*args).detach()
    e32 = float((hc.ref32(*args).double() - ref).abs().max())
    assert e32 > 0
    err = (got.double() - ref).abs()
    half_ulp = ref.abs() * 2.0 ** -11 + 2.0 ** -25
    print("A2 %s key %d = %d: E32 %.3e, max |err| %.3e, max (err - half-ulp) / E32 = %.3f" % (
        c["id"], dc.KEY, on, e32, float(err.max()), float(((err - half_ulp) / e32).max())))
    assert not torch.isnan(got).any()
    over = err > half_ulp + 4.0 * e32
    assert not bool(over.any()), int(over.sum())
