"""The fp16 compute mode's new operations at kernel level: the deformable convolution (cn_dcn_v2_forward_nhwc_f16, both forms,
through the C ABI), ConvTranspose 4x4/s2, the max-pool and the offset convolution that writes plain fp32 from a half
activation (through the plan builder).  Cases, operand builders and the float64 references: tests/dcn_half_cases.py.

A1, exact operands: x integers in [-2, 2], w in {-1, 0, 1}, offsets multiples of 0.5, masks in {0, 0.5, 1}, scales in
{1, 2, -1, 0.5}, integer shifts.  Every sample is a multiple of 1/8 and every step of the chain -- corner reads as
halves, fp32 blend and mask, the rounding to fp16, fp32 accumulation in any order, fp32 epilogue, the rounding at the
store -- is exact (asserted on the reference first), so the output must EQUAL the float64 reference cast to half.

A2, normal data: x and w rounded to fp16 first, offsets fp32, masks probabilities.  Element-wise
    |got - ref64| <= 2^-11 |ref64| + 2^-25 + |scale| 2^-11 (|w| . |cols|) + 4 E32
with E32 = max |C-oracle fp32 result - ref64| on the same operands: the half-ulp of the stored result, the one
rounding of every sample bounded term by term, and the margin of 4 over an fp32 evaluation's own error that
tests/test_gpu_half.py uses.  mask_sigmoid = 1 with logit masks adds 2e-5 (1 + |ref|) (dcn_cases.TOL) for the
in-kernel sigmoid.  Each case prints the observed max((err - first three terms) / E32).

Every output is pre-filled with a NaN sentinel; columns behind Cout must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centernet_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as dh   # noqa: E402
import half_cases as hc       # noqa: E402
from dcn_cases import TOL     # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [c["id"] for c in dh.CASES]
SENT16 = 0x7E5A             # a half NaN no kernel produces


@pytest.fixture(autouse=True)
def _default_tuning():
    """Every test of this module leaves the cn_set_tuning keys at the library's defaults."""
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _run_dcn(dev, c, d, msig=False, keys=None):
    """One cn_dcn_v2_forward_nhwc_f16 call under the case's keys.
    -> (y (B, Cout, H, W) float32 on the CPU, the raw (B, H, W, out_pitch) int16 view, route info)"""
    from centernet_amd import native
    lib = native.lib()
    B, Cin, H, W, Cout = (c[n] for n in ("B", "Cin", "H", "W", "Cout"))
    pitch = Cout + c["pad"]
    x = d["x"].permute(0, 2, 3, 1).contiguous().to(dev, torch.float16)
    w = d["w"].float().contiguous().to(dev)
    wp = torch.empty(lib.cn_packed_conv_weight_elems(Cout, Cin, 3, 3, native.DTYPE_F16), device=dev, dtype=torch.float16)
    native.check(lib.cn_pack_conv_weight(native.ptr(w), native.ptr(wp), Cout, Cin, 3, 3, native.DTYPE_F16,
                                         native.stream_ptr()), "cn_pack_conv_weight")
    om = torch.full((B, H, W, 32), float("nan"), dtype=torch.float32)       # columns >= 27 are never read
    om[..., :18] = d["off"].permute(0, 2, 3, 1)
    m = d["mask"].permute(0, 2, 3, 1)
    if msig:
        m64 = m.double()
        m = torch.log(m64 / (1.0 - m64)).float()
    om[..., 18:27] = m
    om = om.to(dev)
    bias, scale, shift = (d[k].float().contiguous().to(dev) for k in ("bias", "scale", "shift"))
    y = torch.empty((B, H, W, pitch), device=dev, dtype=torch.float16)
    y.view(torch.int16).fill_(SENT16)
    ws, wsb = None, 0
    if c["ws"]:
        wsb = int(lib.cn_dcn_v2_forward_nhwc_workspace_bytes(B, Cin, H, W, Cout))
        assert wsb > 0
        ws = torch.full((wsb // 4,), float("nan"), device=dev, dtype=torch.float32)
    info = native.DcnRouteInfo()
    with native.tuning(dict(c["keys"] if keys is None else keys)):
        args = (native.ptr(x), native.ptr(wp), native.ptr(bias), native.ptr(om), 32, native.ptr(scale), native.ptr(shift),
                native.ptr(y), pitch, B, Cin, H, W, Cout, int(msig), int(c["relu"]), native.ptr(ws), wsb,
                native.stream_ptr())
        native.check(lib.cn_dcn_v2_route_f16(*args, ctypes.byref(info)), "cn_dcn_v2_route_f16")
        native.check(lib.cn_dcn_v2_forward_nhwc_f16(*args), "cn_dcn_v2_forward_nhwc_f16")
        torch.cuda.synchronize()
    raw = y.view(torch.int16).cpu()
    return y[..., :Cout].permute(0, 3, 1, 2).float().cpu(), raw, info


def _check_route_and_padding(c, raw, info):
    from centernet_amd import native
    want = {"window": native.DCNH_WINDOW, "gather": native.DCN_GATHER, "gather_pad": native.DCN_GATHER_PAD}[c["form"]]
    assert info.form == want, (c["id"], native.dcn_form_name(info.form))
    assert (info.ksplit > 1) == bool(c["ws"]), (c["id"], info.ksplit)
    if c["pad"]:
        assert bool((raw[..., c["Cout"]:] == np.int16(SENT16)).all()), "columns behind Cout were written"


@pytest.mark.parametrize("cid", IDS)
def test_dcn_exact_operands_give_the_reference_exactly(dev, cid):
    c, d = dh.case(cid), dh.int_case(cid)
    ok, top, nonzero = dh.exactness(d["ref"])
    assert ok and nonzero >= 0.9, (cid, top, nonzero)
    got, raw, info = _run_dcn(dev, c, d)
    _check_route_and_padding(c, raw, info)
    want = d["ref"].half().float()
    bad = got != want
    assert torch.equal(got, want), "%s: %d of %d values differ, first at %s: got %s, want %s" % (
        cid, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), got[bad][:4].tolist(), want[bad][:4].tolist())


def _a2_check(cid, got, d, extra=None):
    three, e4 = dh.a2_bar(d)
    if extra is not None:
        three = three + extra
    err = (got.double() - d["ref"]).abs()
    ratio = float(((err - three) / d["e32"]).max())
    print("A2 %s: E32 %.3e, max |err| %.3e, max (err - first three terms) / E32 = %.3f" % (
        cid, d["e32"], float(err.max()), ratio))
    assert not torch.isnan(got).any(), cid
    over = err > three + e4
    assert not bool(over.any()), "%s: %d values beyond the bar, ratio %.3f" % (cid, int(over.sum()), ratio)


@pytest.mark.parametrize("cid", IDS)
def test_dcn_normal_operands_within_the_bar(dev, cid):
    c, d = dh.case(cid), dh.normal_case(cid)
    got, raw, info = _run_dcn(dev, c, d)
    _check_route_and_padding(c, raw, info)
    _a2_check(cid, got, d)


@pytest.mark.parametrize("cid", ["win_2x2_two_chunks", "gat_pad"])
def test_dcn_in_kernel_sigmoid(dev, cid):
    """mask_sigmoid = 1 with logit masks, one case per form: the bar plus 2e-5 (1 + |ref|) for the sigmoid."""
    c, d = dh.case(cid), dh.normal_case(cid)
    got, raw, info = _run_dcn(dev, c, d, msig=True)
    _check_route_and_padding(c, raw, info)
    _a2_check(cid + "/sigmoid", got, d, extra=TOL * (1 + d["ref"].abs()))


@pytest.mark.parametrize("cid", ["win_one_tile", "win_stress"])
def test_the_two_forms_agree(dev, cid):
    """The same operands on a shape both forms take, window form forced and gather form forced: within the A2 bar
    of each other."""
    from centernet_amd import native
    c, d = dh.case(cid), dh.normal_case(cid)
    a, _, ia = _run_dcn(dev, c, d, keys=dh.WINDOW_KEYS)
    b, _, ib = _run_dcn(dev, c, d, keys=dh.GATHER_KEYS)
    assert ia.form == native.DCNH_WINDOW and ib.form == native.DCN_GATHER
    three, e4 = dh.a2_bar(d)
    diff = (a.double() - b.double()).abs()
    print("forms %s: max |window - gather| %.3e, %d of %d values differ" % (cid, float(diff.max()), int((diff > 0).sum()),
                                                                           diff.numel()))
    assert not torch.isnan(a).any() and not torch.isnan(b).any()
    assert not bool((diff > three + e4).any())


# ---- ConvTranspose 4x4 / s2, max-pool, offset convolution: through the plan builder ---------------------------------
def _half_builder(dev, B, H, W):
    from centernet_amd.engine import PlanBuilder
    return PlanBuilder(dev, B, H, W, dtype=torch.float16)


def _act(t_nchw, dev, dtype=torch.float16):
    from centernet_amd.engine import Act
    B, C, H, W = t_nchw.shape
    return Act(t_nchw.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=dtype), B, H, W, C,
               fmt="f16" if dtype == torch.float16 else "f32")


def _run_plan(pb, out):
    out.t.fill_(float("nan"))
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    return out.t[..., out.c_off:out.c_off + out.C].permute(0, 3, 1, 2).float().cpu()


@pytest.mark.parametrize("i", range(len(dh.DECONV_CASES)))
def test_transposed_conv_exact_and_normal(dev, i):
    B, Cin, H, W, Cout = dh.DECONV_CASES[i]
    # A1
    d = dh.deconv_int_case(i)
    ok, top, nonzero = dh.exactness(d["ref"])
    assert ok and nonzero >= 0.9, (i, top, nonzero)
    pb = _half_builder(dev, B, H, W)
    y = pb.conv_transpose4x4s2(_act(d["x"], dev), d["w"].float(), bn=d["bn"], relu=True)
    assert y.t.dtype == torch.float16 and (y.H, y.W, y.C) == (2 * H, 2 * W, Cout)
    got = _run_plan(pb, y)
    assert torch.equal(got, d["ref"].half().float()), "deconv %d: %d values differ" % (
        i, int((got != d["ref"].half().float()).sum()))
    # A2: the existing fp16-output bar, E32 from torch's fp32 CPU evaluation
    x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 11 + i)).half().float()
    w = torch.from_numpy(synth.normal((Cin, Cout, 4, 4), (2.0 / (Cin * 4)) ** 0.5, 21 + i)).half().float()
    bn = torch.nn.BatchNorm2d(Cout)
    synth.fill_state_dict_(bn, 31 + i)
    bn.eval()
    ref = torch.relu(hc.bn64(F.conv_transpose2d(x.double(), w.double(), None, 2, 1), bn)).detach()
    r32 = torch.relu(bn(F.conv_transpose2d(x, w, None, 2, 1))).detach()
    e32 = float((r32.double() - ref).abs().max())
    pb = _half_builder(dev, B, H, W)
    y = pb.conv_transpose4x4s2(_act(x, dev), w, bn=bn, relu=True)
    got = _run_plan(pb, y)
    err = (got.double() - ref).abs()
    half_ulp = ref.abs() * 2.0 ** -11 + 2.0 ** -25
    print("A2 deconv %d: E32 %.3e, max |err| %.3e, max (err - half-ulp) / E32 = %.3f" % (
        i, e32, float(err.max()), float(((err - half_ulp) / e32).max())))
    assert not torch.isnan(got).any()
    assert not bool((err > half_ulp + 4.0 * e32).any())


@pytest.mark.parametrize("case", dh.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_max_pool_is_exact(dev, case):
    B, C, H, W, k, s, p = case
    for name, x in (("ints", dh._ints(np.random.RandomState(5), (B, C, H, W), -8, 8)),
                    ("normal", torch.from_numpy(synth.normal((B, C, H, W), 1.0, 6)).half().float())):
        pb = _half_builder(dev, B, H, W)
        y = pb.maxpool(_act(x, dev), k, s, p)
        assert y.t.dtype == torch.float16
        got = _run_plan(pb, y)
        want = dh.pool_ref(x, k, s, p).float()
        assert got.shape == want.shape and torch.equal(got, want), (case, name, int((got != want).sum()))


@pytest.mark.parametrize("shape,form", [((2, 64, 12, 20), "halo"), ((1, 512, 4, 4), "split-K")],
                         ids=["halo", "splitk"])
def test_offset_conv_writes_plain_fp32_from_halves(dev, shape, form):
    """The 27-channel conv_offset_mask of a half plan: half activation in, plain fp32 at pitch 32 out
    (CN_CONV_Y_PLAIN with CN_DTYPE_F16).  The fp32-output bar of tests/test_gpu_half.py: |got - ref64| <= 4 E32.
    Columns 27 .. 31 keep the NaN fill."""
    B, Cin, H, W = shape
    x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 41)).half().float()
    w = torch.from_numpy(synth.normal((27, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, 42)).half().float()
    bias = torch.from_numpy(synth.normal((27,), 0.3, 43))
    pb = _half_builder(dev, B, H, W)
    om = pb._new(B, H, W, 27, pitch=32, fmt="f32")
    assert om.t.dtype == torch.float32
    pb.conv(_act(x, dev), w, bias=bias, stride=1, padding=1, out=om)
    om.t.fill_(float("nan"))
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    t = om.t.cpu()
    assert bool(torch.isnan(t[..., 27:]).all()), "pad columns were written"
    got = t[..., :27].permute(0, 3, 1, 2)
    args = (x, w, bias, None, None, False, 1, 1)
    ref = hc.ref64(*args)
    e32 = float((hc.ref32(*args).double() - ref).abs().max())
    err = (got.double() - ref).abs()
    print("A2 offset conv %s: E32 %.3e, max |err| %.3e = %.3f E32" % (form, e32, float(err.max()), float(err.max()) / e32))
    assert not torch.isnan(got).any()
    assert not bool((err > 4.0 * e32).any())
    # and exactly: integer operands
    xi = dh._ints(np.random.RandomState(7), (B, Cin, H, W), -1, 1)
    wi = dh._ints(np.random.RandomState(8), (27, Cin, 3, 3), -1, 1)
    bi = dh._ints(np.random.RandomState(9), (27,), -8, 8)
    pb = _half_builder(dev, B, H, W)
    om = pb._new(B, H, W, 27, pitch=32, fmt="f32")
    pb.conv(_act(xi, dev), wi, bias=bi, stride=1, padding=1, out=om)
    om.t.fill_(float("nan"))
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    assert torch.equal(om.t.cpu()[..., :27].permute(0, 3, 1, 2).double(), hc.ref64(xi, wi, bi, None, None, False, 1, 1))
