"""The half-precision convolution kernels (BASELINE configs[4]) at kernel level, through the plan
builder, against a float64 torch reference.  The case list, the kernel form each case reaches and
the operand builders live in tests/half_cases.py.

A1, exact integers: operands in {-1, 0, 1}, power-of-two / half scales, integer shifts and residuals.
fp16 storage, fp32 accumulation in any order and the epilogue are then all exact (the condition is
asserted on the reference first, and for the whole list on the CPU by test_half_cases_host.py), so
the result must EQUAL the reference: a difference is a wrong or missing term.  The same cases run on
the fp32-MFMA kernels (split=False), for which the argument holds as well.  (Equality of values: a
NaN -- every output is pre-filled with NaN -- or any wrong number fails it; the sign of a zero, which
no term of the sum decides, does not.)

A2, normal data: operands rounded to fp16 first.  With ref64 the float64 result and E32 the largest
error of torch's own fp32 CPU evaluation of the same operands against ref64,
    |got - ref64| <= 2^-11 |ref64| + 2^-25 + 4 E32        (fp16 outputs)
    |got - ref64| <= 4 E32                                 (fp32 NCHW outputs)
element-wise: the half-ulp of the one fp16 rounding of the stored result (normal / subnormal range)
plus a margin of 4 over the reference's own fp32 accumulation error for another summation order
(MFMA blocks, K split, fma against mul + add in the epilogue).  Each case prints the observed
max((err - half-ulp term) / E32)."""
import os
import sys

import pytest
import torch

from centernet_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_cases as hc   # noqa: E402

pytestmark = pytest.mark.gpu
RUNS = hc.runs()
RUN_IDS = [rid for _, _, rid in RUNS]


@pytest.fixture(autouse=True)
def _default_tuning():
    """Every test of this module leaves the cn_set_tuning keys at the library's defaults."""
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _nhwc(t, dev, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=dtype)


def _builder(dev, c, dtype):
    from centernet_amd.engine import PlanBuilder
    if dtype == torch.float16:
        return PlanBuilder(dev, c["B"], c["H"], c["W"], dtype=torch.float16)
    return PlanBuilder(dev, c["B"], c["H"], c["W"], dtype=torch.float32, split=False)


def _launch(dev, c, knobs, dtype, x, w, bias, bn, res, lasts=()):
    """Build and run the case under ``knobs``.  Returns [first output as (B, C, H, W) on the CPU, then one
    NCHW map per entry of ``lasts`` = ((w2, b2), ...), the 1x1 heads on 64-channel slices of the first output]."""
    from centernet_amd import native
    from centernet_amd.engine import Act
    with native.tuning(dict(knobs)):
        pb = _builder(dev, c, dtype)
        if c["kind"] == "stem":
            xa = pb.set_input(3)
            pb.input.t = x.float().to(dev)
        else:
            xa = Act(_nhwc(x, dev, dtype), c["B"], c["H"], c["W"], c["Cin"])
        ra = None
        if res is not None:
            ra = Act(_nhwc(res, dev, dtype), res.shape[0], res.shape[2], res.shape[3], res.shape[1])
        y = pb.conv(xa, w.float(), bias=bias, bn=bn, relu=c["relu"], residual=ra, stride=c["s"], padding=c["p"])
        assert y.t.dtype == dtype and not y.nchw and y.pitch == c["Cout"]
        outs = [y]
        off = 0
        for w2, b2 in lasts:      # as PlanBuilder.heads_from_convs slices the hidden layer
            hcn = w2.shape[1]
            sl = Act(y.t, y.B, y.H, y.W, hcn, pitch=y.pitch, c_off=off, fmt=y.fmt, exp=y.exp, lid=y.lid)
            z = pb.conv(sl, w2.float(), bias=b2, stride=1, padding=0, out_nchw=True)
            assert z.nchw and z.t.dtype == torch.float32
            outs.append(z)
            off += hcn
        for o in outs:
            o.t.fill_(float("nan"))
        for op in pb.ops:
            op()
        torch.cuda.synchronize()
    return [outs[0].t.permute(0, 3, 1, 2).cpu()] + [o.t.cpu() for o in outs[1:]]


# ---- A1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32mfma"])
@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_integer_operands_give_the_reference_exactly(dev, run, dtype):
    c, knobs, rid = run
    d = hc.int_case(c["id"])
    for name, ref in hc.int_refs(c["id"]):
        ok, top, nonzero = hc.exactness(ref)
        assert ok and nonzero >= 0.9, (rid, name, top, nonzero)
    lasts = tuple((w2, b2) for w2, b2, _ in d.get("lasts", ()))
    got = _launch(dev, c, knobs, dtype, d["x"], d["w"], d["bias"], d["bn"], d["res"], lasts)
    refs = [r for _, r in hc.int_refs(c["id"])]
    assert len(got) == len(refs)
    for i, (g, r) in enumerate(zip(got, refs)):
        want = r.to(g.dtype)
        assert g.shape == want.shape, (rid, i, g.shape, want.shape)
        bad = g != want
        assert torch.equal(g, want), "%s output %d: %d of %d values differ, first at %s: got %s, want %s" % (
            rid, i, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()),
            g[bad][:4].tolist(), want[bad][:4].tolist())


# ---- A2 ---------------------------------------------------------------------------------------------------
def _normal_operands(c):
    """Operands as test_fp16_conv_vs_fp32_reference draws them, rounded to fp16 (the shift stays fp32)."""
    B, Cin, H, W, Cout, k = (c[n] for n in ("B", "Cin", "H", "W", "Cout", "k"))
    x = (synth.images(B, H, W, 3) if c["kind"] == "stem" else
         torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 1))).half().float()
    w = torch.from_numpy(synth.normal((Cout, Cin, k, k), (2.0 / (Cin * k * k)) ** 0.5, 2)).half().float()
    bn = bias = res = None
    if c["bn"]:
        bn = torch.nn.BatchNorm2d(Cout)
        synth.fill_state_dict_(bn, 4)
        bn.eval()
    elif c["bias"]:
        bias = torch.from_numpy(synth.normal((Cout,), 0.3, 3))
    if c["res"]:
        Ho, Wo = hc.out_hw(c)
        res = torch.from_numpy(synth.normal((B, Cout, Ho, Wo), 1.0, 5)).half().float()
    return x, w, bias, bn, res


def _rounding_check(rid, name, got, ref, e32, fp16_out):
    """The A2 bar; returns the observed max((err - half-ulp term) / E32)."""
    assert e32 > 0
    err = (got.double() - ref).abs()
    half_ulp = (ref.abs() * 2.0 ** -11 + 2.0 ** -25) if fp16_out else torch.zeros_like(ref)
    ratio = float(((err - half_ulp) / e32).max())
    print("A2 %s/%s: E32 %.3e, max |err| %.3e, max (err - half-ulp) / E32 = %.3f" % (
        rid, name, e32, float(err.max()), ratio))
    assert not torch.isnan(got).any(), (rid, name)
    over = err > half_ulp + 4.0 * e32
    assert not bool(over.any()), "%s/%s: %d values beyond the bar, accumulation ratio %.3f" % (
        rid, name, int(over.sum()), ratio)
    return ratio


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_normal_operands_within_the_rounding_bar(dev, run):
    c, knobs, rid = run
    x, w, bias, bn, res = _normal_operands(c)
    lasts = ()
    if c["kind"] == "heads":
        lasts = tuple((torch.from_numpy(synth.normal((co, hc.HEAD_HIDDEN, 1, 1), 0.1, 7 + i)).half().float(),
                       torch.from_numpy(synth.normal((co,), 0.1, 17 + i))) for i, co in enumerate(hc.HEAD_COUTS))
    got = _launch(dev, c, knobs, torch.float16, x, w, bias, bn, res, lasts)
    args = (x, w, bias, bn, res, c["relu"], c["s"], c["p"])
    ref = hc.ref64(*args).detach()
    e32 = float((hc.ref32(*args).double() - ref).abs().max())
    _rounding_check(rid, "y", got[0], ref, e32, True)
    # each 1x1 head against a reference on ITS input: the fp16 hidden layer the first launch wrote
    for i, ((w2, b2), z) in enumerate(zip(lasts, got[1:])):
        mid = got[0][:, i * hc.HEAD_HIDDEN:(i + 1) * hc.HEAD_HIDDEN].float()
        a2 = (mid, w2, b2, None, None, False, 1, 0)
        r2 = hc.ref64(*a2)
        e2 = float((hc.ref32(*a2).double() - r2).abs().max())
        _rounding_check(rid, "map%d" % w2.shape[0], z, r2, e2, False)
