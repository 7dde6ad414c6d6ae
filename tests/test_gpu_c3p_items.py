"""The item loop of the persistent 3x3 kernel (csrc/cn_conv3x3p.hip) against a float64 reference.

The launchers size the grid as 8 * min(ceil(items / 8), key 47): at the default cap of 64 every launch of up to
512 items gives a workgroup ONE item, so no test-sized shape runs the code at an item boundary -- the halo cursor
that moves on while the epilogue runs, the weight block (set_wofs) and parity (wpar) refreshed at an item change,
the halo buffer (stage & 1) and ring slot (g & 3) that run on across items, the epilogue strips that alias a halo
buffer.  Here every form (3x3 / s1 without / with an f32s / plain residual, f32s and plain output; stride 2;
ConvTranspose 4x4 / 2; the fused heads) runs the cases of tests/c3p_cases.py at caps 64, 3 and 1 (key 28 = 2
forces the kernel onto small shapes); tests/test_c3p_cases_host.py shows on the CPU which boundaries they reach.

* exact-integer operands: the result EQUALS the float64 result, every output of every image;
* normal data with a folded BatchNorm: within 2e-5 * (1 + |ref|) of float64, every image;
* the raw output tensors at caps 3 and 1 are bit-identical to those at cap 64 and over a second run;
* the loaders' stage count per workgroup (instrumented instantiation) is the mirror's nit * nchunk.

Largest normal-data error against float64 seen on the MI355X, |y - ref| / (1 + |ref|): 3x3 / s1 2.7e-6, stride 2
1.9e-6, transposed 1.1e-6, heads 1.5e-6 (printed per run).

Outputs are filled before every run with a pattern no run produces (NaN; an f32s pair that decodes to 60000):
an unwritten tile cannot pass as a ReLU zero.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c3p_cases as cc   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-5                # the bar of test_gpu_conv.py: |y - ref| <= TOL * (1 + |ref|)
IDS = [c["id"] for c in cc.CASES]
_RUNS = {}                # (case, kind, residual, plain output, cap) -> [(raw int32, values fp32, second run equal)]
_WORST = {}               # form -> largest normal-data error seen (printed)


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _keys(c, cap):
    return {**c["keys"], 28: 2, 47: cap}


def _nhwc_act(x, dev):
    from centernet_amd.engine import Act
    B, C, H, W = x.shape
    return Act(x.permute(0, 2, 3, 1).contiguous().to(dev), B, H, W, C)


def _build(dev, c, d, res, out_plain):
    """The case as a plan: (builder, output activations)."""
    from centernet_amd.engine import PlanBuilder
    pb = PlanBuilder(dev, c["B"], c["H"], c["W"], split=True)
    xin = pb.packed(_nhwc_act(d["x"], dev))
    if c["form"] == "heads":
        outs = pb.heads_from_convs(xin, d["pairs"])
        acts = [outs[n] for n, _, _ in c["heads"]]
        assert len(pb.ops) == 2 and all(a.nchw for a in acts), "convert + one fused launch"
        return pb, acts
    if c["form"] == "deconv":
        y = pb.conv_transpose4x4s2(xin, d["w"], bn=d["bn"], relu=True, out_plain=out_plain)
    else:
        r = None
        if res is not None:
            r = _nhwc_act(d["res"], dev)
            pb.keep.append(r.t)        # (the launch holds the residual's address only)
            r = pb.packed(r) if res == "f32s" else r
            assert r.fmt == ("f32s" if res == "f32s" else "f32")
        y = pb.conv(xin, d["w"], bias=d["bias"], bn=d["bn"], relu=True, stride=2 if c["form"] == "s2" else 1,
                    padding=1, residual=r, out_plain=out_plain)
    assert y.fmt == ("f32" if out_plain else "f32s") and (y.H, y.W) == cc.out_hw(c) and y.pitch == c["Cout"]
    return pb, [y]


def _poison(act):
    if act.fmt == "f32s":
        act.t.view(torch.float16).fill_(30000.0)      # (high, low) = (30000, 30000)
    else:
        act.t.fill_(float("nan"))


def _run_once(pb, acts):
    for a in acts:
        _poison(a)
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    return [a.t.view(torch.int32).cpu() for a in acts]


def _result(dev, cid, kind, res, out_plain, cap):
    key = (cid, kind, res, out_plain, cap)
    if key not in _RUNS:
        from centernet_amd import native
        c = cc.case(cid)
        with native.tuning(_keys(c, cap)):
            pb, acts = _build(dev, c, cc.data(cid, kind), res, out_plain)
            raws = _run_once(pb, acts)
            vals = [a.to_float().cpu() for a in acts]             # (B, H, W, C)
            again = _run_once(pb, acts)
        _RUNS[key] = [(r, v, bool(torch.equal(r, r2))) for r, v, r2 in zip(raws, vals, again)]
    return _RUNS[key]


def _refs(c, d, res):
    """Float64 references, (B, H, W, C), in the order of the output activations."""
    if c["form"] == "heads":
        return [d["refs"][n][1].permute(0, 2, 3, 1) for n, _, _ in c["heads"]]
    return [d["ref"][res is not None].permute(0, 2, 3, 1)]


@pytest.mark.parametrize("cap", cc.CAPS)
@pytest.mark.parametrize("cid", IDS)
def test_integer_operands_equal_float64(dev, cid, cap):
    """x in 0 ... 3, weights in {-1, 0, 1}, integer biases and residual, ReLU: every partial sum is exact
    (test_c3p_cases_host.py), so a lost, doubled or misplaced term, tile or weight block changes a value."""
    c, d = cc.case(cid), cc.int_case(cid)
    for res, out_plain in cc.variants(c):
        got = _result(dev, cid, "int", res, out_plain, cap)
        for (_, val, _), ref in zip(got, _refs(c, d, res)):
            bad = val.double() != ref            # (NaN != ref: unwritten outputs count)
            if bool(bad.any()):
                where = bad.nonzero()
                b, y, x, ch = where[0].tolist()
                pytest.fail("%s cap %d residual %s plain %s: %d of %d outputs differ, first at image %d pixel (%d, %d) "
                            "channel %d: %r, float64 %r" % (cid, cap, res, out_plain, len(where), bad.numel(), b, y,
                                                            x, ch, float(val[b, y, x, ch]), float(ref[b, y, x, ch])))


@pytest.mark.parametrize("cap", cc.CAPS)
@pytest.mark.parametrize("cid", IDS)
def test_normal_data_within_fp32_rounding_of_float64(dev, cid, cap):
    c, d = cc.case(cid), cc.normal_case(cid)
    for res, out_plain in cc.variants(c):
        got = _result(dev, cid, "normal", res, out_plain, cap)
        for (_, val, _), ref in zip(got, _refs(c, d, res)):
            err = (val.double() - ref).abs() / (1 + ref.abs())
            worst = float(err.max()) if not bool(torch.isnan(err).any()) else float("nan")
            _WORST[c["form"]] = max(_WORST.get(c["form"], 0.0), worst)
            print("%s cap %d residual %s plain %s: max |y - ref| / (1 + |ref|) = %.3e (form %s so far %.3e)"
                  % (cid, cap, res, out_plain, worst, c["form"], _WORST[c["form"]]))
            assert worst < TOL, (cid, cap, res, out_plain, worst)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("cid", IDS)
def test_output_does_not_depend_on_the_item_to_workgroup_map(dev, cid, kind):
    """An item's summation order does not depend on which workgroup computes it, nor on what that workgroup did
    before: the raw tensors at caps 3 and 1 are those of cap 64, bit for bit, and each run repeats itself."""
    c = cc.case(cid)
    for res, out_plain in cc.variants(c):
        base = _result(dev, cid, kind, res, out_plain, 64)
        for cap in cc.CAPS:
            got = _result(dev, cid, kind, res, out_plain, cap)
            for i, ((raw, _, same), (raw0, _, _)) in enumerate(zip(got, base)):
                assert same, "%s cap %d residual %s plain %s output %d: not deterministic run to run" \
                    % (cid, cap, res, out_plain, i)
                n = int((raw != raw0).sum())
                assert n == 0, "%s cap %d residual %s plain %s output %d: %d words differ from cap 64" \
                    % (cid, cap, res, out_plain, i, n)


def test_schedule_mirror_matches_the_device(dev):
    """The 3x3 / s1 cases without a residual, f32s output, on the instrumented instantiation
    (cn_conv3x3p_probe): the stage count both loader waves of every workgroup report is nit * nchunk of the
    mirror at caps 64, 3 and 1, workgroups without items and beyond the grid report nothing -- so the kernel
    that ran is the persistent one, on the grid and with the item lists test_c3p_cases_host.py reasons about."""
    from centernet_amd import native
    lib = native.lib()
    lib.cn_conv3x3p_probe.argtypes = [ctypes.c_int, ctypes.c_void_p]
    prof = torch.zeros((512, 6, 8), device=dev, dtype=torch.int64)
    try:
        for c in (k for k in cc.CASES if k["form"] == "s1"):
            a, d = cc.p3_args(c), cc.int_case(c["id"])
            for cap in cc.CAPS:
                with native.tuning(_keys(c, cap)):
                    pb, acts = _build(dev, c, d, None, False)
                    prof.zero_()
                    assert lib.cn_conv3x3p_probe(0, prof.data_ptr()) == 0
                    _run_once(pb, acts)
                    assert lib.cn_conv3x3p_probe(0, None) == 0
                want = [len(w) * a["nchunk"] for w in cc.workgroup_items(a, cap)]
                want += [0] * (512 - len(want))
                got = prof.cpu()
                for wave in (4, 5):
                    assert got[:, wave, 3].tolist() == want, (c["id"], cap, wave)
                assert bool(torch.equal(acts[0].to_float().cpu().double(), _refs(c, d, None)[0])), (c["id"], cap)
    finally:
        lib.cn_conv3x3p_probe(0, None)
