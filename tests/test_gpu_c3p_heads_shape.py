"""The fused heads of the persistent 3x3 kernel (csrc/cn_conv3x3p.hip, template HEADS) in both MFMA shapes against a
float64 reference: v_mfma_f32_16x16x32_f16 (the default, cn_set_tuning key 30 = 2) and v_mfma_f32_32x32x16_f16
(key 30 = 6).  Both read the same packed 1x1 buffer (cn_pack_head_w2_f32s); the 16x16x32 form runs the 1x1 GEMM in
cdiv(outputs, 16) blocks of 16 rows, the 32x32x16 form in blocks of 32.

Cases: the `heads` cases of tests/c3p_cases.py, and two maps of B = 2, 64 input channels with heads of 1, 2, 17, 80
and 96 outputs (one and two rows, a block of 16 and one row, five blocks of 16 = 2.5 of 32, the largest a head may
have): 8 x 16 = ONE tile per image, and 9 x 17 = four tiles with a ragged bottom row and right column.  Every case runs at caps
(key 47) 64, 3 and 1 under key 28 = 2.

* exact-integer operands: both shapes EQUAL the float64 result, every output of every image;
* normal data: within 2e-5 * (1 + |ref|) of float64 (the bar of test_gpu_c3p_items.py);
* outputs are filled with NaN before every launch, and a second launch repeats the first bit for bit.
The two shapes sum in different orders and need not be bit-equal to each other.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c3p_cases as cc   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-5
SHAPES = {"16x16x32": 2, "32x32x16": 6}          # key 30
COUTS = (1, 2, 17, 80, 96)
_EDGE_HEADS = [("h%d" % co, co, co != 17) for co in COUTS]
EDGE = [dict(id="heads_64_8x16", form="heads", B=2, Cin=64, H=8, W=16, Cout=0, keys={}, heads=_EDGE_HEADS),
        dict(id="heads_64_9x17", form="heads", B=2, Cin=64, H=9, W=17, Cout=0, keys={}, heads=_EDGE_HEADS)]
CASES = [c for c in cc.CASES if c["form"] == "heads"] + EDGE
IDS = [c["id"] for c in CASES]
_RUNS = {}


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _case(cid):
    return next(c for c in CASES if c["id"] == cid)


@functools.lru_cache(maxsize=None)
def _data(cid, kind):
    """dict(x, pairs, refs) -- the shared cases: those of c3p_cases; the edge cases: by the same recipes."""
    if cid in [c["id"] for c in cc.CASES]:
        return cc.data(cid, kind)
    from centernet_amd import synth
    c = _case(cid)
    if kind == "int":
        rng = np.random.RandomState(5100 + IDS.index(cid))
        x = cc._ints(rng, (c["B"], c["Cin"], c["H"], c["W"]), 0, 3)
        pairs = cc._head_modules(c, rng=rng)
    else:
        x = torch.from_numpy(synth.normal((c["B"], c["Cin"], c["H"], c["W"]), 1.0, 11)).relu_()
        pairs = cc._head_modules(c, seed=c["B"] + c["H"])
    return dict(x=x, pairs=pairs, refs=cc._head_refs(x, pairs))


def _result(dev, cid, kind, shape, cap):
    """[(values (B, H, W, C) fp32, second launch bit-equal)] per head, outputs NaN-filled before each launch"""
    key = (cid, kind, shape, cap)
    if key not in _RUNS:
        from centernet_amd import native
        from centernet_amd.engine import Act, PlanBuilder
        c, d = _case(cid), _data(cid, kind)
        with native.tuning({28: 2, 47: cap, 30: SHAPES[shape]}):
            pb = PlanBuilder(dev, c["B"], c["H"], c["W"], split=True)
            x = d["x"]
            xin = pb.packed(Act(x.permute(0, 2, 3, 1).contiguous().to(dev), c["B"], c["H"], c["W"], c["Cin"]))
            outs = pb.heads_from_convs(xin, d["pairs"])
            acts = [outs[n] for n, _, _ in c["heads"]]
            assert len(pb.ops) == 2 and all(a.nchw for a in acts), "convert + one fused launch"
            raws = []
            for _ in range(2):
                for a in acts:
                    a.t.fill_(float("nan"))
                for op in pb.ops:
                    op()
                torch.cuda.synchronize()
                raws.append([a.t.view(torch.int32).cpu() for a in acts])
            vals = [a.to_float().cpu() for a in acts]
        _RUNS[key] = [(v, bool(torch.equal(r0, r1))) for v, r0, r1 in zip(vals, raws[0], raws[1])]
    return _RUNS[key]


def _refs(c, d):
    return [d["refs"][n][1].permute(0, 2, 3, 1) for n, _, _ in c["heads"]]


def test_the_edge_cases_sum_exactly():
    """what the bit comparison of the two added maps rests on: fp16-exact operands, and every sum of magnitudes of
    both layers below 2^24 (test_c3p_cases_host.py shows the same for the shared cases)"""
    import torch.nn.functional as F
    from centernet_amd.engine import prescale_rows
    for c in EDGE:
        d = _data(c["id"], "int")
        x = d["x"]
        assert bool(torch.equal(x.half().float(), x))
        for n, (c1, c2) in d["pairs"].items():
            hid, ref = d["refs"][n]
            w1, w2 = c1.weight.detach(), c2.weight.detach()
            for w in (w1, w2):
                assert bool(torch.equal(w.half().float(), w))
                ws = prescale_rows(w.flatten(1))[0]
                assert bool(torch.equal(ws.half().float(), ws))
            s1 = F.conv2d(x.double().abs(), w1.double().abs(), None, 1, 1) + c1.bias.detach().double().abs().view(1, -1, 1, 1)
            s2 = F.conv2d(hid.abs(), w2.double().abs())
            assert max(float(s1.max()), float(s2.max())) + 8 < 2 ** 24
            assert float((ref != 0).double().mean()) > 0.5


@pytest.mark.parametrize("cap", cc.CAPS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("cid", IDS)
def test_integer_operands_equal_float64_in_both_shapes(dev, cid, shape, cap):
    c, d = _case(cid), _data(cid, "int")
    for (name, co, _), (val, same), ref in zip(c["heads"], _result(dev, cid, "int", shape, cap), _refs(c, d)):
        assert same, "%s %s cap %d head %s: a second launch differs" % (cid, shape, cap, name)
        bad = val.double() != ref                # (NaN != ref: unwritten outputs count)
        if bool(bad.any()):
            where = bad.nonzero()
            b, y, x, ch = where[0].tolist()
            pytest.fail("%s %s cap %d head %s (%d outputs): %d of %d values differ, first at image %d pixel (%d, %d) row "
                        "%d: %r, float64 %r" % (cid, shape, cap, name, co, len(where), bad.numel(), b, y, x, ch,
                                                float(val[b, y, x, ch]), float(ref[b, y, x, ch])))


@pytest.mark.parametrize("cap", cc.CAPS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("cid", IDS)
def test_normal_data_within_fp32_rounding_of_float64_in_both_shapes(dev, cid, shape, cap):
    c, d = _case(cid), _data(cid, "normal")
    for (name, co, _), (val, same), ref in zip(c["heads"], _result(dev, cid, "normal", shape, cap), _refs(c, d)):
        assert same, "%s %s cap %d head %s: a second launch differs" % (cid, shape, cap, name)
        err = (val.double() - ref).abs() / (1 + ref.abs())
        worst = float(err.max()) if not bool(torch.isnan(err).any()) else float("nan")
        print("%s %s cap %d head %s: max |y - ref| / (1 + |ref|) = %.3e" % (cid, shape, cap, name, worst))
        assert worst < TOL, (cid, shape, cap, name, worst)
