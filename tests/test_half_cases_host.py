"""The exact-integer cases of tests/test_gpu_half.py, checked on the CPU: the float64 reference alone
must meet the exactness condition the bit comparison rests on -- every value an fp16 number with
|y| <= 2048 -- and at least 90 % of the outputs must be non-zero, so that ReLU (or an unlucky shift)
does not blank the comparison.  Runs without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import half_cases as hc   # noqa: E402


@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES])
def test_integer_case_reference_is_exact_and_dense(cid):
    for name, ref in hc.int_refs(cid):
        ok, top, nonzero = hc.exactness(ref)
        print("%s/%s: max |y| %.1f, non-zero %.3f" % (cid, name, top, nonzero))
        assert ok, (cid, name, top)
        assert nonzero >= 0.9, (cid, name, nonzero)


@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES])
def test_integer_case_operands_are_fp16_numbers(cid):
    """Inputs, weights, residual, and the (scale, shift) fold_bn derives from the BatchNorm: all exact in
    fp16 / as small multiples of 1/2 in fp32."""
    from centernet_amd.engine import fold_bn
    d = hc.int_case(cid)
    for name in ("x", "w", "res", "bias"):
        t = d[name]
        if t is not None:
            assert torch.equal(t.half().float(), t) and torch.equal(t, t.round()), name
    if d["bn"] is not None:
        scale, shift = fold_bn(None, d["bn"], d["w"].shape[0], torch.device("cpu"))
        assert set(scale.tolist()) <= {1.0, 2.0, -1.0, 0.5}
        assert torch.equal(shift * 2, (shift * 2).round()) and float(shift.abs().max()) <= 512


def test_every_form_is_listed_once():
    ids = [c["id"] for c in hc.CASES]
    assert len(set(ids)) == len(ids)
    assert all(c["form"] and c["variants"] for c in hc.CASES)
    assert len({rid for _, _, rid in hc.runs()}) == len(hc.runs())
