"""The MFMA shape of the persistent 3x3 kernel's generic consumers that is NOT the default (csrc/cn_conv3x3p.hip,
template S16; cn_set_tuning key 30 bit 2 = v_mfma_f32_32x32x16_f16 where the default is v_mfma_f32_16x16x32_f16).

The default shape runs in every other suite (test_gpu_c3p_items.py, test_gpu_conv.py, the network tests); the other
one stays in the library as the A/B arm and runs only here.  The cases, operands and float64 references are those
of tests/c3p_cases.py at caps 64, 3 and 1 with key 28 = 2 -- the smallest shapes with edge tiles, a half-empty
output block, three chunks and item boundaries -- on every generic form (3x3 / s1 without / with an f32s / plain
residual, f32s and plain output; stride 2; transposed), with key 30 = 4 (unpipelined schedule) and 6 (pipelined):

* exact-integer operands: the result EQUALS the float64 result;
* normal data: within 2e-5 * (1 + |ref|) of float64 (the bar of test_gpu_c3p_items.py);
* the raw tensors are bit-identical between key 30 = 4 and 6, across caps, and over a second run;
* the two shapes (key 30 = 6 against the default 2) agree within that same bar: they differ only in the order
  in which an MFMA sums its K products.

Outputs are poisoned before every run, as test_gpu_c3p_items.py does.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c3p_cases as cc   # noqa: E402
import test_gpu_c3p_items as items   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = items.TOL
KNOBS = (4, 6)            # key 30: the 32x32x16 shape, unpipelined / pipelined
IDS = [c["id"] for c in cc.CASES if c["form"] != "heads"]     # (the fused heads have one shape)
_RUNS = {}                # (case, kind, residual, plain output, cap, key 30) -> (raw int32, values fp32, second run equal)


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _result(dev, cid, kind, res, out_plain, cap, knobs):
    key = (cid, kind, res, out_plain, cap, knobs)
    if key not in _RUNS:
        from centernet_amd import native
        c = cc.case(cid)
        with native.tuning({**c["keys"], 28: 2, 47: cap, 30: knobs}):
            pb, (act,) = items._build(dev, c, cc.data(cid, kind), res, out_plain)
            (raw,) = items._run_once(pb, [act])
            val = act.to_float().cpu()
            (again,) = items._run_once(pb, [act])
        _RUNS[key] = (raw, val, bool(torch.equal(raw, again)))
    return _RUNS[key]


def _ref(c, d, res):
    return d["ref"][res is not None].permute(0, 2, 3, 1)


@pytest.mark.parametrize("cid", IDS)
def test_integer_operands_equal_float64(dev, cid):
    c, d = cc.case(cid), cc.int_case(cid)
    for res, out_plain in cc.variants(c):
        for cap in cc.CAPS:
            for knobs in KNOBS:
                _, val, _ = _result(dev, cid, "int", res, out_plain, cap, knobs)
                bad = val.double() != _ref(c, d, res)            # (NaN != ref: unwritten outputs count)
                assert not bool(bad.any()), "%s cap %d key 30 = %d residual %s plain %s: %d of %d outputs differ" % (
                    cid, cap, knobs, res, out_plain, int(bad.sum()), bad.numel())


@pytest.mark.parametrize("cid", IDS)
def test_normal_data_within_fp32_rounding_of_float64(dev, cid):
    c, d = cc.case(cid), cc.normal_case(cid)
    for res, out_plain in cc.variants(c):
        ref = _ref(c, d, res)
        for cap in cc.CAPS:
            for knobs in KNOBS:
                _, val, _ = _result(dev, cid, "normal", res, out_plain, cap, knobs)
                err = (val.double() - ref).abs() / (1 + ref.abs())
                worst = float(err.max()) if not bool(torch.isnan(err).any()) else float("nan")
                print("%s cap %d key 30 = %d residual %s plain %s: max |y - ref| / (1 + |ref|) = %.3e"
                      % (cid, cap, knobs, res, out_plain, worst))
                assert worst < TOL, (cid, cap, knobs, res, out_plain, worst)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("cid", IDS)
def test_raw_output_is_one_for_both_schedules_every_cap_and_a_second_run(dev, cid, kind):
    c = cc.case(cid)
    for res, out_plain in cc.variants(c):
        raw0, _, _ = _result(dev, cid, kind, res, out_plain, 64, KNOBS[0])
        for cap in cc.CAPS:
            for knobs in KNOBS:
                raw, _, same = _result(dev, cid, kind, res, out_plain, cap, knobs)
                assert same, "%s cap %d key 30 = %d residual %s plain %s: not deterministic run to run" % (
                    cid, cap, knobs, res, out_plain)
                n = int((raw != raw0).sum())
                assert n == 0, "%s cap %d key 30 = %d residual %s plain %s: %d words differ from cap 64, key 30 = %d" % (
                    cid, cap, knobs, res, out_plain, n, KNOBS[0])


@pytest.mark.parametrize("cid", IDS)
def test_the_two_shapes_agree(dev, cid):
    """key 30 = 6 against key 30 = 2 (the default shape, same schedule) on normal data."""
    c, d = cc.case(cid), cc.normal_case(cid)
    for res, out_plain in cc.variants(c):
        ref = _ref(c, d, res)
        _, a, _ = _result(dev, cid, "normal", res, out_plain, 64, 6)
        _, b, _ = _result(dev, cid, "normal", res, out_plain, 64, 2)
        err = (a.double() - b.double()).abs() / (1 + ref.abs())
        worst = float(err.max()) if not bool(torch.isnan(err).any()) else float("nan")
        print("%s residual %s plain %s: max |y(32x32x16) - y(16x16x32)| / (1 + |ref|) = %.3e" % (cid, res, out_plain, worst))
        assert worst < TOL, (cid, res, out_plain, worst)
