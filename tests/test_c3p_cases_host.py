"""The case list of tests/test_gpu_c3p_items.py, checked on the CPU against the schedule mirror of
tests/c3p_cases.py: at caps below 64 the cases reach the item boundaries of the persistent 3x3 kernel
(csrc/cn_conv3x3p.hip) that the default grid never reaches at a test-sized shape -- and the integer cases meet
the exactness condition their bit comparison rests on.  Runs without a GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c3p_cases as cc   # noqa: E402

LOW = [cap for cap in cc.CAPS if cap < 64]


def _launches(form, caps=LOW):
    """(case, args, cap, item list per workgroup) of every launch of a form."""
    for c in cc.CASES:
        if c["form"] == form:
            a = cc.p3_args(c)
            for cap in caps:
                yield c, a, cap, cc.workgroup_items(a, cap)


def _boundaries(form):
    """(args, decoded item, decoded next item) of every item boundary inside a workgroup."""
    for _, a, _, wgs in _launches(form):
        for items in wgs:
            for i, j in zip(items, items[1:]):
                yield a, cc.p3_decode(a, i), cc.p3_decode(a, j)


def test_case_list_is_the_one_described():
    assert cc.CAPS == (64, 3, 1) and set(c["form"] for c in cc.CASES) == set(cc.FORMS)
    ids = [c["id"] for c in cc.CASES]
    assert len(set(ids)) == len(ids)
    got = {c["id"]: (cc.p3_args(c)["items"], cc.p3_args(c)["nchunk"]) for c in cc.CASES}
    assert got == {"s1_96_20x40": (54, 3), "s1_32_17x33": (18, 1), "s1_64_16x32": (16, 2), "s1_32_24x16": (15, 1),
                   "deconv_96_9x20": (96, 3), "deconv_32_8x40": (12, 1), "s2_32_35x45": (36, 1),
                   "s2_96_32x64": (24, 3), "heads_64_20x24": (36, 2), "heads_96_17x40": (45, 3),
                   "heads_32_16x32": (24, 1)}


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c["id"])
def test_every_item_is_walked_exactly_once(c):
    """The mirror itself: at every cap the workgroups' lists partition 0 ... items - 1, the grid is a multiple of
    8 with at most one workgroup per item, and decoding is a bijection onto (image, tile, parity, block)."""
    a = cc.p3_args(c)
    for cap in cc.CAPS:
        wgs = cc.workgroup_items(a, cap)
        assert len(wgs) == cc.grid(a, cap) and len(wgs) % 8 == 0 and len(wgs) <= 8 * cap
        assert sorted(i for w in wgs for i in w) == list(range(a["items"]))
    seen = {tuple(sorted(cc.p3_decode(a, i).items())) for i in range(a["items"])}
    assert len(seen) == a["items"]
    d = cc.p3_decode(a, a["items"] - 1)
    assert (d["b"], d["ty"], d["tx"], d["par"], d["nb"]) == \
        (c["B"] - 1, a["tiles_y"] - 1, a["tiles_x"] - 1, a["npar"] - 1, a["nblk"] - 1)


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c["id"])
def test_default_cap_gives_one_item_per_workgroup(c):
    """The gap, stated: at cap 64 no workgroup of any case has a second item."""
    assert max(len(w) for w in cc.workgroup_items(cc.p3_args(c), 64)) <= 1


def test_one_xcd_share_at_cap_1():
    """With cap 1 a launch has 8 workgroups, each its XCD's whole contiguous share."""
    c = cc.case("s1_96_20x40")
    wgs = cc.workgroup_items(cc.p3_args(c), 1)
    assert [len(w) for w in wgs] == [7] * 7 + [5] and wgs[1] == list(range(7, 14))
    assert [len(w) for w in cc.workgroup_items(cc.p3_args(cc.case("s1_32_17x33")), 1)] == [3] * 6 + [0, 0]
    assert [len(w) for w in cc.workgroup_items(cc.p3_args(cc.case("s2_32_35x45")), 1)] == [5] * 7 + [1]
    assert [len(w) for w in cc.workgroup_items(cc.p3_args(cc.case("deconv_96_9x20")), 1)] == [12] * 8


@pytest.mark.parametrize("form", cc.FORMS)
def test_low_caps_reach_the_item_loop(form):
    launches = list(_launches(form))
    nits = [[len(w) for w in wgs] for _, _, _, wgs in launches]
    assert any(max(n) >= 3 for n in nits)
    assert any(len(set(n)) > 1 for n in nits), "workgroups of unequal nit in one launch"
    assert any(0 in n for n in nits), "a workgroup without items"
    for nchunk in (1, 3):
        assert any(a["nchunk"] == nchunk and max(len(w) for w in wgs) >= 2 for _, a, _, wgs in launches), nchunk
    if form != "deconv":        # 4 * nchunk steps: the ring phase of the transposed form never moves
        assert all(cc.steps_per_item(c) % 4 for c, _, _, _ in launches)


@pytest.mark.parametrize("form", cc.FORMS)
def test_low_caps_reach_every_kind_of_item_change(form):
    kinds = set()
    for a, p, q in _boundaries(form):
        same_tile = (p["b"], p["ty"], p["tx"]) == (q["b"], q["ty"], q["tx"])
        if same_tile and p["par"] == q["par"] and p["nb"] != q["nb"]:
            kinds.add("block only")
        if p["b"] == q["b"] and p["ty"] != q["ty"]:
            kinds.add("tile row")
        if p["b"] != q["b"]:
            kinds.add("image")
        if p["par"] != q["par"]:
            kinds.add("parity")
    want = {"block only", "tile row", "image"} | ({"parity"} if form == "deconv" else set())
    assert kinds == want, (form, sorted(want - kinds))


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c["id"])
def test_every_case_is_one_the_kernel_takes(c):
    for res, out_plain in cc.variants(c):
        assert cc.takes(c, res, out_plain), (c["id"], res, out_plain)
    if c["form"] == "heads":
        assert cc.HIDDEN == 64


@pytest.mark.parametrize("cid", [c["id"] for c in cc.CASES])
def test_integer_case_is_exact(cid):
    """Every partial sum is an integer below 2^24 (exact in the fp32 accumulator whatever the order; the
    power-of-two weight prescale moves the exponent only), every stored value fits the high half of an f32s
    pair, every operand is an fp16 number -- and ReLU does not blank the comparison."""
    e = cc.int_exactness(cid)
    print(cid, e)
    assert e["sum_abs"] < 2 ** 24 and e["top"] <= 65504, e
    assert e["operands_exact"] and e["rows_nonzero"], e
    assert e["nonzero"] >= 0.75, e
