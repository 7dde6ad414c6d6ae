"""What tests/test_gpu_dcn_half.py relies on, checked without a GPU: the A1 conditions of tests/dcn_half_cases.py,
its float64 reference against oracle's C deformable convolution, the routes cn_dcn_v2_route_f16 gives half calls,
the fp32 / f32s routes against the recorded ones, and the --fp16 option."""
import ctypes
import importlib.util
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as dh   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["id"] for c in dh.CASES]


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


@pytest.mark.parametrize("cid", IDS)
def test_a1_reference_is_exact_in_fp16_and_mostly_nonzero(cid):
    ok, top, nonzero = dh.exactness(dh.int_case(cid)["ref"])
    assert ok and nonzero >= 0.9, (cid, top, nonzero)


def test_a1_operands_are_what_the_argument_needs():
    for cid in IDS:
        d = dh.int_case(cid)
        assert set(d["x"].unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert set(d["w"].unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert set(d["mask"].unique().tolist()) <= {0.0, 0.5, 1.0}
        assert set(d["scale"].unique().tolist()) <= {1.0, 2.0, -1.0, 0.5}
        assert bool(((d["off"] * 2).round() == d["off"] * 2).all())
        assert bool((d["shift"].round() == d["shift"]).all()) and bool((d["bias"].round() == d["bias"]).all())
    # the stress set is there: samples exactly at -1 and at H / W, +-3 / +-3.5 (window reach), +-40 (far)
    for cid in ("win_stress", "gat_stress"):
        c, d = dh.case(cid), dh.int_case(cid)
        off = d["off"]
        for v in (3.0, -3.0, 3.5, -3.5, 40.0, -40.0):
            assert bool((off == v).any()), (cid, v)
        oy = torch.arange(c["H"]).view(1, c["H"], 1).float()
        h_im = torch.stack([oy - 1 + tap // 3 + off[:, 2 * tap] for tap in range(9)])
        assert bool((h_im == -1).any()) and bool((h_im == c["H"]).any()) and bool((h_im == c["H"] - 1).any())


def test_transposed_conv_and_pool_a1_conditions():
    for i in range(len(dh.DECONV_CASES)):
        ok, top, nonzero = dh.exactness(dh.deconv_int_case(i)["ref"])
        assert ok and nonzero >= 0.9, (i, top, nonzero)


@pytest.mark.parametrize("cid", IDS)
def test_float64_reference_agrees_with_the_c_oracle(cid):
    """fp32 rounding apart: E32 = max |C oracle - ref64| is a few fp32 ulps of the accumulated magnitude
    sum |w| |cols| (2^-24 per operation, K = 9 * Cin of them bounded by 8 sqrt(K) in practice)."""
    d = dh.normal_case(cid)
    c = dh.case(cid)
    K = 9 * c["Cin"]
    mag = float((dh.sample_term(d["w"], d["cols"], d["scale"]) * 2.0 ** 11).max()) + float(d["ref"].abs().max())
    assert 0 < d["e32"] <= 8 * K ** 0.5 * 2.0 ** -24 * mag, (cid, d["e32"], mag)
    # the float64 columns are the oracle's im2col
    from oracle import cref
    cols32 = cref.dcn_v2_im2col(d["x"][0].numpy(), d["off"][0].numpy(), d["mask"][0].numpy())
    err = (torch.from_numpy(cols32).double().reshape(d["cols"].shape[1], -1) - d["cols"][0]).abs().max()
    assert float(err) < 1e-5, (cid, float(err))


def _route(lib, c, ws=False, Cin=None, keys=None):
    from centernet_amd import native
    B, Cin, H, W, Cout = c["B"], Cin or c["Cin"], c["H"], c["W"], c["Cout"]
    info = native.DcnRouteInfo()
    slabs = 9 * 4 * B * H * W * ((Cout + 31) // 32 * 32)
    a = 0x10000000
    with native.tuning(dict(c["keys"] if keys is None else keys)):
        rc = lib.cn_dcn_v2_route_f16(a, 2 * a, 3 * a, 4 * a, 32, 5 * a, 6 * a, 7 * a, Cout + c["pad"], B, Cin, H, W,
                                     Cout, 0, int(c["relu"]), 8 * a if ws else None, slabs if ws else 0, None,
                                     ctypes.byref(info))
    return rc, info


@pytest.mark.parametrize("cid", IDS)
def test_half_calls_are_routed(cid):
    """cn_dcn_v2_route_f16, the host query of the half entry (the parent commit has neither), names the form."""
    from centernet_amd import native
    c = dh.case(cid)
    rc, info = _route(native.lib(), c, ws=c["ws"])
    assert rc == 0, rc
    want = {"window": native.DCNH_WINDOW, "gather": native.DCN_GATHER, "gather_pad": native.DCN_GATHER_PAD}[c["form"]]
    assert info.form == want, (cid, native.dcn_form_name(info.form))
    if c["form"] == "window":
        assert info.ksplit == 1 and info.grid_x == c["B"] * (c["H"] // 8) * (c["W"] // 16)
        assert info.grid_y == 1      # one block of 64 or 128 output channels in every case of the list
        # by default a grid this small is the gather form's (its tap split fills the chip), forced off as well
        for keys in ({}, dh.GATHER_KEYS):
            rc, d = _route(native.lib(), c, keys=keys)
            assert rc == 0 and d.form == native.DCN_GATHER
    if cid == "gat_split":
        assert info.ksplit > 1
    if cid == "gat_nosplit":
        assert info.ksplit == 1


def test_half_route_fills_the_chip_with_the_window_form_and_refuses_odd_channels():
    from centernet_amd import native
    lib = native.lib()
    big = dict(B=32, Cin=128, H=64, W=64, Cout=64, pad=0, relu=1, keys={})      # resdcn_18's last deformable layer
    rc, info = _route(lib, big)
    assert rc == 0 and info.form == native.DCNH_WINDOW and info.grid_x * info.grid_y == 1024
    rc, info = _route(lib, dict(big, B=1))                    # 32 tiles: gather
    assert rc == 0 and info.form == native.DCN_GATHER
    assert _route(lib, big, Cin=68)[0] == -2                  # Cin % 8 != 0: CN_ERR_UNSUPPORTED
    assert _route(lib, big, Cin=36)[0] == -2
    rc, info = _route(lib, big, Cin=72)                       # whole 16-byte corners, partial chunk
    assert rc == 0 and info.form == native.DCN_GATHER_PAD


def test_fp32_and_f32s_routes_are_the_parents():
    """Over the grid tests/test_dcn_route_host.py walks (tests/golden/gen_dcn_routes.py), every answer to an fp32 and
    an f32s call -- form, grid, K split, flags, workspace query -- is the one tests/golden/dcn_routes.json records.
    The file is the parent commit's, untouched: its refused calls hold too, the CN_DTYPE_F16 one among them (the
    dtype-generic entries take float pointers; halves go through cn_dcn_v2_forward_nhwc_f16)."""
    spec = importlib.util.spec_from_file_location("gen_dcn_routes", os.path.join(ROOT, "tests", "golden", "gen_dcn_routes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, "tests", "golden", "dcn_routes.json")) as f:
        recorded = gen.unpack(json.load(f))
    assert {p[5] for p in gen.main_grid()} == {gen.F32, gen.F32S}
    got = gen.answers()
    for g in ("main", "pitch", "query", "bad"):
        assert got[g] == recorded[g], g
    assert [a for d, a in zip(gen.bad_grid(), got["bad"]) if d["dtype"] == gen.F16] == [[-2]]


def test_fp16_option_parses_and_excludes_fp32_mfma():
    from centernet_amd.opts import opts
    opt = opts().init("ctdet --arch resdcn_18 --fp16".split())
    assert opt.fp16 and not opt.fp32_mfma and opt.arch == "resdcn_18"
    assert not opts().init("ctdet --arch resdcn_18".split()).fp16
    with pytest.raises(SystemExit):
        opts().init("ctdet --arch resdcn_18 --fp16 --fp32_mfma".split())


def test_header_and_bindings_name_the_half_form():
    import re
    from centernet_amd import native
    with open(os.path.join(ROOT, "include", "centernet_amd.h")) as f:
        src = f.read()
    assert int(re.search(r"^#define\s+CN_DCNH_WINDOW\s+(\d+)", src, re.M).group(1)) == native.DCNH_WINDOW == 7
    assert native.dcn_form_name(native.DCNH_WINDOW) == "window_f16" and native.dcn_form_name(0) == "gather"
    assert hasattr(native.lib(), "cn_maxpool_nhwc_f16")
