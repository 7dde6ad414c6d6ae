"""The streaming exct / agnex grouping, host side: the blocked reference of tests/exct_stream_ref.py against the
oracle and the reference's goldens at K > 64, the workspace bound of the streaming entries (no K^4 array), the
exported symbols and the --ex_stream flag.  No GPU."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

import exct_stream_ref as SR
from oracle import cref
from test_oracle_agnex import GEN as AGEN
from test_oracle_exct import GEN, assert_same

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_bigk():
    spec = importlib.util.spec_from_file_location("gen_golden_exct_bigk",
                                                  os.path.join(HERE, "golden", "gen_golden_exct_bigk.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BIGK = _load_bigk()
BIGK_GOLD = np.load(os.path.join(HERE, "golden", "exct_bigk_golden.npz"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(GEN.EXCT_CASES))
def test_helper_is_the_oracle_exct(name):
    heats, regs, K, num_dets = GEN.exct_inputs(name)
    assert np.array_equal(_bits(SR.exct_decode(*heats, *regs, K=K, num_dets=num_dets)),
                          _bits(cref.exct_decode(*heats, *regs, K=K, num_dets=num_dets)))


@pytest.mark.parametrize("name", sorted(GEN.AGGR_CASES))
def test_helper_is_the_oracle_with_edge_aggregation(name):
    base, w = GEN.AGGR_CASES[name]
    heats, regs, K, num_dets = GEN.exct_inputs(base)
    assert np.array_equal(_bits(SR.exct_decode(*heats, *regs, K=K, num_dets=num_dets, aggr_weight=w)),
                          _bits(cref.exct_decode(*heats, *regs, K=K, num_dets=num_dets, aggr_weight=w)))


@pytest.mark.parametrize("name", sorted(AGEN.AGNEX_CASES))
def test_helper_is_the_oracle_agnex(name):
    heats, regs, K, num_dets = AGEN.agnex_inputs(name)
    assert np.array_equal(_bits(SR.agnex_ct_decode(*heats, *regs, K=K, num_dets=num_dets)),
                          _bits(cref.agnex_ct_decode(*heats, *regs, K=K, num_dets=num_dets)))
    if name == "agnex_small":       # the aggregation in front of the class-agnostic form, and no offset maps
        assert np.array_equal(_bits(SR.agnex_ct_decode(*heats, K=K, num_dets=num_dets, aggr_weight=0.1)),
                              _bits(cref.agnex_ct_decode(*heats, K=K, num_dets=num_dets, aggr_weight=0.1)))


@pytest.mark.parametrize("name", ["exct_k72", "exct_k100"])
def test_helper_matches_the_reference_beyond_k64(name):
    heats, regs, K, num_dets = BIGK.exct_inputs(name)
    gold = BIGK_GOLD[name + "/dets"]
    assert_same(SR.exct_decode(*heats, *regs, K=K, num_dets=num_dets), gold)
    if name == "exct_k72":          # the cut lies in the penalty tail: positive and penalised rows
        assert 0 < int((gold[..., 4] > 0).sum()) < num_dets


def test_golden_file_holds_only_the_rows():
    want = {n + "/dets" for n in list(BIGK.EXCT_BIGK_CASES) + list(BIGK.AGNEX_BIGK_CASES)}
    assert set(BIGK_GOLD.files) == want
    for n in want:
        assert BIGK_GOLD[n].shape == (1, 1000, 14) and BIGK_GOLD[n].dtype == np.float32


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("shape", [(2, 80, 128, 128, 128), (32, 80, 128, 128, 100)])
def test_streaming_workspace_has_no_k4_array(shape):
    """Beyond the top-K workspace: the twelve lists, the one clamped map, at most 1 MiB of select state per image."""
    from centernet_amd import native
    lib = native.lib()
    B, C, H, W, K = shape
    lists = 12 * _align(B * K * 4)
    for query, base_c, extra in (
            (lib.cn_exct_decode_stream_workspace_bytes, C, 0),
            (lib.cn_agnex_ct_decode_stream_workspace_bytes, 1, 2 * _align(B * H * W * 4))):   # + max / arg-max planes
        base = lib.cn_ctdet_decode_workspace_bytes(B, base_c, H, W, K)
        got = query(B, C, H, W, K)
        assert base > 0 and got > 0
        state = got - base - lists - _align(B * base_c * H * W * 4) - extra
        assert 0 < state <= B * (1 << 20), (shape, state)
        assert got < B * K ** 4 * 4                        # (what the candidates alone would take)


def test_symbols_and_stored_queries():
    from centernet_amd import native
    lib = native.lib()
    raw = ctypes.CDLL(lib._name)
    for name in ("cn_exct_decode_stream_workspace_bytes", "cn_exct_decode_stream_f32",
                 "cn_agnex_ct_decode_stream_workspace_bytes", "cn_agnex_ct_decode_stream_f32"):
        assert hasattr(raw, name), name
    assert lib.cn_exct_decode_stream_f32.argtypes == lib.cn_exct_decode_f32.argtypes
    assert lib.cn_version() == 313
    # the stored forms' queries answer as recorded, K^4 floats included (tests/test_decode_route_host.py holds the
    # whole grid; one point here, the reference's operating point)
    spec = importlib.util.spec_from_file_location("gen_decode_queries", os.path.join(HERE, "golden", "gen_decode_queries.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(HERE, "golden", "decode_queries.json")) as f:
        recorded = json.load(f)
    point = (1, 80, 128, 128, 100)
    at = list(gen.points()).index(point)
    assert lib.cn_exct_decode_workspace_bytes(*point) == recorded["exct"][at] > 4 * 100 ** 4
    assert lib.cn_agnex_ct_decode_workspace_bytes(*point) == recorded["agnex_ct"][at] > 4 * 100 ** 4
    assert lib.cn_exct_decode_stream_workspace_bytes(1, 80, 128, 128, 129) == 0      # past the top-K's own limit


def test_ex_stream_flag():
    from centernet_amd.opts import opts
    assert opts().init(["exdet", "--arch", "hourglass", "--ex_stream"]).K == 100
    assert opts().init(["exdet", "--arch", "hourglass", "--ex_stream", "--K", "72"]).K == 72
    o = opts().init(["exdet", "--arch", "hourglass"])
    assert o.K == 40 and o.ex_stream is False
    for task in ("ctdet", "multi_pose", "ddd"):
        plain, flagged = opts().init([task]), opts().init([task, "--ex_stream"])
        assert plain.ex_stream is False and flagged.ex_stream is True
        a, b = dict(vars(plain)), dict(vars(flagged))
        a.pop("ex_stream"), b.pop("ex_stream")
        assert a == b and flagged.K == 100
