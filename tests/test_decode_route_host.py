"""The host-only decode queries answer as they did before they moved onto topk_route (csrc/cn_decode.hip):
tests/golden/decode_queries.json holds the answers of the library of the commit before that, over the grid of
tests/golden/gen_decode_queries.py.  And the flag constants of native.py are the header's.  No GPU."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
QUERIES = ("ctdet", "ddd", "exct", "agnex_ct", "multi_pose_j1", "multi_pose_j17")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_decode_queries", os.path.join(GOLDEN, "gen_decode_queries.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "decode_queries.json")) as f:
        return json.load(f)


def test_grid_reaches_every_answer(gen, recorded):
    """The recorded grid is the generator's, it holds every model shape of bench.py, and it is not one-sided:
    shapes with and without a state region (the one-launch form taken or not), refusals, and more than one
    size per query."""
    grid = list(gen.points())
    assert recorded["n"] == len(grid) == len(set(grid)) > 2000
    assert all(s[:5] in grid for s in gen.MODEL_SHAPES)
    assert set(recorded) == set(QUERIES) | {"n", "state_rc", "state_offset", "state_bytes", "refused"}
    for q in QUERIES:
        assert len(recorded[q]) == recorded["n"], q
        assert 0 in recorded[q] and len(set(recorded[q]) - {0}) > 1, q
    rc, off, nb = recorded["state_rc"], recorded["state_offset"], recorded["state_bytes"]
    assert len(rc) == len(off) == len(nb) == recorded["n"]
    assert 0 in rc and set(rc) - {0}                                      # plans and refusals
    assert any(r == 0 and n == 0 for r, n in zip(rc, nb))                 # a plan without the one-launch form
    assert any(r == 0 and n > 0 and o > 0 for r, o, n in zip(rc, off, nb))
    assert all(n == 0 and o == 0 for r, o, n in zip(rc, off, nb) if r)
    # the conditions of the route that the state region shows, on both sides, among the shapes with a plan
    has = {p: n > 0 for p, r, n in zip(grid, rc, nb) if r == 0}
    assert has[(1, 80, 128, 128, 100)] and not has[(1, 80, 129, 128, 100)] and not has[(1, 80, 128, 132, 100)]
    assert has[(1, 1024, 16, 16, 4)] and not has[(1, 1025, 16, 16, 4)]     # OP_CMAX
    assert has[(1, 3, 64, 64, 5)] and not has[(1, 3, 64, 64, 40)]           # C * groups against 4 K
    assert not has[(1, 80, 10, 18, 4)] and not has[(1, 1, 128, 128, 100)]   # W & 3; the pose centre map


def test_queries_answer_as_recorded(gen, recorded):
    assert all(recorded["refused"])      # (nothing the generator calls with made-up pointers was ever accepted)
    got = gen.answers()
    assert got["n"] == recorded["n"]
    grid = list(gen.points())
    calls = gen.refused_calls()
    for q in sorted(set(recorded) - {"n"}):
        g, w = got[q], recorded[q]
        if g != w:
            bad = [i for i in range(len(w)) if g[i] != w[i]]
            what = calls[bad[0]] if q == "refused" else grid[bad[0]]
            pytest.fail("%s: %d answers differ, first at %r: %r, recorded %r" % (q, len(bad), what, g[bad[0]], w[bad[0]]))


def test_refused_calls_are_recorded_as_refused(gen, recorded):
    """Every call of the generator's refused_calls() was refused, for more than one reason over the list (they
    carry pointers that must never be followed), and there is one recorded code per call."""
    assert len(recorded["refused"]) == len(gen.refused_calls()) > 300
    assert all(recorded["refused"]) and len(set(recorded["refused"])) >= 5


def test_flag_constants_are_the_headers():
    """Every DECODE_* / EXCT_* constant of native.py equals the #define CN_<name> of include/centernet_amd.h."""
    from centernet_amd import native
    with open(os.path.join(ROOT, "include", "centernet_amd.h")) as f:
        defines = dict(re.findall(r"^#define\s+CN_((?:DECODE|EXCT)_\w+)\s+(\d+)\s*$", f.read(), re.M))
    names = [n for n in dir(native) if n.startswith(("DECODE_", "EXCT_"))]
    assert len(names) >= 7 and set(names) == set(defines), (sorted(names), sorted(defines))
    for n in names:
        assert getattr(native, n) == int(defines[n]), n
