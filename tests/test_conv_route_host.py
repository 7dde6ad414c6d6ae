"""The four host-only convolution queries answer as they did before they moved onto conv_route
(csrc/cn_conv.hip): tests/golden/conv_queries.json holds the answers of the library of the commit before
that, over the grid of tests/golden/gen_conv_queries.py.  No GPU."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_conv_queries", os.path.join(GOLDEN, "gen_conv_queries.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "conv_queries.json")) as f:
        return json.load(f)


def test_grid_reaches_every_answer(gen, recorded):
    """The recorded grid is the generator's, and it is not one-sided: every 0 / 1 query says both, and
    some layers want a split-K workspace, at the default keys; each flipped key changes an answer."""
    assert recorded["n"] == len(list(gen.descriptors())) > 3000
    assert set(recorded["knobs"]) == {json.dumps(k, sort_keys=True) for k in gen.KNOBS}
    base = recorded["knobs"]["{}"]
    for q in ("res_pitch", "stem_maxpool", "stem_f32s"):
        assert len(base[q]) == recorded["n"] and {"0", "1"} == set(base[q]), q
    assert len(base["workspace"]) == recorded["n"] and set(base["workspace"]) - {"0"}
    for k, v in recorded["knobs"].items():
        assert k == "{}" or v, k


def test_queries_answer_as_recorded(gen, recorded):
    from centernet_amd import native
    native.lib().cn_reset_tuning()
    got = gen.answers()
    assert got["n"] == recorded["n"]
    grid = list(gen.descriptors())
    for k, want in recorded["knobs"].items():
        assert set(got["knobs"][k]) == set(want), (k, sorted(got["knobs"][k]), sorted(want))
        for q, w in want.items():
            g = got["knobs"][k][q]
            if g != w:
                bad = [i for i in range(len(w)) if g[i] != w[i]]
                d = grid[bad[0]]
                desc = {f: getattr(d, f) for f, _ in d._fields_ if f != "ctl"}
                pytest.fail("%s, keys %s: %d answers differ, first at %d (%s, recorded %s): %r"
                            % (q, k, len(bad), bad[0], g[bad[0]], w[bad[0]], desc))
