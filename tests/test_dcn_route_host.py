"""dcn_route (csrc/cn_dcn.hip) decides what the deformable entry decided before the decision had one home:
tests/golden/dcn_routes.json holds, over the grid of tests/golden/gen_dcn_routes.py, what the library of the commit
before did with every call -- recorded from a dry-run build of that commit, see the generator -- and the host query
cn_dcn_v2_route of the tree's library must say the same.  No GPU."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("B", "Cin", "Cout", "H", "W", "dtype", "flags", "out_pitch", "om_pitch", "om_offset", "y_offset", "workspace")
D = "{}"     # the default keys


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_dcn_routes", os.path.join(GOLDEN, "gen_dcn_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(gen):
    with open(os.path.join(GOLDEN, "dcn_routes.json")) as f:
        return gen.unpack(json.load(f))


def _k(**keys):
    return json.dumps({str(k)[1:]: v for k, v in keys.items()}, sort_keys=True)


def test_grid_reaches_every_answer(gen, recorded):
    """The recorded grid is the generator's and holds what the route can say: every form, every split, every
    fall-through edge of the order of preference, every refusal code, and a changed answer for every key."""
    main, pitch = list(gen.main_grid()), list(gen.pitch_grid())
    assert set(recorded["main"]) == {json.dumps(k, sort_keys=True) for k in gen.KEYS}
    assert set(recorded["pitch"]) == {json.dumps(k, sort_keys=True) for k in gen.KEYS_PITCH}
    assert all(len(v) == len(main) > 2000 for v in recorded["main"].values())
    assert all(len(v) == len(pitch) > 8000 for v in recorded["pitch"].values())
    # the shapes, dtypes, pitches, alignments and workspaces of the grid
    shapes = set(gen.SHAPES)
    assert {s[0] for s in shapes} == {1, 8, 32}
    for layer in ((512, 256, 16, 16), (256, 128, 32, 32), (128, 64, 64, 64), (256, 256, 32, 32), (128, 128, 64, 64),
                  (64, 64, 128, 128)):
        assert all((B,) + layer in shapes for B in (1, 8, 32)), layer
    assert any(s[3] % 8 for s in shapes) and any(s[4] % 16 for s in shapes) and any(s[1] % 32 for s in shapes)
    assert {24, 32, 36, 64, 66, 128, 192, 256} <= {s[2] for s in shapes}
    assert {(p[5], p[6]) for p in main} == {(gen.F32, 0), (gen.F32, 2), (gen.F32S, 0), (gen.F32S, 2)}
    assert {p[11] for p in main} == {"none", "query", "short2", "short4", "short8", "short3", "short9", "ample", "misaligned"}
    assert {p[8] for p in pitch} == {27, 32, 40} and {p[9] for p in pitch} == {0, 4} and {p[10] for p in pitch} == {0, 4}
    pitches = {(gen._pitch(p[7], p[2], p[5], p[6]) - p[2], gen._pitch(p[7], p[2], p[5], p[6]) % 4) for p in pitch}
    assert any(d == 0 for d, _ in pitches) and any(d >= 32 for d, _ in pitches) and any(m for _, m in pitches)
    # the answers
    base = recorded["main"][D]
    ok = [a for a in base if a[0] == 0]
    everything = [a for v in recorded["main"].values() for a in v if a[0] == 0]
    assert {a[1] for a in everything} == set(range(7)), "every form"
    assert {a[4] for a in ok} == {1, 2, 3, 4, 8, 9}, "every split, at the default keys"
    assert {a[0] for a in recorded["bad"]} == {0, -1, -2, -5, -6}, "every refusal code of the entry's checks"
    assert len(recorded["bad"]) == len(list(gen.bad_grid()))
    for k, v in recorded["main"].items():
        # (key 36 = 2 against its default 3 shows only with the wide form off: the pair below)
        assert k in (D, _k(k36=2)) or v != base, "key %s changes no answer" % k
    assert recorded["main"][_k(k36=2, k41=0)] != recorded["main"][_k(k41=0)]
    for k, v in recorded["pitch"].items():
        assert k == D or v != recorded["pitch"][D], k
    # a key 37 / 42 far above and far below the workgroup counts: deeper and shallower splits than the default's
    for key in (37, 42):
        hi, lo = recorded["main"][json.dumps({str(key): 4096})], recorded["main"][json.dumps({str(key): 1})]
        assert any(h[4] > b[4] for h, b in zip(hi, base) if h[0] == 0 == b[0])
        assert any(l[4] < b[4] for l, b in zip(lo, base) if l[0] == 0 == b[0])
    # the edges, read off pairs of key settings on the same call (f32s calls only: fp32 is always the gather form)
    s = [i for i, p in enumerate(main) if p[5] == gen.F32S and base[i][0] == 0]
    form = {k: [a[1] if a[0] == 0 else None for a in v] for k, v in recorded["main"].items()}
    gather = (gen.GATHER, gen.GATHER_PAD)
    team, wide = (gen.TEAM_T, gen.TEAM_N), (gen.WIDE4, gen.WIDE8)
    for forced in (4, 5, 6, 7):         # a forced form that does not take the call: the gather form, not the next one
        assert any(form[_k(k23=forced)][i] in gather and form[D][i] not in gather for i in s), forced
    # (the register-sampling form takes every shape the team form takes: what it refuses is an offset tensor that
    # is not 8-byte aligned or of odd pitch, which is in the pitch grid)
    assert any(f[0] == 0 and f[1] in gather and d[1] in team and (p[8] % 2 or p[9])
               for p, f, d in zip(pitch, recorded["pitch"][_k(k23=2)], recorded["pitch"][D]) if p[5] == gen.F32S)
    # wide -> team: a call the wide form does not serve (forced, it goes to the gather form) runs the team form
    assert any(form[D][i] in team and form[_k(k23=6)][i] in gather for i in s)
    # ... and with the wide form off (key 41) its calls are the team form's
    assert any(form[D][i] in wide and form[_k(k41=0)][i] in team for i in s)
    # team -> window: the team form refuses the call (forced: gather) on a grid that fills the chip
    assert any(form[D][i] == gen.WINDOW and form[_k(k23=4)][i] in gather and
               main[i][0] * (main[i][3] // 8) * (main[i][4] // 16) >= 64 for i in s)
    # window -> gather by the 192 / 256 workgroup rule: the forced window form (minimum grid 1) takes the call
    assert any(form[D][i] in gather and form[_k(k23=2)][i] == gen.WINDOW for i in s)


def _describe(point):
    return dict(zip(FIELDS, point))


def test_routes_are_the_recorded_ones(gen, recorded):
    from centernet_amd import native
    native.lib().cn_reset_tuning()
    got = gen.answers()
    grids = {"main": list(gen.main_grid()), "pitch": list(gen.pitch_grid())}
    for g, grid in grids.items():
        assert set(got[g]) == set(recorded[g])
        for k, want in recorded[g].items():
            if got[g][k] != want:
                bad = [i for i in range(len(want)) if got[g][k][i] != want[i]]
                pytest.fail("%s grid, keys %s: %d of %d routes differ, first at %d: [rc, form, grid_x, grid_y, ksplit, flags] "
                            "%r, recorded %r, for %r" % (g, k, len(bad), len(want), bad[0], got[g][k][bad[0]], want[bad[0]],
                                                         _describe(grid[bad[0]])))
    bad = [(d, g, w) for d, g, w in zip(gen.bad_grid(), got["bad"], recorded["bad"]) if g != w]
    assert not bad, "refused calls: %r" % (bad[0],)
    for k, want in recorded["query"].items():
        bad = [(s, g, w) for s, g, w in zip(gen.SHAPES, got["query"][k], want) if g != w]
        assert not bad, "workspace query, keys %s: %d differ, first (B, Cin, Cout, H, W) %r: %d slabs, recorded %d" % (
            (k, len(bad)) + bad[0])


def test_the_workspace_query_never_cuts_a_split_short(gen, recorded):
    """The relation the code relies on (see cn_dcn_v2_forward_nhwc_workspace_bytes): at the default keys a call
    given the bytes the query answers gets the split it would get with all the workspace it could use."""
    main = list(gen.main_grid())
    base = recorded["main"][D]
    at = {p: a for p, a in zip(main, base)}
    n = 0
    for p in main:
        if p[11] == "query":
            ample = at[p[:11] + ("ample",)]
            assert at[p] == ample, "%r: %r with the query's bytes, %r with nine slabs" % (_describe(p), at[p], ample)
            n += ample[0] == 0 and ample[4] > 1
    assert n > 50     # ... and that is said of calls that split


def test_form_constants_are_the_headers():
    """Every DCN_* constant of native.py equals the #define CN_<name> of include/centernet_amd.h."""
    from centernet_amd import native
    with open(os.path.join(ROOT, "include", "centernet_amd.h")) as f:
        defines = dict(re.findall(r"^#define\s+CN_(DCN_\w+)\s+(\d+)\s", f.read(), re.M))
    names = [n for n in dir(native) if n.startswith("DCN_") and isinstance(getattr(native, n), int)]
    assert len(names) == 11 and set(names) == set(defines), (sorted(names), sorted(defines))
    for n in names:
        assert getattr(native, n) == int(defines[n]), n
    assert len(native.DCN_FORM_NAMES) == 7
    assert ctypes_fields(native.DcnRouteInfo) == header_fields("cn_dcn_route_info")


def ctypes_fields(struct):
    return [n for n, _ in struct._fields_]


def header_fields(name):
    with open(os.path.join(ROOT, "include", "centernet_amd.h")) as f:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n.strip() for decl in body.split(";") for n in decl.replace("int ", "").split(",") if n.strip()]
