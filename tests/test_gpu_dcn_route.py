"""What cn_dcn_v2_route says of a call is what cn_dcn_v2_forward_nhwc runs: every form of dcn_route
(csrc/cn_dcn.hip) once unsplit and once split, both tap splits of the gather form, forced forms that fall through
to it, and the small grid that the default keys leave to it.  Per case: ask the query, run the call with a
sentinel-filled workspace of nine slabs, count the slabs it wrote (every form writes its partial sums as whole
[B * H * W][cout_pad] slabs, one per K slice, the gather form included: its tiles store every row m < B * H * W and
every column n < cout_pad), and hold the output to the bar of tests/test_gpu_dcn.py against the C oracle.

One image, maps of 1 / 4 / 8 window tiles: the forms are forced with key 23 (at such grids the default keys choose
the gather form), the splits steered with keys 13 / 37 / 42 and the depth of K.  Cout = 256 gives the window, T-mode
team, four-block wide and gather forms two blocks of output channels."""
import functools
import os
import sys

import pytest

from centernet_amd import native
from oracle import cref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dcn_cases import _Layer, _case, _check, _is_sentinel, _nchw, _sentinel   # noqa: E402

pytestmark = pytest.mark.gpu
PREFETCH, STAGGER, TILE2D, VEC_OUT = (native.DCN_FLAG_PREFETCH, native.DCN_FLAG_STAGGER, native.DCN_FLAG_TILE2D,
                                      native.DCN_FLAG_VEC_OUT)

# id, cn_set_tuning keys, (Cin, H, W, Cout), the form, K split and flags the route must say.  A window form splits
# K only down to two 32-channel chunks per slice: Cin = 64 never splits, Cin = 128 splits in two, Cin = 256 in four
CASES = [
    ("window", {23: 2}, (64, 16, 32, 64), native.DCN_WINDOW, 1, 0),
    ("window-split", {23: 2}, (128, 16, 32, 256), native.DCN_WINDOW, 2, 0),
    ("team_t", {23: 4, 37: 1}, (128, 16, 32, 64), native.DCN_TEAM_T, 1, STAGGER),
    ("team_t-split", {23: 4}, (128, 16, 32, 128), native.DCN_TEAM_T, 2, STAGGER),
    ("team_n", {23: 5, 37: 1}, (64, 8, 16, 128), native.DCN_TEAM_N, 1, STAGGER),
    ("team_n-split", {23: 5}, (128, 16, 32, 128), native.DCN_TEAM_N, 2, STAGGER),
    ("wide4", {23: 7, 42: 1}, (64, 16, 32, 256), native.DCN_WIDE4, 1, 0),
    ("wide4-split", {23: 7}, (256, 8, 16, 128), native.DCN_WIDE4, 4, PREFETCH),
    ("wide8", {23: 6, 42: 1}, (64, 16, 32, 256), native.DCN_WIDE8, 1, 0),
    ("wide8-split", {23: 6}, (128, 32, 32, 256), native.DCN_WIDE8, 2, 0),
    ("gather", {23: 1, 13: 1}, (64, 16, 32, 64), native.DCN_GATHER, 1, TILE2D | VEC_OUT),
    ("gather-split3", {23: 1, 13: 3}, (64, 16, 32, 256), native.DCN_GATHER, 3, TILE2D | VEC_OUT),
    ("gather-split9", {23: 1}, (128, 16, 32, 64), native.DCN_GATHER, 9, TILE2D | VEC_OUT),
    ("gather_pad", {13: 1}, (48, 16, 32, 64), native.DCN_GATHER_PAD, 1, TILE2D | VEC_OUT),
    ("gather_pad-split", {}, (48, 16, 32, 64), native.DCN_GATHER_PAD, 9, TILE2D | VEC_OUT),
    # a forced form that does not take the shape: straight to the gather form
    ("wide-forced-on-64-channels", {23: 6}, (64, 16, 32, 64), native.DCN_GATHER, 9, TILE2D | VEC_OUT),
    ("team-forced-on-12-rows", {23: 4}, (64, 12, 32, 64), native.DCN_GATHER, 9, VEC_OUT),
    # the default keys on four tiles: below the window form's 192 workgroups
    ("default-keys-small-grid", {}, (64, 16, 32, 64), native.DCN_GATHER, 9, TILE2D | VEC_OUT),
]


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    native.lib().cn_reset_tuning()


@functools.lru_cache(maxsize=None)
def _layer(dev, shape):
    """the layer of a shape and its oracle output: computed once, shared by the cases of the shape"""
    Cin, H, W, Cout = shape
    x, off, mask, w, b = _case(1, Cin, H, W, Cout, 5200 + Cin + H + W + Cout, off_std=1.5)
    return _Layer(dev, x, off, mask, w, b), cref.dcn_v2_forward(x, off, mask, w, b)


@pytest.mark.parametrize("name,keys,shape,form,ksplit,flags", CASES, ids=[c[0] for c in CASES])
def test_the_route_said_is_the_route_run(dev, name, keys, shape, form, ksplit, flags):
    L, want = _layer(dev, shape)
    guard = 1024
    with native.tuning(keys):
        for out_plain, msig in ((False, True), (True, False)):
            ws = _sentinel((9 * L.slab + guard,), dev)
            info = L.route(out_plain, msig=msig, ws=ws, ws_bytes=9 * L.slab * 4)
            said = (info.form, info.ksplit, info.flags)
            assert said == (form, ksplit, flags), (name, said)
            rc, t, act = L.run(out_plain, msig=msig, ws=ws, ws_bytes=9 * L.slab * 4)
            assert rc == 0
            assert L.slabs_written(ws[:9 * L.slab]) == (info.ksplit if info.ksplit > 1 else 0), name
            assert bool(_is_sentinel(ws[9 * L.slab:]).all())
            assert not bool(_is_sentinel(t).any())
            _check(_nchw(act), want, "%s plain %d msig %d:" % (name, out_plain, msig))
