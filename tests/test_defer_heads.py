"""The deferred-heads mode of PlannedModule on the host: what it stores, what it survives, and the C entry's
argument checks that need no device."""
import contextlib
import ctypes
import sys

import pytest
import torch

from centernet_amd.model import create_model


def test_defer_mode_survives_plan_drops_and_follows_the_compute_mode():
    m = create_model("resdcn_18", {"hm": 80, "wh": 2, "reg": 2}, 64).eval()
    assert m.deferred_names() == ()
    assert m.defer_heads(("wh", "reg")) is m
    m.drop_plans()
    assert m.deferred_names() == ("wh", "reg")
    m.invalidate_plans()
    assert m.deferred_names() == ("wh", "reg")
    m.fp32_mfma()
    assert m.deferred_names() == ("wh", "reg")          # both fp32 compute modes
    m.half_compute()
    assert m.deferred_names() == ()
    m.half_compute(False)
    assert m.deferred_names() == ("wh", "reg")
    m.defer_heads(())
    assert m.deferred_names() == ()


def test_heads_at_cells_refuses_bad_arguments():
    from centernet_amd import native
    lib = native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)          # 16-byte alignment is not guaranteed: checked last by the entry

    def call(feat=p, B=1, H=4, W=4, Cin=64, pitch=64, dtype=native.DTYPE_F32S, hidden=64, n_heads=2, K=4, dets=p):
        return lib.cn_ctdet_heads_at_cells_f32(feat, B, H, W, Cin, pitch, dtype, 1.0, p, p, p, K, p, p, hidden,
                                               n_heads, p, None, dets, None, None)
    assert call(feat=None) == -5 and call(dets=None) == -5
    assert call(K=0) == -1 and call(pitch=32) == -1
    assert call(dtype=native.DTYPE_F16) == -2
    assert call(hidden=96) == -2 and call(hidden=320) == -2 and call(n_heads=3) == -2
    assert call(Cin=48, pitch=48) == -2 and call(dtype=native.DTYPE_F32S, pitch=68) == -2
    assert lib.cn_pack_cell_heads_w1(None, p, 64, 64, None) == -5
    assert lib.cn_pack_cell_heads_w1(p, p, 96, 64, None) == -2
    assert lib.cn_pack_cell_heads_w1(p, p, 1024, 64, None) == -2


def _ctdet_opt(extra=()):
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        return opts().init(["ctdet"] + list(extra))


# what CtdetDetector._deferred_heads returned for these options while the predicate was a method of the class
@pytest.mark.parametrize("extra, reg_head, want", [
    ([], None, ("wh", "reg")),
    (["--flip_test"], None, ()),                  # the averaged maps are needed
    (["--cat_spec_wh"], None, ()),                # 2 x classes outputs
    (["--K", "130"], None, ()),
    (["--not_reg_offset"], None, ("wh",)),        # the options leave the network without a reg head
    (["--not_reg_offset"], 2, ()),                # a reg head the decode does not read: nothing is deferred
], ids=["default", "flip_test", "cat_spec_wh", "K130", "no_reg", "not_reg_offset_with_reg_head"])
def test_deferred_ctdet_heads(extra, reg_head, want):
    from centernet_amd.detectors.ctdet import deferred_ctdet_heads
    opt = _ctdet_opt(extra)
    if reg_head is not None:
        opt.heads = dict(opt.heads, reg=reg_head)
    assert ("reg" in opt.heads) == (extra != ["--not_reg_offset"] or reg_head is not None)
    assert deferred_ctdet_heads(opt) == want
    assert "hm" not in want


class _Packed:
    """Stands for a packed device tensor: DeferredHeads only keeps it and asks for its address."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def test_deferred_heads_groups():
    from centernet_amd.engine import DeferredHeads
    g0 = tuple(_Packed(0x1000 + 16 * i) for i in range(4)) + (3,)
    g1 = tuple(_Packed(0x2000 + 16 * i) for i in range(4)) + (2,)
    one = DeferredHeads(("wh", "hps", "reg"), None, 64, [g0], couts=(2, 34, 2))
    assert one.groups == (g0,) and one.couts == (2, 34, 2) and one.hidden == 64
    assert (one.w1, one.b1, one.w2, one.b2) == g0[:4]          # the only group's tensors themselves
    assert DeferredHeads(("wh", "reg"), None, 64, [g0[:4] + (2,)]).couts == (2, 2)
    # a single group as pack_cell_heads returns it, positionally or with couts: the same one shape
    flat = DeferredHeads(("wh", "hps", "reg"), None, 64, *g0[:4], couts=(2, 34, 2))
    assert flat.groups == one.groups and flat.w1 is g0[0] and flat.couts == one.couts
    assert DeferredHeads(("wh", "reg"), None, 64, groups=[g0[:4] + (2,)]).groups == (g0[:4] + (2,),)
    for bad in ((), g0[:2], g0[:4] + (g0[0],)):
        with pytest.raises(TypeError):
            DeferredHeads(("wh", "reg"), None, 64, *bad)
    with pytest.raises(TypeError):
        DeferredHeads(("wh", "reg"), None, 64, *g0[:4], groups=[g0])
    two = DeferredHeads(("dep", "rot", "dim", "wh", "reg"), None, 256, (g0, g1), couts=(1, 8, 3, 2, 2))
    for field in ("w1", "b1", "w2", "b2"):
        with pytest.raises(RuntimeError, match="single group"):
            getattr(two, field)
        with pytest.raises(AttributeError):                    # read-only
            setattr(one, field, None)
    tab = two.group_table()
    assert len(tab) == 2 and tab is two.group_table()
    for t, g in zip(tab, (g0, g1)):
        assert (t.w1_packed, t.bias1, t.w2, t.bias2, t.n_heads) == tuple(x.addr for x in g[:4]) + (g[4],)
    assert len(one.group_table()) == 1 and one.group_table()[0].n_heads == 3
