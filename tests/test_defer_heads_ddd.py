"""The deferred heads of the ddd task on the host: which heads the detector leaves to the decode, and the argument
checks of the C entry (cn_ddd_heads_at_cells_f32) that need no device."""
import contextlib
import ctypes
import sys

import pytest


def _opt(extra=()):
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        return opts().init(["ddd"] + list(extra))


@pytest.mark.parametrize("extra, want", [
    ([], ("dep", "rot", "dim", "wh", "reg")),
    (["--not_reg_offset"], ("dep", "rot", "dim", "wh")),
    (["--not_reg_bbox"], ("dep", "rot", "dim", "reg")),
    (["--not_reg_offset", "--not_reg_bbox"], ("dep", "rot", "dim")),
    (["--K", "130"], ()),
], ids=["default", "not_reg_offset", "not_reg_bbox", "neither", "K130"])
def test_deferred_ddd_heads(extra, want):
    from centernet_amd.detectors.ddd import deferred_ddd_heads
    opt = _opt(extra)
    assert deferred_ddd_heads(opt) == want
    assert "hm" in opt.heads and "hm" not in want


@pytest.mark.parametrize("gone", ["dep", "rot", "dim", "wh", "reg"])
def test_deferred_ddd_heads_needs_the_heads(gone):
    from centernet_amd.detectors.ddd import deferred_ddd_heads
    opt = _opt()
    opt.heads = {k: v for k, v in opt.heads.items() if k != gone}
    assert deferred_ddd_heads(opt) == ()


def test_cell_head_group_sizes():
    from centernet_amd.engine import cell_head_group_sizes
    assert cell_head_group_sizes(5, 256, wide=False) == (1, 1, 1, 1, 1)
    assert cell_head_group_sizes(3, 64, wide=False) == (1, 1, 1)
    assert cell_head_group_sizes(5, 256, wide=True) == (3, 2)       # (dep, rot, dim) + (wh, reg)
    assert cell_head_group_sizes(5, 64, wide=True) == (3, 2)        # a group takes three heads at the most
    assert cell_head_group_sizes(4, 192, wide=True) == (3, 1)


def _buf():
    # 16-byte alignment is not guaranteed by ctypes, so take an aligned address inside a larger buffer
    raw = (ctypes.c_float * 128)()
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, addr


def test_ddd_heads_at_cells_refuses_bad_arguments():
    from centernet_amd import native
    lib = native.lib()
    _keep, addr = _buf()
    p = ctypes.c_void_p(addr)
    RAW = native.DECODE_DDD_RAW_DEPTH

    def table(sizes, w1=addr, b1=addr, w2=addr):
        tab = (native.CellHeadGroup * max(len(sizes), 1))()
        for t, n in zip(tab, sizes):
            t.w1_packed, t.bias1, t.w2, t.bias2, t.n_heads = w1, b1, w2, None, n
        return tab

    def call(feat=p, B=1, H=4, W=4, Cin=64, pitch=64, dtype=native.DTYPE_F32S, hidden=64, sizes=(1, 1, 1, 1, 1),
             groups=True, has_wh=1, has_reg=1, K=4, dets=p, scores=p, n_groups=None, **kw):
        tab = table(sizes, **kw) if groups else None
        return lib.cn_ddd_heads_at_cells_f32(feat, B, H, W, Cin, pitch, dtype, 1.0, scores, p, p, K, hidden,
                                             len(sizes) if n_groups is None else n_groups, tab, has_wh, has_reg,
                                             RAW, dets, None, None)
    # null
    assert call(feat=None) == -5 and call(dets=None) == -5 and call(scores=None) == -5
    assert call(groups=False) == -5
    assert call(w1=None) == -5 and call(b1=None) == -5 and call(w2=None) == -5
    # shape
    assert call(K=0) == -1 and call(B=0) == -1 and call(pitch=32) == -1 and call(n_groups=0) == -1
    # f16
    assert call(dtype=native.DTYPE_F16) == -2
    # hidden outside {64, 128, 192, 256}
    assert call(hidden=96) == -2 and call(hidden=320) == -2 and call(hidden=0) == -2
    # a group with more than three heads (N > 768 would take a fourth 256-wide one) or with none; six groups
    assert call(sizes=(5,)) == -2 and call(sizes=(4, 1)) == -2
    assert call(sizes=(1, 0, 1, 1, 1, 1), n_groups=5) == -2
    assert call(sizes=(1, 1, 1, 1, 1, 1), has_wh=1, has_reg=1) == -2
    # the groups' heads do not sum to 3 + has_wh + has_reg
    assert call(sizes=(1, 1, 1, 1)) == -2 and call(sizes=(3, 3)) == -2
    assert call(sizes=(1, 1, 1, 1, 1), has_reg=0) == -2 and call(sizes=(3,), has_wh=1, has_reg=0) == -2
    # Cin % 32, pitch rules
    assert call(Cin=48, pitch=48) == -2
    assert call(pitch=68, dtype=native.DTYPE_F32S) == -2 and call(pitch=66, dtype=native.DTYPE_F32) == -2
    # alignment is looked at last
    assert call(feat=ctypes.c_void_p(addr + 4)) == -6 and call(w1=addr + 4) == -6
    assert call(feat=ctypes.c_void_p(addr + 4), hidden=96) == -2
