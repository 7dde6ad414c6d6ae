"""The deferred heads of the multi_pose task on the host: which heads the detector leaves to the decode, and the
argument checks of the two C entries (cn_multi_pose_heads_at_cells_f32, cn_multi_pose_match_f32) that need no
device."""
import contextlib
import ctypes
import sys

import pytest


def _opt(extra=()):
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        return opts().init(["multi_pose"] + list(extra))


@pytest.mark.parametrize("extra, want", [
    ([], ("wh", "hps", "reg")),
    (["--not_reg_offset"], ("wh", "hps")),
    (["--flip_test"], ()),
    (["--K", "130"], ()),
    (["--not_hm_hp"], ("wh", "hps", "reg")),     # the centre heads are still deferred; hm stays dense
], ids=["default", "not_reg_offset", "flip_test", "K130", "not_hm_hp"])
def test_deferred_pose_heads(extra, want):
    from centernet_amd.detectors.multi_pose import deferred_pose_heads
    opt = _opt(extra)
    assert deferred_pose_heads(opt) == want
    assert "hm" in opt.heads and "hm" not in want


def test_deferred_pose_heads_needs_the_heads():
    from centernet_amd.detectors.multi_pose import deferred_pose_heads
    opt = _opt()
    opt.heads = {k: v for k, v in opt.heads.items() if k != "hps"}
    assert deferred_pose_heads(opt) == ()
    opt = _opt()
    opt.heads = {k: v for k, v in opt.heads.items() if k != "wh"}
    assert deferred_pose_heads(opt) == ()


def _buf():
    # 16-byte alignment is not guaranteed by ctypes, so take an aligned address inside a larger buffer
    raw = (ctypes.c_float * 128)()
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, ctypes.c_void_p(addr)


def test_pose_heads_at_cells_refuses_bad_arguments():
    from centernet_amd import native
    lib = native.lib()
    _keep, p = _buf()

    def call(feat=p, B=1, H=4, W=4, Cin=64, pitch=64, dtype=native.DTYPE_F32S, hidden=64, n_heads=3, J=17, K=4,
             dets=p):
        return lib.cn_multi_pose_heads_at_cells_f32(feat, B, H, W, Cin, pitch, dtype, 1.0, p, p, p, K, p, p, hidden,
                                                    n_heads, J, p, None, dets, None, None)
    assert call(feat=None) == -5 and call(dets=None) == -5
    assert call(K=0) == -1 and call(pitch=32) == -1
    assert call(dtype=native.DTYPE_F16) == -2
    assert call(hidden=96) == -2 and call(hidden=320) == -2
    assert call(n_heads=1) == -2 and call(n_heads=4) == -2
    assert call(J=0) == -2 and call(J=18) == -2
    assert call(Cin=48, pitch=48) == -2


def test_pose_match_refuses_bad_arguments():
    from centernet_amd import native
    lib = native.lib()
    _keep, p = _buf()
    B, J, H, W, K = 1, 17, 16, 16, 8
    need = lib.cn_multi_pose_decode_workspace_bytes(B, 1, H, W, J, K)
    assert need > 16

    def call(hm_hp=p, K=K, dets=p, ws=p, nbytes=need):
        return lib.cn_multi_pose_match_f32(hm_hp, None, B, J, H, W, K, 1, dets, ws, nbytes, None)
    assert call(hm_hp=None) == -5 and call(dets=None) == -5
    assert call(K=129) == -2
    assert call(nbytes=16) == -3


def test_pack_cell_heads_w1_takes_three_wide_heads():
    """N = 768 (three 256-wide heads) is a size the packer takes: with a null `w` nothing is launched and the
    return is the null code, not "unsupported"; the other refusals keep their codes."""
    from centernet_amd import native
    lib = native.lib()
    _keep, p = _buf()
    assert lib.cn_pack_cell_heads_w1(None, p, 768, 64, None) == -5
    assert lib.cn_pack_cell_heads_w1(p, p, 1024, 64, None) == -2
    assert lib.cn_pack_cell_heads_w1(p, p, 96, 64, None) == -2
    assert lib.cn_pack_cell_heads_w1(p, p, 768, 48, None) == -2
