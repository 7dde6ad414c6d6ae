"""The deferred-heads mode of PlannedModule on the host: what it stores, what it survives, and the C entry's
argument checks that need no device."""
import ctypes

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
