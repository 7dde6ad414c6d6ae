"""Case table of the convolution entry cn_conv2d: one descriptor per row, the call around it, and what the host-only
query cn_conv2d_route must say of it.  Shared by tests/test_conv_route_cases_host.py (no GPU: the query with
fabricated aligned addresses) and tests/test_gpu_conv_route.py (the same query with the real pointers, then the
call against a float64 reference).  Not a test module.

A case is a dict (see _c): the tuning keys it runs under, the descriptor fields, dtype and flags, the residual
(none / at the output's pitch / at its own pitch), whether the queried workspace is passed, and the expectation:
status, route, variant, n_tile, m_tile, ksplit.  The expectations were read off conv_route (csrc/cn_conv.hip) and
the launchers of the routed files; the host test holds the library to them, so a predicate, key default or route
order that moves a case onto another kernel fails there, and the GPU test then cannot compare the wrong kernel
unnoticed.

Shapes are the smallest at which the kernel named still has a ragged edge in every tiled dimension: B 1..3, maps at
most 33 wide except where a kernel takes whole 128-pixel rows only (the 16-channel kernels, the stems), or a form
starts at a number of tiles (256-pixel tiles: 1024 of them; the stem + max-pool kernel: 192 strips)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script: the list of cases per route and variant)
    sys.path.insert(0, ROOT)

from centernet_amd import native   # noqa: E402
from centernet_amd.native import (C3_KSKIP, C3_OCC4, C3_PERSIST, C3_TILE, C3_TW32,   # noqa: E402
                                  C3_WAVES8, C3_WREG, CONV_R_PLAIN, CONV_STEM_F32S, CONV_STEM_MAXPOOL, CONV_X_PLAIN,
                                  CONV_Y_PLAIN, DTYPE_F16, DTYPE_F32, DTYPE_F32S, LAYOUT_NCHW, LAYOUT_NHWC, STEM_16S,
                                  STEM_PERSIST, STEM_PERSIST_F32S, STEM_WINDOW)

OK, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2
F32, F16, F32S = "f32", "f16", "f32s"
DTYPES = {F32: DTYPE_F32, F16: DTYPE_F16, F32S: DTYPE_F32S}
XP, YP, RP = CONV_X_PLAIN, CONV_Y_PLAIN, CONV_R_PLAIN


def pf(taps):
    """variant bits of an f32s tile kernel that keeps its weight tile in LDS: `taps` of weight prefetch"""
    return taps << 12


def r32(c):
    return (c + 31) // 32 * 32


def _c(id, route, variant=0, n_tile=0, m_tile=0, ksplit=1, *, shape, k=(3, 3), s=1, pad=None, dil=1, dt=F32,
       flags=0, keys=None, res=None, ws=False, nchw=False, out_pitch=None, c_off=0, res_pitch=None, res_off=0,
       scatter=None, relu=1, rc=OK, stem=False):
    """shape = (B, Cin, H, W, Cout); pad: (pad_h, pad_w), default "same" for the kernel; res: None, "same" (the
    residual's tensor has the output's pitch) or "own" (res_pitch); c_off / res_off: first channel of y / of the
    residual inside their tensors (elements; moves the pointer); scatter = (oy_mul, oy_add, ox_mul, ox_add, OH, OW);
    ws: pass the workspace cn_conv2d_workspace_bytes asks for"""
    B, Cin, H, W, Cout = shape
    if pad is None:
        pad = (dil * (k[0] - 1) // 2, dil * (k[1] - 1) // 2)
    return dict(id=id, route=route, variant=variant, n_tile=n_tile, m_tile=m_tile, ksplit=ksplit, B=B, Cin=Cin, H=H,
                W=W, Cout=Cout, KH=k[0], KW=k[1], s=s, pad_h=pad[0], pad_w=pad[1], dil=dil, dt=dt, flags=flags,
                keys=dict(keys or {}), res=res, ws=ws, nchw=nchw, out_pitch=out_pitch, c_off=c_off,
                res_pitch=res_pitch, res_off=res_off, scatter=scatter, relu=relu, rc=rc, stem=stem)


T = C3_TILE
P28 = {28: 2}          # the persistent kernels at every size
CASES = [
    # ---- LDS-halo tile kernel (no workspace: a layer with KT >= 16 stays unsplit and on this kernel) -------------
    # fp32: Cin = 8 / 40: the last chunk is less than 3/4 full (K-skip); Cout 27 / 33 / 65 / 129: N tiles 32 / 64 /
    # 128 / 64 (129: a 128-wide tile would waste a whole 64-wide one); W = 15, 17: 8 x 16 tiles, W = 33: 4 x 32
    _c("halo_f32_w15_co27_ci8", "halo", T | C3_KSKIP, 32, 128, shape=(2, 8, 5, 15, 27)),
    _c("halo_f32_w17_co33_ci40", "halo", T | C3_KSKIP, 64, 128, shape=(1, 40, 9, 17, 33), res="same"),
    _c("halo_f32_w33_co65_ci128", "halo", T | C3_TW32 | C3_WAVES8, 128, 128, shape=(1, 128, 5, 33, 65)),
    _c("halo_f32_w33_co65_4waves", "halo", T | C3_TW32, 128, 128, shape=(1, 32, 5, 33, 65), keys={15: 0}),
    _c("halo_f32_w17_co129_ci128", "halo", T, 64, 128, shape=(1, 128, 9, 17, 129), res="own", res_pitch=192,
       res_off=32, out_pitch=160, c_off=16),
    _c("halo_f32_w33_co33_occ4", "halo", T | C3_TW32 | C3_OCC4, 64, 128, shape=(1, 32, 9, 33, 33), keys={19: 1}),
    _c("halo_f32_w17_co33_occ4", "halo", T | C3_OCC4, 64, 128, shape=(3, 32, 5, 17, 33), keys={19: 1}, res="same"),
    # key 14: 256-pixel tiles from 1024 of them up (16 x 5 x 3 tiles x 5 blocks of 64 channels), not below
    _c("halo_f32_w33_co64_bm256_small", "halo", T | C3_TW32, 64, 128, shape=(1, 32, 9, 33, 64), keys={14: 1}),
    _c("halo_f32_bm256", "halo", T | C3_TW32, 64, 256, shape=(16, 8, 33, 65, 257), keys={14: 1}),
    _c("halo_f16_bm256", "halo", T | C3_TW32, 64, 256, shape=(16, 8, 33, 65, 257), keys={14: 1}, dt=F16),
    _c("halo_f32s_bm256_4waves", "halo", T | C3_TW32 | pf(3), 64, 256, shape=(16, 8, 33, 65, 257), keys={14: 1},
       dt=F32S),
    _c("halo_f32s_bm256_8waves_pf1", "halo", T | C3_TW32 | C3_WAVES8 | pf(1), 64, 256, shape=(16, 8, 33, 65, 257),
       keys={14: 2}, dt=F32S),
    _c("halo_f32s_bm256_8waves_pf3", "halo", T | C3_TW32 | C3_WAVES8 | pf(3), 64, 256, shape=(16, 8, 33, 65, 257),
       keys={14: 3}, dt=F32S),
    _c("halo_f32s_co33_key21_2", "halo", T | pf(2), 64, 128, shape=(1, 40, 9, 17, 33), dt=F32S, keys={21: 2}),
    _c("halo_f32s_w33_key21_4", "halo", T | pf(1), 64, 128, shape=(1, 40, 5, 33, 33), dt=F32S, keys={21: 4}),
    # f32s, tensors packed on both sides (key 28 = 0: the persistent kernel would take the Cout % 32 == 0 ones)
    _c("halo_f32s_w15_co27_ci8", "halo", T | pf(3), 32, 128, shape=(2, 8, 5, 15, 27), dt=F32S),
    _c("halo_f32s_w17_co33_ci40", "halo", T | pf(1), 64, 128, shape=(1, 40, 9, 17, 33), dt=F32S, res="same"),
    _c("halo_f32s_w33_co33_ci128", "halo", T | C3_TW32 | pf(3), 64, 128, shape=(1, 128, 5, 33, 33), dt=F32S),
    _c("halo_f32s_w33_co65_ci128", "halo", T | C3_TW32 | pf(2), 128, 128, shape=(1, 128, 5, 33, 65), dt=F32S),
    _c("halo_f32s_w17_co65_wreg", "halo", T | C3_WREG, 128, 128, shape=(1, 40, 9, 17, 65), dt=F32S, keys={20: 0}),
    _c("halo_f32s_w33_co65_8waves", "halo", T | C3_TW32 | C3_WAVES8 | pf(3), 128, 128, shape=(1, 32, 5, 33, 65),
       dt=F32S, keys={21: 1}),
    _c("halo_f32s_w17_co129_res_own", "halo", T | pf(3), 64, 128, shape=(1, 128, 9, 17, 129), dt=F32S, res="own",
       res_pitch=192, res_off=32, keys={28: 0}),
    _c("halo_f32s_co64_key28_0", "halo", T | pf(1), 64, 128, shape=(1, 32, 9, 17, 64), dt=F32S, keys={28: 0}),
    # ... plain on one side or both: only the arithmetic is f32s
    _c("halo_f32s_plain_co65", "halo", T | pf(2), 128, 128, shape=(1, 40, 9, 17, 65), dt=F32S, flags=XP | YP | RP,
       res="same"),
    _c("halo_f32s_yplain_co27", "halo", T | C3_TW32 | pf(3), 32, 128, shape=(1, 32, 5, 33, 27), dt=F32S, flags=YP),
    # fp16: 64-channel chunks; no K-skip, no four-workgroup form
    _c("halo_f16_w15_co27_ci8", "halo", T, 32, 128, shape=(2, 8, 5, 15, 27), dt=F16),
    _c("halo_f16_w17_co33_ci40", "halo", T, 64, 128, shape=(1, 40, 9, 17, 33), dt=F16, res="same"),
    _c("halo_f16_w33_co65_ci128", "halo", T | C3_TW32 | C3_WAVES8, 128, 128, shape=(1, 128, 5, 33, 65), dt=F16),
    _c("halo_f16_w17_co130_res_own", "halo", T, 64, 128, shape=(1, 128, 9, 17, 130), dt=F16, res="own",
       res_pitch=192, res_off=32),
    # ---- persistent 3x3 / s1 (key 28 = 2) -----------------------------------------------------------------------
    _c("c3p_co32", "halo", C3_PERSIST, shape=(1, 32, 9, 17, 32), dt=F32S, keys=P28),
    _c("c3p_co96_res", "halo", C3_PERSIST, shape=(2, 64, 9, 17, 96), dt=F32S, keys=P28, res="same"),
    _c("c3p_co96_res_plain", "halo", C3_PERSIST, shape=(1, 32, 9, 17, 96), dt=F32S, keys=P28, res="same", flags=RP),
    _c("c3p_co32_yplain", "halo", C3_PERSIST, shape=(1, 96, 9, 17, 32), dt=F32S, keys=P28, flags=YP),
    _c("c3p_res_own", "halo", C3_PERSIST, shape=(1, 32, 9, 17, 64), dt=F32S, keys=P28, res="own", res_pitch=128,
       res_off=32),
    # ---- persistent 3x3 / s2 (key 28 = 2) -----------------------------------------------------------------------
    _c("s2p_17x19_ci32_co96", "s2p", shape=(1, 32, 17, 19, 96), s=2, dt=F32S, keys=P28),
    _c("s2p_16x32_ci96_co32", "s2p", shape=(2, 96, 16, 32, 32), s=2, dt=F32S, keys=P28),
    _c("s2p_key33_0", "igemm", 0, 128, 64, shape=(1, 32, 17, 19, 96), s=2, dt=F32S, keys={28: 2, 33: 0}),
    # ---- cn_proj -------------------------------------------------------------------------------------------------
    _c("proj_s1_ci32_co160", "proj", shape=(1, 32, 17, 19, 160), k=(1, 1), dt=F32S),
    _c("proj_s2_ci96_co32", "proj", shape=(1, 96, 17, 19, 32), k=(1, 1), s=2, dt=F32S),
    _c("proj_m129", "proj", shape=(3, 32, 1, 43, 32), k=(1, 1), dt=F32S),
    _c("proj_yplain_co160", "proj", shape=(1, 96, 17, 19, 160), k=(1, 1), dt=F32S, flags=YP,
       out_pitch=160),
    _c("proj_key46_0", "igemm", 0, 64, 128, shape=(1, 32, 17, 19, 160), k=(1, 1), dt=F32S, keys={46: 0}),
    # ---- cn_offconv (f32s arithmetic, plain in, plain out at pitch 32) -------------------------------------------
    _c("offconv_ci32_co27", "offconv", 2, shape=(1, 32, 8, 16, 27), dt=F32S, flags=XP | YP, out_pitch=32, relu=0),
    _c("offconv_ci64_co1_split2", "offconv", 2, ksplit=2, shape=(2, 64, 8, 16, 1), dt=F32S, flags=XP | YP,
       out_pitch=32, ws=True, relu=0),
    _c("offconv_ci96_co32_split3", "offconv", 2, ksplit=3, shape=(1, 96, 16, 48, 32), dt=F32S, flags=XP | YP,
       out_pitch=32, ws=True),
    _c("offconv_one_team", "offconv", 1, shape=(1, 32, 8, 16, 27), dt=F32S, flags=XP | YP, out_pitch=32,
       keys={40: 1}),
    _c("offconv_one_team_split2", "offconv", 1, ksplit=2, shape=(1, 64, 8, 16, 27), dt=F32S, flags=XP | YP,
       out_pitch=32, keys={40: 2}, ws=True),
    _c("offconv_h12_refused", "halo", T | pf(3), 32, 128, shape=(1, 32, 12, 16, 27), dt=F32S, flags=XP | YP,
       out_pitch=32),
    _c("offconv_key39_0", "halo", T | pf(3), 32, 128, shape=(1, 32, 8, 16, 27), dt=F32S, flags=XP | YP,
       out_pitch=32, keys={39: 0}),
    # ---- 16-channel kernels (rows of whole 128-pixel tiles) ------------------------------------------------------
    _c("c16_f32_s1_co16", "conv16", shape=(1, 16, 3, 128, 16)),
    _c("c16_f32_s1_co9", "conv16", shape=(2, 16, 3, 128, 9)),
    _c("c16_f32_s2_co32", "conv16", shape=(1, 16, 5, 256, 32), s=2),
    _c("c16_f32_s2_co17", "conv16", shape=(1, 16, 5, 256, 17), s=2, out_pitch=32),
    _c("c16_f32s_s1_co32", "conv16s", shape=(1, 16, 3, 128, 32), dt=F32S, flags=XP | YP),
    _c("c16_f32s_s1_co17", "conv16s", shape=(2, 16, 3, 128, 17), dt=F32S, flags=XP | YP),
    _c("c16_f32s_s2_elsewhere", "igemm", 0, 32, 128, shape=(1, 16, 5, 256, 32), s=2, dt=F32S, flags=XP | YP),
    _c("c16_f16_s1_co16", "conv16h", shape=(1, 16, 3, 128, 16), dt=F16),
    _c("c16_f16_s2_co32", "conv16h", shape=(1, 16, 5, 256, 32), s=2, dt=F16),
    _c("c16_f16_s1_key65_0", "halo", T | C3_TW32, 32, 128, shape=(1, 16, 3, 128, 17), dt=F16, keys={65: 0},
       out_pitch=20),
    _c("c16_f32_res_on_halo", "halo", T | C3_TW32 | C3_KSKIP, 32, 128, shape=(1, 16, 3, 128, 16), res="same"),
    # ---- stems (3-channel NCHW image, 7x7) -----------------------------------------------------------------------
    _c("stem_window", "stem", STEM_WINDOW, shape=(2, 3, 20, 34, 33), k=(7, 7), s=2, stem=True),
    _c("stem_persist_s2", "stem", STEM_PERSIST, shape=(1, 3, 6, 256, 40), k=(7, 7), s=2, stem=True),
    _c("stem_persist_s1_co16", "stem", STEM_PERSIST, shape=(1, 3, 3, 128, 16), k=(7, 7), s=1, stem=True,
       keys={27: 0}, flags=CONV_STEM_F32S),
    _c("stem_persist_f32s", "stem", STEM_PERSIST_F32S, shape=(1, 3, 6, 256, 40), k=(7, 7), s=2, stem=True,
       flags=CONV_STEM_F32S),
    _c("stem_16s", "stem", STEM_16S, shape=(1, 3, 3, 128, 16), k=(7, 7), s=1, stem=True, flags=CONV_STEM_F32S),
    _c("stem_window_key12_0", "stem", STEM_WINDOW, shape=(1, 3, 6, 256, 40), k=(7, 7), s=2, stem=True,
       keys={12: 0}),
    _c("stem_nostem_key", "igemm", 0, 64, 128, shape=(1, 3, 20, 34, 33), k=(7, 7), s=2, stem=True, keys={6: 1}),
    _c("stem_f16", "igemm", 0, 128, 128, shape=(1, 3, 20, 34, 65), k=(7, 7), s=2, stem=True, dt=F16),
    # the stem + max-pool kernel: see POOL below (B is found by the host test)
    # ---- implicit GEMM -------------------------------------------------------------------------------------------
    _c("igemm_1x1_res_f32", "igemm", 0, 128, 64, shape=(1, 40, 17, 19, 72), k=(1, 1), res="same"),
    _c("igemm_3x3s2_f32", "igemm", 0, 64, 128, shape=(1, 32, 17, 19, 33), s=2),
    _c("igemm_3x3s2_f32_co27", "igemm", 0, 32, 128, shape=(2, 8, 9, 11, 27), s=2),
    _c("igemm_bm128_key4", "igemm", 0, 128, 128, shape=(1, 32, 17, 19, 72), k=(1, 1), keys={4: 128}),
    _c("igemm_nchw_f32", "igemm", 0, 128, 128, shape=(2, 64, 9, 11, 80), k=(1, 1), nchw=True, relu=0),
    _c("igemm_nchw_f32s_co2", "igemm", 0, 32, 128, shape=(1, 64, 9, 11, 2), k=(1, 1), nchw=True, relu=0, dt=F32S),
    _c("igemm_nchw_f16_co65", "igemm", 0, 128, 128, shape=(1, 64, 9, 11, 65), k=(1, 1), nchw=True, relu=0, dt=F16),
    _c("igemm_split_given_f32", "igemm", 0, 128, 64, ksplit=13, shape=(1, 384, 8, 8, 200), res="same", ws=True),
    _c("igemm_split_not_given_f32", "halo", T | C3_WAVES8, 128, 128, shape=(1, 384, 8, 8, 200), res="same"),
    _c("igemm_split_given_s2_f32", "igemm", 0, 64, 128, ksplit=4, shape=(1, 128, 15, 17, 40), s=2, ws=True),
    _c("igemm_split_not_given_s2_f32", "igemm", 0, 64, 128, shape=(1, 128, 15, 17, 40), s=2),
    _c("igemm_split_given_f32s", "igemm", 0, 128, 64, ksplit=13, shape=(1, 384, 8, 8, 200), dt=F32S, res="same",
       ws=True),
    _c("igemm_split_given_f16", "igemm", 0, 128, 64, ksplit=13, shape=(1, 768, 8, 8, 200), dt=F16, res="same",
       ws=True),
    _c("igemm_nohalo_key10", "igemm", 0, 32, 128, shape=(2, 8, 5, 15, 27), keys={10: 1}),
    # ---- the part of the descriptor no network uses --------------------------------------------------------------
    _c("desc_dil2_f32", "igemm", 0, 64, 128, shape=(1, 40, 9, 17, 33), dil=2, res="same"),
    _c("desc_dil2_f32s", "igemm", 0, 64, 128, shape=(1, 40, 9, 17, 33), dil=2, dt=F32S),
    _c("desc_dil2_f16", "igemm", 0, 64, 128, shape=(1, 40, 9, 17, 33), dil=2, dt=F16),
    _c("desc_1x3_f32", "igemm", 0, 32, 128, shape=(2, 40, 9, 17, 27), k=(1, 3), pad=(0, 1)),
    _c("desc_1x3_f32s", "igemm", 0, 32, 128, shape=(2, 40, 9, 17, 27), k=(1, 3), pad=(0, 1), dt=F32S),
    _c("desc_pad_2x1_f32", "igemm", 0, 64, 128, shape=(1, 40, 9, 17, 33), pad=(2, 1)),
    _c("desc_pad_0x1_f16", "igemm", 0, 64, 128, shape=(1, 40, 9, 17, 33), pad=(0, 1), dt=F16),
    # scalar stores: out_pitch % 4 != 0, y one float into a wider tensor, the residual likewise
    _c("scalar_pitch27_halo_f32", "halo", T | C3_KSKIP, 32, 128, shape=(1, 40, 9, 17, 27), out_pitch=27),
    _c("scalar_yoff1_halo_f32", "halo", T | C3_KSKIP, 32, 128, shape=(1, 40, 9, 17, 27), out_pitch=32, c_off=1,
       res="same"),
    _c("scalar_resoff1_halo_f32", "halo", T | C3_KSKIP, 32, 128, shape=(1, 40, 9, 17, 27), out_pitch=28, res="own",
       res_pitch=32, res_off=1),
    _c("scalar_pitch27_halo_f32s", "halo", T | pf(3), 32, 128, shape=(1, 40, 9, 17, 27), out_pitch=27, dt=F32S,
       flags=YP),
    _c("scalar_yoff1_halo_f32s", "halo", T | pf(3), 32, 128, shape=(1, 40, 9, 17, 27), out_pitch=32, c_off=1,
       dt=F32S, flags=YP | RP, res="same"),
    _c("scalar_resoff1_halo_f32s", "halo", T | pf(3), 32, 128, shape=(1, 40, 9, 17, 27), out_pitch=28, dt=F32S,
       flags=YP | RP, res="own", res_pitch=32, res_off=1),
    _c("scalar_pitch27_igemm_f32", "igemm", 0, 32, 128, shape=(1, 40, 9, 17, 27), k=(1, 1), out_pitch=27),
    _c("scalar_yoff1_igemm_f32", "igemm", 0, 32, 128, shape=(1, 40, 17, 19, 27), s=2, out_pitch=32, c_off=1),
    _c("scalar_resoff1_igemm_f32", "igemm", 0, 32, 128, shape=(1, 40, 9, 17, 27), k=(1, 1), out_pitch=28,
       res="same", res_off=1),
    _c("scalar_pitch27_igemm_f32s", "igemm", 0, 32, 128, shape=(1, 64, 9, 17, 27), k=(1, 1), out_pitch=27, dt=F32S,
       flags=YP),
    _c("scalar_resoff1_igemm_f32s", "igemm", 0, 32, 128, shape=(1, 64, 9, 17, 27), k=(1, 1), out_pitch=28, dt=F32S,
       flags=YP | RP, res="same", res_off=1),
    _c("scalar_yoff1_igemm_f32s", "igemm", 0, 32, 128, shape=(1, 64, 9, 17, 27), k=(1, 1), out_pitch=32, c_off=1,
       dt=F32S, flags=YP | RP, res="same"),
]

# ---- scatter: Cin = 512 on 8 x 8 wants a K split; a scattered call is never split, with or without the workspace
_SC_FORMS = (("f32", F32, 0, False), ("f32s_yplain", F32S, YP | RP, False), ("f32s_packed", F32S, 0, False),
             ("f16", F16, 0, False), ("nchw", F32, 0, True))
for _n, _dt, _fl, _nchw in _SC_FORMS:
    for _ws in (False, True):
        _t = "%s_%s" % (_n, "ws" if _ws else "nows")
        _kw = dict(shape=(1, 512, 8, 8, 40), dt=_dt, flags=_fl, nchw=_nchw, res=None if _nchw else "same", ws=_ws,
                   relu=0 if _nchw else 1)
        _nt = 64            # Cout = 40
        for _py in (0, 1):
            for _px in (0, 1):
                # the four parity classes of one (B, 2H, 2W) map: the GPU test runs the four into ONE map
                CASES.append(_c("scatter2_%s_p%d%d" % (_t, _py, _px), "igemm", 0, _nt, 128,
                                scatter=(2, _py, 2, _px, 16, 16), **_kw))
        CASES.append(_c("scatter1_topleft_%s" % _t, "igemm", 0, _nt, 128, scatter=(1, 0, 1, 0, 11, 13), **_kw))
        CASES.append(_c("scatter1_interior_%s" % _t, "igemm", 0, _nt, 128, scatter=(1, 2, 1, 3, 11, 13), **_kw))
# the same layer with the identity scatter does split (the contrast the scatter cases stand against)
CASES.append(_c("scatter_none_split_given", "igemm", 0, 64, 128, ksplit=16, shape=(1, 512, 8, 8, 40), res="same",
                ws=True))

# ---- refused scatters: CN_ERR_SHAPE from cn_conv2d, cn_conv2d_route and the workspace query (0 bytes) alike
for _n, _sc in (("oy_mul0", (0, 0, 1, 0, 8, 8)), ("ox_mul0", (1, 0, 0, 0, 8, 8)),
                ("oy_add_neg", (1, -1, 1, 0, 9, 8)), ("ox_add_neg", (1, 0, 1, -1, 8, 9)),
                ("oy_past", (2, 1, 1, 0, 15, 8)), ("ox_past", (1, 0, 2, 1, 8, 15)),
                ("oh_is_ho_mul2", (2, 0, 2, 0, 8, 8))):
    CASES.append(_c("refused_%s" % _n, "none", ksplit=0, rc=ERR_SHAPE, shape=(1, 512, 8, 8, 40), scatter=_sc, res="same",
                    ws=True))

# the stem + max-pool kernel: 7x7 / s2, 64 output channels, rows of one 128-pixel tile, 4 pooled rows; B is the
# smallest cn_stem_maxpool_supported accepts (tests/test_conv_route_cases_host.py scans for it: 192 strips of 4)
POOL = _c("stem_pool", "stem_pool", shape=(192, 3, 16, 256, 64), k=(7, 7), s=2, stem=True,
          flags=CONV_STEM_F32S | CONV_STEM_MAXPOOL)
CASES.append(POOL)

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- the descriptor and the pointers of a case ---------------------------------------------------------------------
def out_hw(c):
    ho = (c["H"] + 2 * c["pad_h"] - c["dil"] * (c["KH"] - 1) - 1) // c["s"] + 1
    wo = (c["W"] + 2 * c["pad_w"] - c["dil"] * (c["KW"] - 1) - 1) // c["s"] + 1
    return ho, wo


def scatter(c):
    """(oy_mul, oy_add, ox_mul, ox_add, OH, OW); the identity onto (Ho, Wo) without one"""
    ho, wo = out_hw(c)
    return c["scatter"] or (1, 0, 1, 0, ho, wo)


def packed_in(c):
    return c["dt"] == F32S and not c["flags"] & XP and not c["stem"]


def packed_out(c):
    return c["dt"] == F32S and not c["flags"] & YP and not c["nchw"]


def packed_res(c):
    return c["dt"] == F32S and not c["flags"] & RP


def pitches(c):
    """(in_pitch, out_pitch, pitch of the residual's tensor) in elements"""
    ip = 3 if c["stem"] else (r32(c["Cin"]) if packed_in(c) else c["Cin"])
    op = c["out_pitch"] or (r32(c["Cout"]) if packed_out(c) else c["Cout"])
    rp = c["res_pitch"] if c["res"] == "own" else op
    return ip, op, rp


def desc(c):
    ho, wo = out_hw(c)
    ym, ya, xm, xa, OH, OW = scatter(c)
    ip, op, rp = pitches(c)
    d = native.ConvDesc(B=c["B"], H=c["H"], W=c["W"], Cin=c["Cin"], Ho=ho, Wo=wo, Cout=c["Cout"], KH=c["KH"],
                        KW=c["KW"], stride=c["s"], pad_h=c["pad_h"], pad_w=c["pad_w"], dil=c["dil"],
                        in_layout=LAYOUT_NCHW if c["stem"] else LAYOUT_NHWC, in_pitch=ip,
                        out_layout=LAYOUT_NCHW if c["nchw"] else LAYOUT_NHWC, out_pitch=op, OH=OH, OW=OW,
                        oy_mul=ym, oy_add=ya, ox_mul=xm, ox_add=xa, relu=c["relu"], dtype=DTYPES[c["dt"]],
                        flags=c["flags"], res_pitch=rp if c["res"] == "own" else 0)
    d.ctl.x_mul = d.ctl.res_mul = 1.0
    return d


def elem_bytes(c, which):
    """bytes per element of "x", "y" or "res" """
    if c["dt"] != F16:
        return 4
    if which == "y":
        return 4 if (c["nchw"] or c["flags"] & YP) else 2
    return 4 if (which == "x" and c["stem"]) else 2


def query(c, x, w, scale, shift, res, y, ws, ws_bytes):
    """(status, ConvRouteInfo) of the case's call with these addresses, under the case's keys"""
    d = desc(c)
    info = native.ConvRouteInfo()
    vp = ctypes.c_void_p
    with native.tuning(c["keys"]):
        rc = native.lib().cn_conv2d_route(ctypes.byref(d), vp(x), vp(w), vp(scale), vp(shift), vp(res), vp(y),
                                          vp(ws), ws_bytes, None, ctypes.byref(info))
    return rc, info


def workspace_bytes(c):
    with native.tuning(c["keys"]):
        return int(native.lib().cn_conv2d_workspace_bytes(ctypes.byref(desc(c))))


def fake_pointers(c):
    """addresses for a host-only query: every tensor 256-byte aligned, y and the residual moved to their channel"""
    y = 0x7000_0000_0000 + c["c_off"] * elem_bytes(c, "y")
    res = (0x7100_0000_0000 + c["res_off"] * elem_bytes(c, "res")) if c["res"] else None
    need = workspace_bytes(c)
    ws = 0x7200_0000_0000 if (c["ws"] and need) else None
    return dict(x=0x7300_0000_0000, w=0x7400_0000_0000, scale=0x7500_0000_0000, shift=0x7500_0001_0000, res=res,
                y=y, ws=ws, ws_bytes=need if ws else 0)


def expected(c):
    return (c["rc"], c["route"], c["variant"], c["n_tile"], c["m_tile"], c["ksplit"])


def said(rc, info):
    return (rc, native.conv_route_name(info.route), info.variant, info.n_tile, info.m_tile, info.ksplit)


def variant_name(route, v):
    if route == "halo":
        if v == C3_PERSIST:
            return "persistent"
        bits = [n for b, n in ((C3_TW32, "tw32"), (C3_WAVES8, "waves8"), (C3_OCC4, "occ4"), (C3_KSKIP, "kskip"),
                               (C3_WREG, "wreg")) if v & b]
        return "tile" + "".join("+" + b for b in bits) + ("+pf%d" % native.c3_prefetch(v) if v >> 12 else "")
    if route == "stem":
        return ("none", "window", "persist", "persist_f32s", "16s")[v]
    if route == "offconv":
        return "%d team%s" % (v, "s" * (v > 1))
    return ""


def pins():
    """{(route, variant name, "m_tile x n_tile" or ""): [case ids]}: which cases pin which kernel form"""
    out = {}
    for c in CASES:
        tile = "%dx%d" % (c["m_tile"], c["n_tile"]) if c["m_tile"] else ""
        out.setdefault((c["route"], variant_name(c["route"], c["variant"]), tile), []).append(c["id"])
    return out


if __name__ == "__main__":      # python tests/conv_route_cases.py: the list, per route and variant
    for (route, var, tile), ids in sorted(pins().items()):
        print("%-9s %-22s %-8s %s" % (route, var, tile, " ".join(ids)))
