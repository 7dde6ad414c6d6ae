// cn_dcn.hip -- the NHWC entry of the modulated deformable convolution (DCNv2): argument checks, the one call
// description (DcnCall, cn_internal.h), the one route, the switch over its forms, and the two host queries that
// read the same route.  No kernel lives here: the gather forms are the implicit GEMM's (cn_conv.hip, cn_dcn_gather),
// the f32s LDS-window forms are cn_dcn2.hip / cn_dcn3.hip / cn_dcn4.hip, the fp16 LDS-window form cn_dcn_h.hip.
#include "cn_internal.h"
#include "cn_tuning.h"

namespace {

inline int round_up32(int v) { return (v + 31) / 32 * 32; }
inline size_t slab_bytes(const DcnCall &c) { return (size_t)c.B * c.H * c.W * round_up32(c.Cout) * sizeof(float); }

// Tap-split factor of the gather form: the gather makes every K chunk latency-bound, so a
// layer needs ~4 workgroups per CU to keep the matrix cores busy; small maps get them by
// splitting the 9 taps over 3 or 9 workgroups per tile (fp32 partial sums + reduce kernel).
int dcn_ksplit(int B, int H, int W, int Cout)
{
    if (cn_knobs.nosplit || cn_knobs.dcn_split == 1) return 1;
    if (cn_knobs.dcn_split == 3 || cn_knobs.dcn_split == 9) return cn_knobs.dcn_split;
    const long wgs = (long)cn_cdiv(B * H * W, 64) * cn_cdiv(Cout, Cout > 64 ? 128 : 64);
    if (wgs >= 1024) return 1;
    return wgs * 3 >= 600 ? 3 : 9;  // measured (tools/bench_dcn.py): 3 wins from ~2 workgroups/CU
}

// K split of the LDS-window forms.  Too few tiles for the chip but a deep K (512 -> 256 @ 16^2): split the
// 32-channel chunks over 2 / 4 / 8 workgroups per tile -- raw fp32 partial sums in the caller's workspace, summed
// in a fixed order by the reduce launch (deterministic).  The smallest split that reaches `target` workgroups, else
// the deepest one that divides the chunks, leaves two per workgroup and fits the workspace.  Needs an aligned
// workspace and key 5 clear.
int dcnw_pick_ksplit(long wgs, int target, const DcnCall &c)
{
    if (!c.workspace || !cn_aligned16(c.workspace) || cn_knobs.nosplit) return 1;
    const int nchunk = c.Cin / 32;
    int ksplit = 1;
    for (int s2 = 2; s2 <= 8 && wgs * ksplit < target; s2 *= 2)
        if (nchunk % s2 == 0 && nchunk / s2 >= 2 && s2 * slab_bytes(c) <= c.workspace_bytes) ksplit = s2;
    return ksplit;
}

// the register-sampling window form splits K until a launch has this many workgroups (round-4 sweep of 256 / 512 /
// 1024 and of 64-wide N tiles for Cout > 64: within +-5 % on every layer shape, profiles/r04_dcn_split_sweep.txt)
constexpr int WINDOW_SPLIT_WGS = 256;
constexpr int WINDOW_MIN_WGS = 192;     // ... and, unless forced, leaves grids below this many to the gather form

DcnPlan window_plan(const DcnCall &c, int form, int bn, long tiles, int target)
{
    DcnPlan p = {};
    p.form = form;
    p.bn = bn;
    p.grid_x = (unsigned)tiles;
    p.grid_y = (unsigned)cn_cdiv(c.Cout, bn);
    p.ksplit = dcnw_pick_ksplit(tiles * p.grid_y, target, c);
    return p;
}

}  // namespace

// Which form runs a call and how it is laid out.  Everything the entry, the launchers and the queries need to
// know is decided here, from the call and cn_knobs alone.
DcnPlan dcn_route(const DcnCall &c)
{
    const CnTuning &k = cn_knobs;
    const int forced = k.dcn_form;                           // cn_set_tuning key 23
    const long tiles = (long)c.B * (c.H / 8) * (c.W / 16);   // 8 x 16 pixel tiles of the window forms
    if (c.dtype == CN_DTYPE_F32S && forced != 1) {
        // The order of preference: wide, team, window, gather.  Auto (key 23 = 0): wide and team only on grids
        // that fill the chip (wide: key 41, team: key 36), window only on grids the gather form's tap split does
        // not serve better.  A forced form that does not take the shape goes straight to the gather form.
        const bool fills = forced == 0 && tiles >= 64;
        const bool wide_auto = fills && k.dcn_wide && (c.Cout & 127) == 0 && !k.dbgskip;
        const bool team_auto = fills && ((k.dcn_team == 1 && c.Cout <= 64) || k.dcn_team >= 2);
        if ((forced == 6 || forced == 7 || wide_auto) && cn_dcn_wide_takes(c)) {
            // eight 32-channel blocks per workgroup where Cout allows (the grid is not looked at: one too small
            // for the chip gets the K split), four when forced by key 23 = 7
            const int nb = (forced != 7 && c.Cout % 256 == 0) ? 8 : 4;
            DcnPlan p = window_plan(c, nb == 8 ? DCN_WIDE8 : DCN_WIDE4, 32 * nb, tiles, k.dcn_wide_wgs);
            // L2 prefetch: pays where the weight stream is long and cold (four-block form on deep K: +5 % cold); costs 1-4 % elsewhere
            p.prefetch = (k.dcn_wide_prefetch && nb == 4 && c.Cin >= 256) ? 1 : 0;
            return p;
        }
        if ((forced == 4 || forced == 5 || team_auto) && cn_dcn_team_takes(c)) {
            // N mode (the teams split a 128-channel block) halves the workgroup count: unless forced, only where
            // two workgroups per CU remain (measured: 256 -> 128 @ 32^2 at B = 32 has 256 tiles: 0.093 ms in T
            // mode, 0.109 in N mode; 128 -> 128 @ 64^2 and 256 -> 256 @ 32^2: 0.179 / 0.172 against 0.195 / 0.209)
            const bool nmode = (c.Cout & 127) == 0 &&
                               (forced == 5 || (team_auto && k.dcn_team == 3 && tiles * (c.Cout / 128) >= k.dcn_team_wgs));
            DcnPlan p = window_plan(c, nmode ? DCN_TEAM_N : DCN_TEAM_T, nmode ? 128 : 64, tiles, k.dcn_team_wgs);
            p.stagger = k.dcn_team_stagger;
            return p;
        }
        if (forced < 4 && cn_dcn_window_takes(c)) {
            const DcnPlan p = window_plan(c, DCN_WINDOW, c.Cout > 64 ? 128 : 64, tiles, WINDOW_SPLIT_WGS);
            const long wgs = tiles * p.grid_y;
            if (wgs * p.ksplit >= WINDOW_SPLIT_WGS || wgs >= (forced ? 1 : WINDOW_MIN_WGS)) return p;
        }
    }
    if (c.dtype == CN_DTYPE_F16 && forced != 1 && cn_dcn_half_window_takes(c)) {
        // fp16 LDS-window form (key 23: 0 = auto, 2 = forced, 1 = gather).  It has no K split: as for the f32s
        // register-sampling form, grids below WINDOW_MIN_WGS go to the gather form and its tap split unless forced
        DcnPlan p = {};
        p.form = DCNH_WINDOW;
        p.bn = c.Cout > 64 ? 128 : 64;
        p.grid_x = (unsigned)tiles;
        p.grid_y = (unsigned)cn_cdiv(c.Cout, p.bn);
        p.ksplit = 1;
        if (forced == 2 || tiles * p.grid_y >= WINDOW_MIN_WGS) return p;
    }
    // the gather form: 64-pixel tiles by 128 / 64 output channels, 128-pixel tiles at <= 32 output channels
    DcnPlan p = {};
    // (_PAD: the last K chunk -- 32 channels, 64 in fp16 mode -- is partial)
    p.form = (c.Cin & (c.dtype == CN_DTYPE_F16 ? 63 : 31)) ? DCN_GATHER_PAD : DCN_GATHER;
    p.bn = c.Cout > 64 ? 128 : (c.Cout > 32 ? 64 : 32);
    p.grid_x = (unsigned)cn_cdiv(c.B * c.H * c.W, c.Cout > 32 ? 64 : 128);
    p.grid_y = (unsigned)cn_cdiv(c.Cout, p.bn);
    p.vec_out = ((c.Cout & 3) == 0 && (c.out_pitch & 3) == 0 && cn_aligned16(c.y)) ? 1 : 0;
    // tiles as pixel blocks (8 x 8, or 8 x 16 for the 128-pixel tiles of Cout <= 32) when the map
    // divides into them
    p.tile2d = (k.dcn_tile2d && (c.W & 7) == 0 && (c.H % (c.Cout > 32 ? 8 : 16)) == 0) ? 1 : 0;
    // tap split (needs the caller's workspace; without one that holds all slabs the layer runs unsplit)
    p.ksplit = 1;
    if (c.Cout > 32) {
        const int want = dcn_ksplit(c.B, c.H, c.W, c.Cout);
        if (want > 1 && c.workspace && c.workspace_bytes >= want * slab_bytes(c) && cn_aligned16(c.workspace))
            p.ksplit = want;
    }
    return p;
}

// The allowance a caller should give, not what the route of one dtype needs: slabs of the gather form's tap split
// (3 / 9), and never fewer than the 8 of the window forms' deepest split.  The code relies on this relation: at
// the default keys, a caller who gives this many bytes never has a split cut short by workspace_bytes.  It holds
// because, at the default keys, every call whose route splits (gather: plain grid < 1024 workgroups; window forms:
// fewer tiles x blocks than their 256 / 512 / 256 targets, of 128-pixel tiles where dcn_ksplit counts 64-pixel
// ones) also has dcn_ksplit > 1 here (tests/test_dcn_route_host.py checks it over its grid).
extern "C" size_t cn_dcn_v2_forward_nhwc_workspace_bytes(int B, int Cin, int H, int W, int Cout)
{
    if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
    const int s = dcn_ksplit(B, H, W, Cout);
    return s > 1 ? (size_t)(s > 8 ? s : 8) * B * H * W * round_up32(Cout) * sizeof(float) : 0;
}

// the argument checks of the entries and the one place that fills the call description.  CN_DTYPE_F16 comes from
// the typed half entries only (cn_dcn_v2_forward_nhwc_f16 / cn_dcn_v2_route_f16, whose x and y are halves): the
// dtype-generic entries take float pointers and refuse it, as they always have
static int dcn_fill(DcnCall &c, const float *input_nhwc, const void *weight_packed, const float *bias,
                    const float *offset_mask_nhwc, int om_pitch, const float *scale, const float *shift,
                    void *output_nhwc, int out_pitch, int B, int Cin, int H, int W, int Cout, int mask_sigmoid,
                    int relu, int dtype, int flags, const cn_f32s_ctl *ctl, void *workspace, size_t workspace_bytes,
                    bool half_entry = false)
{
    if (!input_nhwc || !weight_packed || !offset_mask_nhwc || !output_nhwc) return CN_ERR_NULL;
    if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || out_pitch < Cout) return CN_ERR_SHAPE;
    if (om_pitch < 27) return CN_ERR_SHAPE;
    const bool f32s = (dtype == CN_DTYPE_F32S), f16 = (dtype == CN_DTYPE_F16);
    if (dtype != CN_DTYPE_F32 && !f32s && !(f16 && half_entry)) return CN_ERR_UNSUPPORTED;
    // every bilinear corner is a 16-byte gather: 4 floats, or 8 halves in fp16 mode (x, w and y are halves there;
    // offsets / masks, bias, scale and shift stay fp32)
    if ((Cin & (f16 ? 7 : 3)) != 0) return CN_ERR_UNSUPPORTED;
    if (f32s && !(flags & CN_CONV_Y_PLAIN) && (out_pitch & 31)) return CN_ERR_UNSUPPORTED;
    if (!cn_aligned16(input_nhwc) || !cn_aligned16(weight_packed)) return CN_ERR_ALIGN;
    // f32s tensors are addressed in 128-byte groups of 32 channels
    if (f32s && !(flags & CN_CONV_Y_PLAIN) && (((uintptr_t)output_nhwc) & 127u)) return CN_ERR_ALIGN;
    if ((long)B * H * W * (long)(Cin > out_pitch ? Cin : out_pitch) >= (1L << 30)) return CN_ERR_UNSUPPORTED;  // 32-bit byte offsets
    c = {};
    c.x = input_nhwc; c.w = weight_packed; c.bias = bias; c.om = offset_mask_nhwc; c.om_pitch = om_pitch;
    c.scale = scale; c.shift = shift; c.y = output_nhwc; c.out_pitch = out_pitch;
    c.out_plain = (flags & CN_CONV_Y_PLAIN) ? 1 : 0;
    c.B = B; c.Cin = Cin; c.H = H; c.W = W; c.Cout = Cout; c.mask_sigmoid = mask_sigmoid; c.relu = relu;
    c.dtype = dtype;
    c.x_mul = (ctl && ctl->x_mul != 0.f) ? ctl->x_mul : 1.f;
    c.range = ctl ? ctl->range : nullptr;
    c.dbg = cn_knobs.dbgskip;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return CN_OK;
}

static void dcn_info(const DcnCall &c, cn_dcn_route_info *info);
static int dcn_launch(const DcnCall &c, hipStream_t st);

extern "C" int cn_dcn_v2_route(const float *input_nhwc, const void *weight_packed, const float *bias,
                               const float *offset_mask_nhwc, int om_pitch, const float *scale,
                               const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                               int H, int W, int Cout, int mask_sigmoid, int relu, int dtype, int flags,
                               const cn_f32s_ctl *ctl, void *workspace, size_t workspace_bytes,
                               void *stream, cn_dcn_route_info *info)
{
    (void)stream;
    if (!info) return CN_ERR_NULL;
    (void)ctl;   // not followed either: the route does not depend on it
    DcnCall c;
    const int rc = dcn_fill(c, input_nhwc, weight_packed, bias, offset_mask_nhwc, om_pitch, scale, shift, output_nhwc,
                            out_pitch, B, Cin, H, W, Cout, mask_sigmoid, relu, dtype, flags, nullptr, workspace,
                            workspace_bytes);
    if (rc != CN_OK) return rc;
    dcn_info(c, info);
    return CN_OK;
}

static void dcn_info(const DcnCall &c, cn_dcn_route_info *info)
{
    const DcnPlan p = dcn_route(c);
    info->form = p.form;
    info->grid_x = (int)p.grid_x;
    info->grid_y = (int)p.grid_y;
    info->ksplit = p.ksplit;
    info->flags = (p.prefetch ? CN_DCN_FLAG_PREFETCH : 0) | (p.stagger ? CN_DCN_FLAG_STAGGER : 0) |
                  (p.tile2d ? CN_DCN_FLAG_TILE2D : 0) | (p.vec_out ? CN_DCN_FLAG_VEC_OUT : 0);
}

extern "C" int cn_dcn_v2_forward_nhwc(const float *input_nhwc, const void *weight_packed,
                                      const float *bias, const float *offset_mask_nhwc,
                                      int om_pitch, const float *scale, const float *shift,
                                      void *output_nhwc, int out_pitch, int B, int Cin, int H,
                                      int W, int Cout, int mask_sigmoid, int relu, int dtype,
                                      int flags, const cn_f32s_ctl *ctl, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    DcnCall c;
    const int rc = dcn_fill(c, input_nhwc, weight_packed, bias, offset_mask_nhwc, om_pitch, scale, shift, output_nhwc,
                            out_pitch, B, Cin, H, W, Cout, mask_sigmoid, relu, dtype, flags, ctl, workspace, workspace_bytes);
    if (rc != CN_OK) return rc;
    return dcn_launch(c, (hipStream_t)stream);
}

// route the call and run its form (and the reduce launch behind a split)
static int dcn_launch(const DcnCall &c, hipStream_t st)
{
    const DcnPlan p = dcn_route(c);
    int rc;
    switch (p.form) {
    case DCN_WIDE4: case DCN_WIDE8: rc = cn_dcn_wide_f32s(c, p, st); break;
    case DCN_TEAM_T: case DCN_TEAM_N: rc = cn_dcn_team_f32s(c, p, st); break;
    case DCN_WINDOW: rc = cn_dcn_window_f32s(c, p, st); break;
    case DCNH_WINDOW: rc = cn_dcn_window_f16(c, p, st); break;
    default: rc = cn_dcn_gather(c, p, st); break;
    }
    if (rc != CN_OK || p.ksplit == 1) return rc;
    // second stage of the split: fixed-order sum of the slabs + the usual epilogue
    return cn_dcn_reduce(c, p.ksplit, st);
}

extern "C" int cn_dcn_v2_forward_nhwc_f32(const float *input_nhwc, const float *weight_packed,
                                          const float *bias, const float *offset_mask_nhwc,
                                          int om_pitch, const float *scale, const float *shift,
                                          float *output_nhwc, int B, int Cin, int H, int W,
                                          int Cout, int mask_sigmoid, int relu, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    return cn_dcn_v2_forward_nhwc(input_nhwc, weight_packed, bias, offset_mask_nhwc, om_pitch, scale,
                                  shift, output_nhwc, Cout, B, Cin, H, W, Cout, mask_sigmoid, relu,
                                  CN_DTYPE_F32, 0, nullptr, workspace, workspace_bytes, stream);
}

// ---- fp16 compute mode: x, the packed weight (cn_pack_conv_weight(..., CN_DTYPE_F16)) and y are halves; offsets /
// masks, bias, scale and shift fp32.  The same call description, route and forms as above with dtype = CN_DTYPE_F16.
extern "C" int cn_dcn_v2_forward_nhwc_f16(const void *input_nhwc, const void *weight_packed, const float *bias,
                                          const float *offset_mask_nhwc, int om_pitch, const float *scale,
                                          const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                                          int H, int W, int Cout, int mask_sigmoid, int relu, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    DcnCall c;
    const int rc = dcn_fill(c, (const float *)input_nhwc, weight_packed, bias, offset_mask_nhwc, om_pitch, scale, shift,
                            output_nhwc, out_pitch, B, Cin, H, W, Cout, mask_sigmoid, relu, CN_DTYPE_F16, 0, nullptr,
                            workspace, workspace_bytes, true);
    if (rc != CN_OK) return rc;
    return dcn_launch(c, (hipStream_t)stream);
}

// Canvas batches: image b owns the rectangle rects_dev[b] >> shift of the (H, W) tensor, and its
// sampling positions are formed relative to that rectangle's origin, then moved back by whole pixels -- the
// fractions, and with them every rounding, are those of the image's own forward wherever the rectangle lies.
// The same route and forms; a null table is cn_dcn_v2_forward_nhwc_f16.
extern "C" int cn_dcn_v2_forward_nhwc_f16_rects(const void *input_nhwc, const void *weight_packed, const float *bias,
                                                const float *offset_mask_nhwc, int om_pitch, const float *scale,
                                                const float *shift, void *output_nhwc, int out_pitch, int B,
                                                int Cin, int H, int W, int Cout, int mask_sigmoid, int relu,
                                                void *workspace, size_t workspace_bytes,
                                                const cn_rect *rects_dev, int rect_shift, void *stream)
{
    if (rect_shift < 0 || rect_shift > 30) return CN_ERR_SHAPE;
    DcnCall c;
    const int rc = dcn_fill(c, (const float *)input_nhwc, weight_packed, bias, offset_mask_nhwc, om_pitch, scale, shift,
                            output_nhwc, out_pitch, B, Cin, H, W, Cout, mask_sigmoid, relu, CN_DTYPE_F16, 0, nullptr,
                            workspace, workspace_bytes, true);
    if (rc != CN_OK) return rc;
    c.rects = rects_dev;
    c.rect_shift = rect_shift;
    return dcn_launch(c, (hipStream_t)stream);
}

extern "C" int cn_dcn_v2_route_f16(const void *input_nhwc, const void *weight_packed, const float *bias,
                                   const float *offset_mask_nhwc, int om_pitch, const float *scale,
                                   const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                                   int H, int W, int Cout, int mask_sigmoid, int relu, void *workspace,
                                   size_t workspace_bytes, void *stream, cn_dcn_route_info *info)
{
    (void)stream;
    if (!info) return CN_ERR_NULL;
    DcnCall c;
    const int rc = dcn_fill(c, (const float *)input_nhwc, weight_packed, bias, offset_mask_nhwc, om_pitch, scale, shift,
                            output_nhwc, out_pitch, B, Cin, H, W, Cout, mask_sigmoid, relu, CN_DTYPE_F16, 0, nullptr,
                            workspace, workspace_bytes, true);
    if (rc != CN_OK) return rc;
    dcn_info(c, info);
    return CN_OK;
}
