// cn_internal.h -- prototypes of the functions one .hip file defines and another calls, and the two call
// descriptions they pass (ConvCall: the convolution family, DcnCall: the deformable convolution, TopkCall: the
// top-K of the decoders).  Included
// by both sides, so the defining file is compiled against the declaration its callers see.
#pragma once
#include "cn_common.h"

// ---- the convolution family: one call description.  cn_conv.hip fills it once per cn_conv2d /
// cn_conv_transpose4x4s2 call (after the descriptor checks); conv_route() there and every launcher and `takes`
// predicate below read it.  An extra argument only for what is not a fact of the call (tile class, tuning key).
// "Describe, don't launch": what cn_conv2d_route hands a routed file.  A launcher that finds one in its call fills it
// at the point where it would launch -- from the same template arguments and grid -- and returns without touching the
// device; cn_conv2d never sets one.  variant: the CN_C3_* bits, a CN_STEM_* form or the teams of cn_offconv
struct ConvForm { int variant, n_tile, m_tile, grid_x, grid_y; };
struct ConvCall {
    const void *x, *w;                    // tensors of `dtype` (the stem: fp32 NCHW image and fp32 weights)
    const float *scale, *shift;
    const void *residual;
    void *y;
    int B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_h, pad_w, dil;
    int in_pitch, out_pitch, res_pitch;   // floats per pixel; res_pitch is resolved (never 0)
    int relu, dtype;                      // CN_DTYPE_*
    int in_plain, out_plain, res_plain;   // CN_CONV_X_PLAIN / Y_PLAIN / R_PLAIN
    int stem, stem_f32s, stem_pool, stem_y_f32s;   // 3-channel NCHW image; CN_CONV_STEM_F32S / _MAXPOOL / _Y_F32S
    int out_nchw, plain_geo;              // plain_geo: output pixel (oy, ox) goes to (oy, ox) of a (B, Ho, Wo) map
    int vec_out;                          // y (and the residual) allow 4-element vector stores
    const cn_f32s_ctl *ctl;               // may be null
    int ksplit;                           // K slices of this launch (1 = no split)
    float *partial;                       // split-K workspace when ksplit > 1
    int cin_pad, cout_pad, nchunk;        // packed weight: K per tap (stem: of all taps), rows per tap, K chunks
    ConvForm *describe;                   // cn_conv2d_route only (above); null: launch
};

// ---- cn_stem.hip
int cn_stem_pool_rows(const ConvCall &c);   // pooled rows per strip of the stem + max-pool kernel, 0 = not taken
int cn_stem_pool_f32s(const ConvCall &c, hipStream_t st);
// the kernel cn_stem_conv_f32 runs for the call: CN_STEM_* of include/centernet_amd.h; persistent: cn_set_tuning key 12
int cn_stem_form(const ConvCall &c, int persistent);
int cn_stem_conv_f32(const ConvCall &c, int persistent, hipStream_t st);

// ---- the deformable convolution (NHWC entry): one call description.  cn_dcn.hip fills it once per
// cn_dcn_v2_forward_nhwc call (after the argument checks); dcn_route() there says which form runs and how it is
// laid out, and every `takes` predicate and launcher below reads the call and the plan.  The forms: the global
// gather of the implicit GEMM (cn_conv.hip, every dtype) and the three f32s LDS-window forms (cn_dcn2.hip
// register-sampling window, cn_dcn3.hip team, cn_dcn4.hip wide; what those share is in cn_dcn_window.h)
struct DcnCall {
    const float *x;            // (B, H, W, Cin) plain fp32; CN_DTYPE_F16 (the _f16 entries): the pointer addresses halves
    const void *w;             // packed weights of `dtype` (f32s: row form + fragment copy)
    const float *bias, *om;    // om: (B, H, W, om_pitch): 18 offsets + 9 masks per pixel
    int om_pitch;
    const float *scale, *shift;
    void *y;
    int out_pitch, out_plain;
    int B, Cin, H, W, Cout, mask_sigmoid, relu;
    int dtype;                 // CN_DTYPE_F32 / CN_DTYPE_F32S / CN_DTYPE_F16
    float x_mul;               // cn_f32s_ctl resolved: f32s input exponent (a power of two, 1 without a ctl)
    uint32_t *range;           // ... and the range words of the launch, or null
    int dbg;                   // cn_set_tuning key 9
    void *workspace;           // as the caller gave them; whether they allow a split is the route's to judge
    size_t workspace_bytes;
    // canvas batches (cn_dcn_v2_forward_nhwc_f16_rects): image b's own origin is (rects[b].x0, rects[b].y0) >> rect_shift
    // and a sampling position is formed relative to it, as the image's own forward forms it; null: the tensor's origin
    const cn_rect *rects;
    int rect_shift;
};
// the values of cn_dcn_route_info::form (include/centernet_amd.h)
enum { DCN_GATHER = CN_DCN_GATHER, DCN_GATHER_PAD = CN_DCN_GATHER_PAD, DCN_WINDOW = CN_DCN_WINDOW,
       DCN_TEAM_T = CN_DCN_TEAM_T, DCN_TEAM_N = CN_DCN_TEAM_N, DCN_WIDE4 = CN_DCN_WIDE4, DCN_WIDE8 = CN_DCN_WIDE8,
       DCNH_WINDOW = CN_DCNH_WINDOW };
struct DcnPlan {
    int form;                  // DCN_*
    int bn;                    // output channels per block
    unsigned grid_x, grid_y;   // tiles, blocks of output channels (cdiv(Cout, bn))
    int ksplit;                // grid.z; > 1: the form writes that many [B*H*W][cout_pad] slabs of raw sums into the
                               // workspace and cn_dcn_reduce follows
    int prefetch, stagger;     // wide: L2 prefetch of the weights; team: start delay of the second occupant
    int tile2d, vec_out;       // gather: tiles are pixel blocks; y allows 16-byte stores
};
DcnPlan dcn_route(const DcnCall &c);   // cn_dcn.hip: pure host function of the call and cn_knobs; launches nothing
// `takes`: the shapes and pointers a window form serves (dcn_route asks in its order of preference).  A launcher
// runs the plan it is given and nothing else: one that is not its own is a bug, not a fallback
bool cn_dcn_window_takes(const DcnCall &c);
bool cn_dcn_team_takes(const DcnCall &c);
bool cn_dcn_wide_takes(const DcnCall &c);
int cn_dcn_window_f32s(const DcnCall &c, const DcnPlan &p, hipStream_t st);
int cn_dcn_team_f32s(const DcnCall &c, const DcnPlan &p, hipStream_t st);
int cn_dcn_wide_f32s(const DcnCall &c, const DcnPlan &p, hipStream_t st);
// cn_dcn_h.hip: the fp16 LDS-window form (CN_DTYPE_F16 calls only; never split: p.ksplit == 1)
bool cn_dcn_half_window_takes(const DcnCall &c);
int cn_dcn_window_f16(const DcnCall &c, const DcnPlan &p, hipStream_t st);
// cn_conv.hip, bound to igemm_kernel: the gather forms, and the second stage of every form's split
int cn_dcn_gather(const DcnCall &c, const DcnPlan &p, hipStream_t st);
int cn_dcn_reduce(const DcnCall &c, int ksplit, hipStream_t st);

// ---- cn_decode.hip: the top-K of a heat-map, one call description.  Every entry that ranks a heat-map fills a
// TopkCall; topk_route() says which form the call takes and where its scratch lives, topk_run() checks, asks
// the route and launches.  cn_decode_tasks.hip (pose, ddd, exct, agnex) reaches the top-K through these.
enum { MODE_CTDET = 0, MODE_CHANNEL = 1, MODE_POSE = 2, MODE_TOPK = 3 };   // what the K rows become
struct EmitArgs {              // outputs of the K rows (emit_rows in cn_decode.hip); unused ones null / 0
    const float *wh, *reg;
    int cat_spec_wh;
    int J;                     // MODE_POSE: joints of kps_map
    float *dets;               // rows of 6 + 2J floats: box, score, 2J keypoint coordinates, class
    int32_t *inds_out;
    float *out_scores;
    int32_t *cls_out;
    const float *kps_map;      // MODE_POSE: (B, 2J, H, W)
};
struct TopkCall {
    const float *heat;         // (B, C, H, W)
    int B, C, H, W, K;
    int flags;                 // the entry's CN_DECODE_* bits
    int mode;                  // MODE_*
    EmitArgs ea;
    void *workspace;
    size_t workspace_bytes;
    bool cand_only;            // the workspace holds the per-band candidate arrays only (the pose stages, which
                               // never take an image-level form); else it must hold TopkPlan::total
    hipStream_t st;
};
enum { TOPK_ONE_LAUNCH, TOPK_TWO_LAUNCHES, TOPK_BAND_MERGE, TOPK_BAND_DIRECT };
struct TopkPlan {
    int rc;                    // CN_OK, or why the shape has no plan (then nothing else is set)
    int form;                  // TOPK_*
    int R, nbands;             // per-band select: rows per band, bands per plane
    size_t lds;                // its dynamic LDS bytes
    int nrg, ncb;              // image-level forms: 8-row groups per plane, 128-column blocks per row
    int cap;                   // candidate keys per image
    // byte offsets in the workspace: the per-band candidate arrays, then the image-level scratch
    size_t cand_score, cand_idx, cand_bytes;
    size_t gpeak, gall, counts, done, floorv, pcount, keys;
    size_t total;              // what cn_ctdet_decode_workspace_bytes answers: the same for every mode and flag
    size_t state_offset, state_bytes;   // TOPK_ONE_LAUNCH: counts | done | floorv, zero between calls; else 0, 0
    bool fill_state;           // ... and the call zeroes them itself (no CN_DECODE_STATE_CLEAN)
};
TopkPlan topk_route(const TopkCall &c);   // pure host function of the shapes, the mode and the flags
int topk_checks(const TopkCall &c);       // the shape / pointer checks every top-K entry starts with
int topk_run(const TopkCall &c);          // topk_checks, the mode's output and workspace checks, route, launch

// ---- cn_dcn_general.hip
int cn_dcn_general_launch(const float *input, const float *weight, const float *bias,
                          const float *offset, const float *mask, float *output, int B, int Cin,
                          int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                          int dh, int dw, int dg, int mask_sigmoid, hipStream_t st);

// ---- cn_offconv.hip (f32s, plain in / plain out, <= 32 output channels; ksplit: the slices the launch would get)
bool cn_offconv_takes(const ConvCall &c, int ksplit);
int cn_offconv_f32s(const ConvCall &c, hipStream_t st);

// ---- cn_proj.hip (f32s 1x1, stride 1 or 2)
bool cn_proj1x1_takes(const ConvCall &c);
int cn_proj1x1_f32s(const ConvCall &c, hipStream_t st);

// ---- cn_conv16.hip (3x3 / pad 1 with 16 input and <= 32 output channels; fp32, or f32s arithmetic on plain tensors)
bool cn_conv16_takes(const ConvCall &c);
int cn_conv3x3_c16(const ConvCall &c, hipStream_t st);
int cn_conv3x3_c16s(const ConvCall &c, hipStream_t st);
// ... and its half form (CN_DTYPE_F16 tensors, stride 1 and 2)
bool cn_conv16h_takes(const ConvCall &c);
int cn_conv3x3_c16h(const ConvCall &c, hipStream_t st);

// ---- cn_conv3x3.hip (LDS-halo kernel); each forwards the call to cn_conv3x3p.hip when that kernel takes it
// bn_class: 2 = 128-wide N tiles, 1 = 64, 0 = 32 (conv_route's)
int cn_conv3x3s1(const ConvCall &c, int bn_class, hipStream_t st);
int cn_deconv4x4s2_halo(const ConvCall &c, hipStream_t st);

// ---- cn_conv3x3p.hip (persistent loader / consumer kernel)
bool cn_conv3x3p_takes(const ConvCall &c);
int cn_conv3x3s1_persist(const ConvCall &c, hipStream_t st);
bool cn_conv3x3s2p_takes(const ConvCall &c);
int cn_conv3x3s2_persist(const ConvCall &c, hipStream_t st);
bool cn_deconv4x4s2p_takes(const ConvCall &c);
int cn_deconv4x4s2_persist(const ConvCall &c, hipStream_t st);
bool cn_heads3x3p_takes(int B, int H, int W, int in_pitch, int head_conv, int n_heads, const cn_head_out *heads,
                        bool in_plain);
int cn_heads3x3p(const void *x, int B, int H, int W, int Cin, int in_pitch, const void *w1_packed,
                 const float *scale1, const float *bias1, int n_heads, const cn_head_out *heads,
                 const cn_f32s_ctl *ctl, hipStream_t st);
