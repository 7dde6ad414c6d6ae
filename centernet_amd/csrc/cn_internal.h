// cn_internal.h -- prototypes of the functions one .hip file defines and another calls.  Included by both
// sides, so the defining file is compiled against the declaration its callers see.
#pragma once
#include "cn_common.h"

// ---- cn_stem.hip
int cn_stem_conv_f32(const float *x, const float *w_packed, const float *scale, const float *shift,
                     float *y, int B, int H, int W, int Ho, int Wo, int Cout, int KH, int KW,
                     int stride, int pad, int relu, int out_pitch, int KP, int persistent,
                     const cn_f32s_ctl *ctl, hipStream_t st);
int cn_stem_pool_rows(int B, int Ho, int Wo, int Cout, int KH, int KW, int stride, int KP);
int cn_stem_pool_f32s(const float *x, const float *w_packed, const float *scale, const float *shift,
                      float *y, int B, int H, int W, int Ho, int Wo, int Cout, int KH, int KW,
                      int stride, int pad, int relu, int out_pitch, int KP, int y_f32s, const cn_f32s_ctl *ctl,
                      hipStream_t st);

// ---- f32s deformable kernels: cn_dcn2.hip (window), cn_dcn3.hip (team), cn_dcn4.hip (wide); what they share is
// in cn_dcn_window.h.  One call description for all three (cn_conv.hip fills it once)
struct DcnWinCall {
    const float *x;            // (B, H, W, Cin) plain fp32
    const void *w;             // f32s-packed weights, row form + fragment copy
    const float *bias, *om;    // om: (B, H, W, om_pitch): 18 offsets + 9 masks per pixel
    int om_pitch;
    const float *scale, *shift;
    void *y;
    int out_pitch, out_plain;
    int B, Cin, H, W, Cout, mask_sigmoid, relu;
    float x_mul;               // f32s input exponent (a power of two)
    uint32_t *range;           // range words of the launch, or null
    int dbg;                   // cn_set_tuning key 9
    float *partial;            // K-split workspace, or null: no split
    size_t partial_bytes;
};
// each returns CN_ERR_UNSUPPORTED for a shape it does not take; *ksplit_out > 1: `partial` holds that many slabs
int cn_dcn_window_f32s(const DcnWinCall &c, int min_wgs, int *ksplit_out, hipStream_t st);
int cn_dcn_team_f32s(const DcnWinCall &c, int nmode, int *ksplit_out, hipStream_t st);
int cn_dcn_wide_f32s(const DcnWinCall &c, int nb, int *ksplit_out, hipStream_t st);

// ---- cn_dcn_general.hip
int cn_dcn_general_launch(const float *input, const float *weight, const float *bias,
                          const float *offset, const float *mask, float *output, int B, int Cin,
                          int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                          int dh, int dw, int dg, int mask_sigmoid, hipStream_t st);

// ---- cn_offconv.hip
bool cn_offconv_takes(int B, int H, int W, int Cin, int Cout, int in_pitch, int out_pitch, int ksplit);
int cn_offconv_f32s(const float *x, const void *w_packed, const float *scale, const float *shift, float *y,
                    int B, int H, int W, int Cin, int Cout, int out_pitch, int relu, const cn_f32s_ctl *ctl,
                    int ksplit, float *partial, hipStream_t st);

// ---- cn_proj.hip
bool cn_proj1x1_takes(int B, int H, int W, int Cin, int Cout, int stride, int in_pitch, int out_pitch);
int cn_proj1x1_f32s(const void *x, const void *w_packed, const float *scale, const float *shift, void *y, int B, int H,
                    int W, int Cin, int Cout, int stride, int in_pitch, int out_pitch, int relu, int out_plain,
                    const cn_f32s_ctl *ctl, hipStream_t st);

// ---- cn_conv16.hip
int cn_conv3x3_c16(const float *x, const float *w_packed, const float *scale, const float *shift,
                   float *y, int B, int H, int W, int Ho, int Wo, int Cin, int Cout, int stride,
                   int in_pitch, int out_pitch, int relu, hipStream_t st);
int cn_conv3x3_c16s(const float *x, const void *w_packed, const float *scale, const float *shift,
                    float *y, int B, int H, int W, int Ho, int Wo, int Cin, int Cout, int stride,
                    int in_pitch, int out_pitch, int relu, const cn_f32s_ctl *ctl, hipStream_t st);

// ---- cn_conv3x3.hip (LDS-halo kernel)
// bn_class: 2 = 128-wide N tiles, 1 = 64, 0 = 32 (chosen by the caller, same rule as cn_conv.hip);
// dtype: CN_DTYPE_*; flags: cn_conv_desc.flags (CN_CONV_X_PLAIN / Y_PLAIN / R_PLAIN)
int cn_conv3x3s1(const void *x, const void *w_packed, const float *scale, const float *shift,
                 const void *residual, void *y, int B, int H, int W, int Cin, int Cout,
                 int in_pitch, int out_pitch, int res_pitch, int relu, int vec_out, int bn_class,
                 int dtype, int flags, const cn_f32s_ctl *ctl, hipStream_t st);
int cn_deconv4x4s2_halo(const void *x, const void *w_packed, const float *scale, const float *shift,
                        void *y, int B, int H, int W, int Cin, int Cout, int in_pitch, int out_pitch,
                        int relu, int vec_out, int dtype, int flags, const cn_f32s_ctl *ctl,
                        hipStream_t st);

// ---- cn_conv3x3p.hip (persistent loader / consumer kernel)
bool cn_conv3x3p_takes(int B, int H, int W, int Cin, int Cout, int in_pitch, int out_pitch, int res_pitch,
                       bool in_plain, bool has_res);
int cn_conv3x3s1_persist(const void *x, const void *w_packed, const float *scale, const float *shift,
                         const void *residual, void *y, int B, int H, int W, int Cin, int Cout,
                         int in_pitch, int out_pitch, int res_pitch, int relu, int out_plain, int res_plain,
                         const cn_f32s_ctl *ctl, hipStream_t st);
bool cn_conv3x3s2p_takes(int B, int Hi, int Wi, int Cin, int Cout, int in_pitch, int out_pitch);
int cn_conv3x3s2_persist(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                         int B, int Hi, int Wi, int Cin, int Cout, int in_pitch, int out_pitch, int relu,
                         int out_plain, const cn_f32s_ctl *ctl, hipStream_t st);
bool cn_deconv4x4s2p_takes(int B, int H, int W, int Cin, int Cout, int in_pitch, int out_pitch, bool in_plain);
int cn_deconv4x4s2_persist(const void *x, const void *w_packed, const float *scale, const float *shift, void *y,
                           int B, int H, int W, int Cin, int Cout, int in_pitch, int out_pitch, int relu,
                           int out_plain, const cn_f32s_ctl *ctl, hipStream_t st);
bool cn_heads3x3p_takes(int B, int H, int W, int in_pitch, int head_conv, int n_heads, const cn_head_out *heads,
                        bool in_plain);
int cn_heads3x3p(const void *x, int B, int H, int W, int Cin, int in_pitch, const void *w1_packed,
                 const float *scale1, const float *bias1, int n_heads, const cn_head_out *heads,
                 const cn_f32s_ctl *ctl, hipStream_t st);
