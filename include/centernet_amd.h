/*
 * centernet_amd.h -- C ABI of libcenternet_amd.so (gfx950 / MI355X only).
 *
 * This is the drop-in boundary for the CenterNet inference hot path
 * (SURVEY.md section 8b).  Every entry point:
 *   - takes plain device pointers, sizes and a hipStream_t passed as void*;
 *   - never allocates, frees or synchronises: the caller owns every buffer,
 *     including the workspace, and the call is stream-ordered and asynchronous;
 *   - returns CN_OK (0) or a negative cn_status; nothing longjmps or prints
 *     (the reference raises THError, DCNv2/src/dcn_v2_cuda.c:33-38, and only
 *     printf()s launch errors, dcn_v2_im2col_cuda.cu:331-335);
 *   - is thread-safe per stream (no hidden global scratch, unlike the
 *     per-Function `ones`/`columns` buffers of DCNv2/dcn_v2_func.py:28).
 *
 * All tensors are fp32.  "NCHW" is the reference's layout; "NHWC" is the
 * native layout of this library (channel vectors contiguous so that the four
 * bilinear taps of the deformable gather are 128-byte coalesced reads).
 *
 * Citations are relative to /root/reference.
 */
#ifndef CENTERNET_AMD_H
#define CENTERNET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cn_status {
    CN_OK = 0,
    CN_ERR_SHAPE = -1,     /* shapes / kernel sizes do not match (THError in the reference) */
    CN_ERR_UNSUPPORTED = -2,
    CN_ERR_WORKSPACE = -3, /* workspace too small; query with the *_workspace_bytes call */
    CN_ERR_LAUNCH = -4,    /* hipGetLastError() != hipSuccess after a launch */
    CN_ERR_NULL = -5,
    CN_ERR_ALIGN = -6      /* a pointer is not 16-byte aligned */
} cn_status;

#define CN_LAYOUT_NCHW 0
#define CN_LAYOUT_NHWC 1

/* Element type of activations / packed weights.  fp32 is the parity path; fp16 (half activations and
 * weights, fp32 accumulate on v_mfma_f32_32x32x16_f16, fp32 epilogue) is a compute mode the reference
 * does not have: it runs Hourglass-104 (BASELINE configs[4]) and the ResNet nets (res_N, resdcn_N) --
 * every convolution form, the deformable convolution (gather forms), ConvTranspose 4x4/s2 and the
 * max-pool take it.  Offsets / masks of the deformable convolution, bias, scale and shift stay fp32. */
#define CN_DTYPE_F32 0
#define CN_DTYPE_F16 1
/* fp32 values stored as fp16 (high, low) pairs, 32-channel groups of 128 bytes; computed
 * with three fp16 MFMAs per product at fp32-level accuracy (csrc/cn_common.h) */
#define CN_DTYPE_F32S 2

/* f32s range control (csrc/cn_common.h "Range").  An f32s tensor holds  stored = real * 2^-e  with a
 * per-tensor exponent e owned by the caller (centernet_amd/engine.py picks it so that the tensor's
 * largest magnitude sits near 2^9; the fp16 pair then keeps its 22 bits over 12 binades below
 * and has 2^6 of head-room above).  The kernels never see e: its effect is folded by the caller
 * into the per-channel epilogue `scale` / `shift` they apply anyway, and into the two multipliers
 * below (powers of two, hence exact).  `range`, when not NULL, points to CN_RANGE_WORDS device
 * words the caller zeroed: the launch max-es into them, as float bit patterns, the largest
 * |value| it split -- side 0 = the output side (the stored tensor / the hidden tile of the fused
 * heads), side 1 = the input side (a plain x, the blended deformable samples); word
 * [(side * CN_RANGE_SLOTS + slot) * CN_RANGE_STRIDE], the maximum over the slots is the
 * launch's (cn_range_fold reduces them).  A maximum > 65504 means a
 * value was clamped: the result is invalid and the caller must re-scale (the reference's plain
 * fp32 never saturates; neither does this library silently).  NULL ctl = all defaults. */
#define CN_RANGE_SLOTS 64   /* words per side a launch spreads its per-wave maxima over ... */
#define CN_RANGE_STRIDE 16  /* ... one per 64-byte line (atomics on one address serialise) */
#define CN_RANGE_WORDS (2 * CN_RANGE_SLOTS * CN_RANGE_STRIDE)  /* words of one launch's `range` */
typedef struct cn_f32s_ctl {
    float x_mul;     /* plain fp32 x (CN_CONV_X_PLAIN, deformable input, stem image): multiplied by
                        this before it is split; 0 = 1 */
    float res_mul;   /* the residual is multiplied by this before it is added; 0 = 1 */
    uint32_t *range; /* device, CN_RANGE_WORDS words, or NULL */
} cn_f32s_ctl;

/* Library / ABI version (major*10000 + minor*100 + patch). */
int cn_version(void);
/* Human-readable text for a cn_status. */
const char *cn_status_string(int status);
/* Architecture the device code was compiled for ("gfx950"). */
const char *cn_arch(void);
/* Kernel-selection knobs for benchmarking (not needed for correctness).
 * THREADING: the knobs are plain process-global integers read by every launch.  cn_set_tuning is NOT
 * thread-safe against concurrent launches: the "thread-safe per stream" rule of the entry points holds only
 * while nobody calls cn_set_tuning.  Set knobs once, before the first launch (as bench.py --tune does), or
 * with all streams of the process idle; a value changed under a running launch list gives a mix of forms
 * (every form computes the same function, so results stay valid, timings do not).
 * cn_set_tuning answers CN_ERR_UNSUPPORTED for an unknown key or a value outside the key's set, and then
 * changes nothing.  (default) marks the value a key has at start and after cn_reset_tuning.
 * Dense implicit GEMM and dispatch (cn_conv.hip):
 * key 1: LDS tile buffers of the dense implicit-GEMM kernels, 0 = per-shape default (default), 1 or 2 = force.
 * key 2: 1 = never pick 64-wide N tiles for Cout > 64; 0 (default) = pick them when they avoid a
 *        half-empty 128-wide tile.
 * key 3: (retired) pixel tile of the deformable kernel; 0 and 64 are accepted and ignored, 64-pixel tiles
 *        are the only form built.  Reads back 0.
 * key 4: pixel tile of the dense kernels for Cout > 64, 0 = by grid size (default), 64 or 128 = force.
 * key 5: 1 = never split K (default 0).
 * key 6: 1 = run the 3-channel stem on the generic implicit-GEMM kernel instead of the LDS-window
 *        kernel (cn_stem.hip) (default 0).
 * key 7: XCD-aware tile order: 0 = deformable kernel only (default, +5-10 % there), 1 = also the dense
 *        implicit-GEMM kernels (no gain measured), 2 = nowhere.
 * key 8: s_setprio(1) around the MFMA clusters, 0 or 1 (default 1).
 * key 9: ablation and probe switches, a bit set, 0 ... 2047 (default 0): bit 0 / 1 = skip A / B staging
 *        (results are then wrong), the further bits are kernel-specific; bits 8 / 9 = instrumented
 *        instantiations of the team / wide deformable forms.
 * key 10: 1 = run 3x3 layers and ConvTranspose2d(4, 2, 1) on the generic implicit GEMM instead of the
 *         LDS-halo kernel (cn_conv3x3.hip) and the other specialised 3x3 kernels (default 0).
 * key 11: (retired) fp32 LDS-window deformable kernel, removed (20-30 % slower than the gather form);
 *         only 0 is accepted.  Reads back 0.
 * key 12: 0 = one-tile-per-workgroup stem kernel instead of the persistent, prefetching one
 *         (default 1; both in cn_stem.hip).
 * key 13: tap split of the gather-form deformable kernel, 0 = auto (default), 1 = never, 3 or 9 = force.
 * key 16: split-K: least K chunks per slice, 1 ... 64 (default 8).
 * key 17: split-K: most slices, 1 ... 64 (default 16).
 * key 22: gather-form deformable kernel: 1 = a tile is an 8-wide BLOCK of pixels (8 x 8 / 8 x 16) when the
 *         map divides into them (default: the nine taps of a block sample a compact neighbourhood that
 *         stays in L1 / L2), 0 = BM consecutive pixels of a row.
 * key 23: form of the f32s deformable kernel.  0 = by shape and grid (default), in the order of preference of
 *         dcn_route (csrc/cn_dcn.hip; cn_dcn_v2_route below says what a call gets).  1 = the global-gather
 *         form always.  For every shape the form takes, the gather form for the others (tests, A/B): 2 = the
 *         register-sampling form (cn_dcn2.hip: every lane samples its own MFMA operand from a window of the
 *         input in LDS), 4 / 5 = the team form in T / N mode, 6 / 7 = the wide form (a workgroup owns ALL
 *         output channels of its tile; 7 = four blocks per workgroup).  3 is refused (the wave-specialised
 *         window form it selected was removed).
 * key 27: 7x7 / stride 1 stem of <= 16 output channels with CN_CONV_STEM_F32S: 1 = f32s kernel
 *         (default), 0 = the fp32 16x16x4 kernel (then cn_stem_f32s_supported answers 0 for it).
 * LDS-halo kernel (cn_conv3x3.hip):
 * key 14: 64-wide layers as 256-pixel tiles: 1 = four waves, 2 / 3 = eight waves (f32s; one / three taps
 *         of weight prefetch); default 0 (measured, no gain).
 * key 15: fp32 / fp16 kernels: 0 = 4-wave instead of 8-wave workgroups for the 128-wide tiles
 *         (default 1: +1 %, measured).
 * key 18: phase shift of the workgroups that share a CU, in percent of one tile's MFMA time, 0 ... 255
 *         (default 100, 0 = off); applied to launches of >= 4 dispatch rounds.
 * key 19: 64-wide tiles at four workgroups per CU (single-buffered weight tile, <= 128 registers):
 *         0 = when that needs fewer dispatch rounds (default), 1 = always, 2 = never.
 * key 20: f32s, 128-wide tiles: 1 = per-tap weight tile in LDS (default), 0 = weights streamed into
 *         registers from the fragment-ordered copy (+5-20 % in a back-to-back micro-benchmark, no gain
 *         inside the network: measured).
 * key 21: f32s (A/B switches, 0 ... 7, default 0): bit 0 = 128-wide tiles as eight waves of 32 x 64 with
 *         weights three taps ahead instead of four waves of 64 x 64 two taps ahead (+1 % on resdcn_18
 *         without it); bit 1 = every 64-wide layer two taps ahead (default: one tap for two-chunk layers,
 *         three for longer K; measured); bit 2 = 8 x 16 pixel tiles on wide maps too (no difference,
 *         measured).
 * key 24: 1-D grid with the column blocks of a pixel tile dispatched together on one XCD (0 ... 3, default 1):
 *         bit 0 = for the fused heads, bit 1 = for plain layers of several Cout blocks; 0 = one grid row
 *         per head / block.
 * key 26: fused f32s heads with a hidden layer wider than 64: 1 = hidden layer kept in registers
 *         (default), 0 = staged through LDS; 2 = 128-wide slices (register-bound, A/B only),
 *         3 = the register form for 64-wide hidden layers too (slower there, A/B only).
 * Persistent loader / consumer 3x3 kernel for f32s tensors (cn_conv3x3p.hip):
 * key 28: 0 = off (the LDS-halo kernel takes its layers), 1 = on for the shapes it takes (default),
 *         2 ... 7 = also for launches of fewer than 256 work items.
 * key 29: start delay of the second resident workgroup, 0 ... 255 units of 256 cycles (default 0).
 * key 30: A/B switches, a bit set, 0 ... 255 (default 2): bit 0 = no s_setprio(1) around the consumers'
 *         MFMA block, bit 1 = the pipelined schedule, bit 2 = v_mfma_f32_32x32x16_f16 in the generic forms
 *         (3x3 / s1, stride 2, transposed) whose default is v_mfma_f32_16x16x32_f16 (the fused heads run
 *         32x32x16 whatever the bit says).
 * key 31: 1 = the fused heads with a 64-wide hidden layer run on it (default), 0 = on the LDS-halo kernel.
 * key 32: 1 = ConvTranspose2d(4, 2, 1) runs on it in parity form (default), 0 = on the LDS-halo kernel.
 * key 33: 1 = 3x3 / stride 2 / pad 1 runs on it in parity-plane form (default), 0 = on the implicit GEMM.
 * key 47: workgroups per XCD of one of its launches, at most, 1 ... 64 (default 64: two per CU).  For tests:
 *         with a smaller cap every workgroup walks several items at small shapes.
 * Team form of the f32s deformable kernel (cn_dcn3.hip):
 * key 36: when key 23 = 0: 0 = off, 1 = layers with <= 64 output channels, 2 = every layer it takes
 *         (T mode), 3 = every layer, N mode where Cout is a multiple of 128 and that still fills the
 *         chip (default).
 * key 37: K split until a launch has this many workgroups, 1 ... 4096 (default 512).
 * key 38: start delay of the second resident workgroup of every CU, 0 ... 1024 units of 256 cycles
 *         (default 32).
 * Offset / mask convolution of the deformable modules (cn_offconv.hip):
 * key 39: 1 = 3x3 layers of <= 32 output channels on a plain fp32 tensor run on it (default),
 *         0 = on the LDS-halo kernel.
 * key 40: workgroups from which its four-wave form is used, 0 ... 1000000 (default 768).
 * Wide form of the f32s deformable kernel (cn_dcn4.hip):
 * key 41: when key 23 = 0: 1 = layers with Cout % 128 == 0 take the wide form (default), 0 = the team form.
 * key 42: K split until a launch has this many workgroups, 1 ... 4096 (default 256).
 * key 45: 1 = L2 prefetch of the weight slabs three steps ahead (default), 0 = none.
 * Stem + max-pool kernel (cn_stem.hip), measurement only:
 * key 43: probe switches of its instrumented instantiation, 0 ... 31 (default 0).
 * key 44: start delay of the second resident workgroup, 0 ... 1024 units of 256 cycles (default 0).
 * 1x1 projections (cn_proj.hip):
 * key 46: 1 = f32s 1x1 layers without residual run on the direct-fragment kernel (default),
 *         0 = on the implicit GEMM. */
int cn_set_tuning(int key, int value);
/* Keys from 65 on.  (tests/test_tuning_host.py records the accepted set of keys -1 ... 64 and reads the comment
 * above against it, and holds 48 to be unknown: the numbers up to 64 are closed, new knobs count on from 65.)
 * 16-channel 3x3 kernel (cn_conv16.hip):
 * knob 65: 1 = fp16 3x3 / pad 1 layers of 16 input and <= 32 output channels without residual run on its half
 *          form (default; cn_conv16_f16_supported says which), 0 = on the LDS-halo kernel (stride 1) or the
 *          implicit GEMM (stride 2).  Key 10 = 1 (everything on the implicit GEMM) switches it off as well, as it
 *          does the fp32 / f32s forms of that file. */
/* Current value of a knob into *value; CN_ERR_UNSUPPORTED for a key cn_set_tuning does not know. */
int cn_get_tuning(int key, int *value);
/* Every knob back to its default. */
int cn_reset_tuning(void);



/* ------------------------------------------------------------------------
 * Deformable convolution v2, forward.
 *
 * Replaces: void dcn_v2_cuda_forward(THCudaTensor *input, *weight, *bias,
 *   *ones, *offset, *mask, *output, *columns, int kernel_h, int kernel_w,
 *   stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
 *   deformable_group)          -- DCNv2/src/dcn_v2_cuda.h:9-17,
 *                                 impl DCNv2/src/dcn_v2_cuda.c:10-102,
 *                                 called from DCNv2/dcn_v2_func.py:29-37.
 * Differences at the boundary: no `ones`/`columns` scratch (the column buffer
 * is never materialised; bias is an epilogue), the batch is one launch (no
 * per-sample host loop, dcn_v2_cuda.c:61), errors are return codes.
 *
 *   y[b,o,h,w] = bias[o] + sum_{c,k} W[o,c,k] * m[b,k,h,w] *
 *                bilinear(x[b,c], h*s-p+i*d+dy[b,k,h,w], w*s-p+j*d+dx[b,k,h,w])
 * with the reference's sampling-window rule (dcn_v2_im2col_cuda.cu:165) and
 * per-corner zeroing (:30-41).  offset channel 2k = dy, 2k+1 = dx of tap k.
 *
 * layout = CN_LAYOUT_NCHW: input (B,Cin,H,W), offset (B,dg*2*kh*kw,Ho,Wo),
 *   mask (B,dg*kh*kw,Ho,Wo), output (B,Cout,Ho,Wo) -- exactly the reference.
 * layout = CN_LAYOUT_NHWC: input (B,H,W,Cin), offset_mask (B,Ho,Wo,om_pitch)
 *   holding [2*kh*kw offsets | kh*kw mask] per pixel (mask pointer ignored,
 *   om_pitch >= 3*kh*kw given through cn_dcn_v2_forward_nhwc_f32 below).
 *
 * weight is always the reference's (Cout,Cin,kh,kw) tensor here; use
 * cn_pack_conv_weight_f32 + the *_packed entry points to skip the repack.
 * Domain: the reference operator's -- any kernel size, stride, padding, dilation,
 * deformable_group (Cin % deformable_group == 0) and channel count.  The configuration
 * CenterNet instantiates (3x3, stride 1, pad 1, dilation 1, one group, Cin % 4 == 0:
 * resnet_dcn.py:221-223, pose_dla_dcn.py:352) runs on the NHWC MFMA kernel and needs
 * cn_dcn_v2_forward_workspace_bytes() of 16-byte aligned scratch (layout change + tap
 * split); every other configuration (e.g. DCNv2/test.py:16-19 inC = 2, :169-179
 * deformable_groups = 2) runs on the general-domain NCHW kernel (cn_dcn_general.hip),
 * which takes no workspace (NULL / 0 accepted).  Invalid geometry -> CN_ERR_SHAPE.
 * ------------------------------------------------------------------------ */
size_t cn_dcn_v2_forward_workspace_bytes(int B, int Cin, int H, int W, int Cout,
                                         int kernel_h, int kernel_w, int layout);

int cn_dcn_v2_forward_f32(const float *input, const float *weight, const float *bias,
                          const float *offset, const float *mask, float *output,
                          int B, int Cin, int H, int W, int Cout,
                          int kernel_h, int kernel_w, int stride_h, int stride_w,
                          int pad_h, int pad_w, int dilation_h, int dilation_w,
                          int deformable_group, int apply_mask_sigmoid,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Native form used by the network plan: NHWC activations, packed weight
 * ([tap][Cout_pad][Cin], see cn_pack_conv_weight_f32), offsets and mask logits
 * interleaved per pixel as produced by the conv_offset_mask convolution
 * (DCNv2/dcn_v2.py:64-68: channels 0..17 offsets, 18..26 mask logits; the
 * sigmoid of :67 is applied inside when mask_sigmoid != 0), and a fused
 * epilogue  y = relu?( (acc + bias) * scale + shift )  that folds the
 * BatchNorm + ReLU following every DCN in resnet_dcn.py:237-239 /
 * pose_dla_dcn.py:345-357.  scale/shift may be NULL (identity).
 * workspace: small maps split the nine taps over 3 or 9 workgroups per output tile (fp32
 * partial sums, deterministic reduce + epilogue in a second launch) so that the
 * latency-bound gather still fills the 256 CUs; that needs
 * cn_dcn_v2_forward_nhwc_workspace_bytes() of 16-byte aligned scratch.  With a NULL or
 * too small workspace the layer runs unsplit (same result up to fp32 summation order).
 */
size_t cn_dcn_v2_forward_nhwc_workspace_bytes(int B, int Cin, int H, int W, int Cout);
/* dtype-generic form: the input stays a PLAIN fp32 NHWC tensor in the fp32 and f32s modes (one 16-byte
 * gather per bilinear corner); dtype = CN_DTYPE_F32S takes an f32s-packed weight, contracts on the
 * fp16 matrix instruction (the blended sample is split as it enters the LDS A tile) and writes
 * y as f32s (pitch % 32 == 0) or, with CN_CONV_Y_PLAIN, as plain fp32.
 * dtype = CN_DTYPE_F16 is refused here (CN_ERR_UNSUPPORTED, as it always was: these pointers address
 * floats): half tensors go through cn_dcn_v2_forward_nhwc_f16 / cn_dcn_v2_route_f16 below. */
int cn_dcn_v2_forward_nhwc(const float *input_nhwc, const void *weight_packed, const float *bias,
                           const float *offset_mask_nhwc, int om_pitch, const float *scale,
                           const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                           int H, int W, int Cout, int mask_sigmoid, int relu, int dtype, int flags,
                           const cn_f32s_ctl *ctl, void *workspace, size_t workspace_bytes,
                           void *stream);
int cn_dcn_v2_forward_nhwc_f32(const float *input_nhwc, const float *weight_packed,
                               const float *bias, const float *offset_mask_nhwc,
                               int om_pitch, const float *scale, const float *shift,
                               float *output_nhwc, int B, int Cin, int H, int W,
                               int Cout, int mask_sigmoid, int relu, void *workspace,
                               size_t workspace_bytes, void *stream);
/* Which kernel form and K split a cn_dcn_v2_forward_nhwc call with these arguments gets under the current
 * tuning keys.  Host only: launches nothing, tests the pointers for null and alignment and never follows them
 * (stream is ignored).  Returns what the call would return from its argument checks; *info is written only
 * with CN_OK. */
#define CN_DCN_GATHER 0      /* global gather on the implicit GEMM */
#define CN_DCN_GATHER_PAD 1  /* ... for Cin % 32 != 0 (CN_DTYPE_F16: Cin % 64 != 0) */
#define CN_DCN_WINDOW 2      /* f32s LDS-window forms: register sampling (cn_dcn2.hip) */
#define CN_DCN_TEAM_T 3      /* team form (cn_dcn3.hip), the teams split the K steps of a 64-channel block */
#define CN_DCN_TEAM_N 4      /* ... the teams split a 128-channel block */
#define CN_DCN_WIDE4 5       /* wide form (cn_dcn4.hip), four 32-channel blocks per workgroup */
#define CN_DCN_WIDE8 6       /* ... eight */
/* the form of CN_DTYPE_F16 calls only, numbered behind the forms above */
#define CN_DCNH_WINDOW 7     /* fp16 LDS-window form: register sampling of halves (cn_dcn_h.hip) */
#define CN_DCN_FLAG_PREFETCH 1  /* wide: L2 prefetch of the weights */
#define CN_DCN_FLAG_STAGGER 2   /* team: the second occupant of a CU starts late */
#define CN_DCN_FLAG_TILE2D 4    /* gather: tiles are pixel blocks */
#define CN_DCN_FLAG_VEC_OUT 8   /* gather: 16-byte stores to y */
typedef struct cn_dcn_route_info {
    int form;            /* CN_DCN_* */
    int grid_x, grid_y;  /* pixel tiles, blocks of output channels */
    int ksplit;          /* 1, or the slabs of partial sums in the workspace that a reduce launch sums */
    int flags;           /* CN_DCN_FLAG_* */
} cn_dcn_route_info;
int cn_dcn_v2_route(const float *input_nhwc, const void *weight_packed, const float *bias,
                    const float *offset_mask_nhwc, int om_pitch, const float *scale,
                    const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                    int H, int W, int Cout, int mask_sigmoid, int relu, int dtype, int flags,
                    const cn_f32s_ctl *ctl, void *workspace, size_t workspace_bytes,
                    void *stream, cn_dcn_route_info *info);

/* fp16 compute mode of the deformable convolution: input_nhwc is a HALF NHWC tensor (B, H, W, Cin) with
 * Cin % 8 == 0 (a bilinear corner is a 16-byte gather of 8 halves, else CN_ERR_UNSUPPORTED), the weight is
 * cn_pack_conv_weight(..., CN_DTYPE_F16)'s (64-channel K chunks), y a half NHWC tensor at out_pitch.
 * offset_mask_nhwc (pitch >= 27, real units), bias, scale and shift stay fp32; mask_sigmoid, relu, the
 * epilogue order, the alignment checks and the workspace (cn_dcn_v2_forward_nhwc_workspace_bytes: fp32 slabs of
 * the gather form's tap split) are those of cn_dcn_v2_forward_nhwc.  The four corners are read as halves,
 * blended and multiplied by the mask in fp32, rounded ONCE to fp16 into the matrix operand, accumulated in
 * fp32; the epilogue is fp32 with one rounding at the store.  cn_dcn_v2_route_f16 is the host query of the
 * same call (forms CN_DCN_GATHER, CN_DCN_GATHER_PAD, CN_DCNH_WINDOW). */
int cn_dcn_v2_forward_nhwc_f16(const void *input_nhwc, const void *weight_packed, const float *bias,
                               const float *offset_mask_nhwc, int om_pitch, const float *scale,
                               const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                               int H, int W, int Cout, int mask_sigmoid, int relu, void *workspace,
                               size_t workspace_bytes, void *stream);
int cn_dcn_v2_route_f16(const void *input_nhwc, const void *weight_packed, const float *bias,
                        const float *offset_mask_nhwc, int om_pitch, const float *scale,
                        const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                        int H, int W, int Cout, int mask_sigmoid, int relu, void *workspace,
                        size_t workspace_bytes, void *stream, cn_dcn_route_info *info);

/* Plain fp32 NHWC <-> f32s NHWC (CN_DTYPE_F32S: fp16 high / low pairs in 128-byte groups of 32
 * channels).  Pitches in channels; f32s pitches are multiples of 32; channels of the last
 * group beyond C are written as zeros.  New surface (the reference has one tensor format). */
int cn_f32_to_f32s(const float *x, void *y, size_t npix, int C, int in_pitch, int out_pitch,
                   void *stream);
int cn_f32s_to_f32(const void *x, float *y, size_t npix, int C, int in_pitch, int out_pitch,
                   void *stream);
/* the same with the tensor's exponent: y = split(x * mul) (side 1 of `range`, CN_RANGE_WORDS words, receives max |x * mul|) and
 * y = join(x) * mul; mul is a power of two (0 = 1), range may be NULL */
int cn_f32_to_f32s_scaled(const float *x, void *y, size_t npix, int C, int in_pitch, int out_pitch,
                          float mul, uint32_t *range, void *stream);
int cn_f32s_to_f32_scaled(const void *x, float *y, size_t npix, int C, int in_pitch, int out_pitch,
                          float mul, void *stream);
/* max |x| over the C channels of npix pixels of a plain fp32 NHWC tensor, max-ed into *word as a
 * float bit pattern (the caller zeroes it): the calibration pass of the f32s exponents */
int cn_absmax_f32(const float *x, size_t npix, int C, int pitch, uint32_t *word, void *stream);
/* end-of-forward bookkeeping of the range words of n_launches launches (cur: n_launches x
 * CN_RANGE_WORDS; hi, lo: n_launches x 2 sides): m = max over the slots, hi = max(hi, m),
 * lo = min(lo, m) over the non-zero m, slots = 0 -- the host reads hi / lo whenever it synchronises anyway (largest
 * and smallest per-forward maximum since its last look) instead of after every forward */
int cn_range_fold(uint32_t *cur, uint32_t *hi, uint32_t *lo, int n_launches, void *stream);
/* The same, plus a sticky two-word digest for a cheap host check: summary[0] = max over all
 * (launch, side) values seen so far (float bits; > 65504 or NaN bits = something was clamped),
 * summary[1] = the smallest NON-ZERO per-forward maximum so far (initialise to 0x7f800000).  The
 * host reads 8 bytes per forward and walks the hi / lo tables only when the digest is out of bounds. */
int cn_range_fold_digest(uint32_t *cur, uint32_t *hi, uint32_t *lo, uint32_t *summary,
                         int n_launches, void *stream);

/* Flip-test averaging (detectors/ctdet.py:34-37, detectors/multi_pose.py:44-55, models/utils.py:28-50).
 * x_pair (2, C, H, W): image 1 is the horizontally mirrored frame; out (1, C, H, W) =
 * (f(x0[c, y, x]) + sign[c] * f(x1[src[c], y, W-1-x])) / 2.  chan_src (C) = left / right joint permutation
 * (flip_lr / flip_lr_off), NULL = identity; chan_sign (C), NULL = +1 (-1 on the x components of joint
 * offsets); apply_sigmoid: f = logistic, written back to x_pair in place (the reference's sigmoid_()),
 * chan_src must then be a permutation. */
int cn_flip_average_f32(float *x_pair, float *out, int C, int H, int W, const int32_t *chan_src,
                        const float *chan_sign, int apply_sigmoid, void *stream);
/* The same for P pairs at once (flip-test of a batch).  x_pairs (2P, C, H, W) = [f0, f0 mirrored, f1, f1
 * mirrored, ...], the layout of cn_warp_normalize_u8_f32_batch(..., flip_concat = 1); out (P, C, H, W).
 * mode 0: the average above, pair p bit-identical to cn_flip_average_f32 on that pair (which is the
 * P = 1 call of this one); mode 1: out[p] = image 0 of pair p (reg / hp_offset, which the reference takes
 * from the un-mirrored frame only), chan_src, chan_sign and apply_sigmoid unused. */
int cn_flip_average_f32_batch(float *x_pairs, float *out, int P, int C, int H, int W, const int32_t *chan_src,
                              const float *chan_sign, int apply_sigmoid, int mode, void *stream);
/* Box calibration (bench.py `box_calibration`; measurement aid, not on the product path; no
 * reference counterpart).  cn_calib_mfma_f16: a register-only v_mfma_f32_32x32x16_f16 loop on
 * every SIMD (1024 workgroups x 4 waves, `iters` x 16 instructions per wave); returns the FLOPs
 * of the launch (0 on error) -- the caller times it with HIP events.  cn_calib_copy: a float4
 * grid-stride copy of `bytes` (multiple of 16) from src to dst. */
double cn_calib_mfma_f16(float *sink, int iters, void *stream);
int cn_calib_copy(const void *src, void *dst, size_t bytes, void *stream);
/* cn_calib_mfma_shape (tools/bench_mfma_shape.py): the bare f32s step of the persistent 3x3 kernel -- a
 * wave tile of 64 pixels x 32 channels, K 32 per step as three fp16 products per tile -- as
 * v_mfma_f32_32x32x16_f16 (shape = 32: two tiles, 12 instructions per step) or v_mfma_f32_16x16x32_f16
 * (shape = 16: eight tiles, 24 instructions), 256 workgroups x 8 waves = two waves per SIMD.  operands:
 * CN_CALIB_SHAPE_OPERAND_BYTES of fp16 values the caller chooses (wave w: 12 fragments of 64 lanes x 16
 * bytes at 12288 w).  from_lds != 0: every step reads its 12 fragments from LDS again (ds_read_b128);
 * 0: once, in front of the loop.  stamps: NULL, or 2 x 256 words that receive per workgroup the shader
 * cycles and the 100 MHz ticks of its loop (a build of its own: without stamps no clock is read).
 * Returns the FLOPs of the launch (0 on error). */
#define CN_CALIB_SHAPE_OPERAND_BYTES 98304
double cn_calib_mfma_shape(const void *operands, float *sink, unsigned long long *stamps, int shape,
                           int from_lds, int iters, void *stream);
/* cn_calib_latency: ONE lane walks `steps` dependent loads through `chain` (chain[i] = index of the
 * next element; the caller lays the walk out: a buffer beyond the caches for the HBM latency, a small
 * one for L2), then `steps` dependent device-scope atomic additions on *atom.  out[0], out[1]: ticks of
 * the constant 100 MHz clock each chain took; out[2]: sink. */
int cn_calib_latency(const uint32_t *chain, uint32_t start, int steps, uint32_t *atom,
                     unsigned long long *out, void *stream);
/* cn_calib_clock: one lane counts shader-core cycles over `ticks` ticks of the constant 100 MHz clock:
 * out[0] = core cycles, out[1] = ticks -- the core clock at the moment the launch runs (enqueue it right
 * behind the work whose clock is asked for). */
int cn_calib_clock(unsigned long long *out, int ticks, void *stream);

/* ------------------------------------------------------------------------
 * Dense convolution as an implicit GEMM on fp32 MFMA (no im2col buffer).
 *
 * Replaces the torch.nn.Conv2d / BatchNorm2d(eval) / ReLU / residual-add call
 * sites of the backbones (resnet_dcn.py:38-67,138-142,155-177;
 * msra_resnet.py; pose_dla_dcn.py:147-221; large_hourglass.py:17-74) and, with
 * the output-scatter arguments, the four parity classes of
 * ConvTranspose2d(k=4,s=2,p=1) (resnet_dcn.py:228-235).
 *
 *   y = relu?( conv(x, w) * scale + shift + residual? )
 *
 * x: NHWC with pixel pitch in_pitch floats (>= Cin; lets a layer read a channel
 * slice of a wider tensor), or NCHW3 for the stem (in_layout = NCHW, Cin = 3).
 * w: packed by cn_pack_conv_weight_f32.  y: NHWC (pitch out_pitch) or NCHW.
 * Output pixel (oy,ox) of the conv grid (Ho,Wo) is written to
 * (oy*oy_mul+oy_add, ox*ox_mul+ox_add) of a (B,OH,OW) map.
 * ------------------------------------------------------------------------ */
typedef struct cn_conv_desc {
    int B, H, W, Cin;       /* input */
    int Ho, Wo, Cout;       /* conv output grid */
    int KH, KW;
    int stride, pad_h, pad_w, dil;
    int in_layout, in_pitch; /* pitch in floats per pixel (NHWC) */
    int out_layout, out_pitch;
    int OH, OW, oy_mul, oy_add, ox_mul, ox_add;
    int relu;
    int dtype;              /* CN_DTYPE_F32 / CN_DTYPE_F16 / CN_DTYPE_F32S (x, w, residual, NHWC y) */
    int flags;              /* CN_CONV_* bits, 0 by default */
    int res_pitch;          /* pixel pitch of the residual in floats; 0 = out_pitch.  A pitch that differs
                               from out_pitch (y or the residual is a channel slice of a wider tensor, e.g. a
                               concatenation buffer: pose_dla_dcn.py:157-165) is taken by the 3x3 / stride 1
                               / pad 1 layers only: ask cn_conv2d_res_pitch_supported() */
    cn_f32s_ctl ctl;        /* dtype = CN_DTYPE_F32S (and the CN_CONV_STEM_F32S stem): range control */
} cn_conv_desc;
/* 1 when cn_conv2d honours d->res_pitch != d->out_pitch for this descriptor (host-only) */
int cn_conv2d_res_pitch_supported(const cn_conv_desc *d);
/* dtype = CN_DTYPE_F32S: x (and the residual) / y are plain fp32 NHWC tensors; the kernel
 * converts while staging / storing (e.g. the offset maps the deformable kernel reads).
 * dtype = CN_DTYPE_F16 takes CN_CONV_Y_PLAIN alone: y is a plain fp32 NHWC tensor (out_pitch in floats,
 * the epilogue stores fp32 without rounding to half) -- the offset / mask convolution of a half plan.
 * x, w and the residual stay halves. */
#define CN_CONV_X_PLAIN 1
#define CN_CONV_Y_PLAIN 2
#define CN_CONV_R_PLAIN 4
/* dtype = CN_DTYPE_F32, 3-channel NCHW stem only: compute with three fp16 MFMAs per product
 * (the image and the packed weight stay fp32 and are split inside the kernel) */
#define CN_CONV_STEM_F32S 8
/* with CN_CONV_STEM_F32S: the MaxPool2d(kernel 3, stride 2, padding 1) that follows the stem in the
 * ResNet backbones (resnet_dcn.py:138-141, msra_resnet.py:116-119) is applied inside the kernel;
 * Ho / Wo stay the convolution's output size, y is the pooled (B, Ho/2, Wo/2, out_pitch) tensor.
 * Only for shapes cn_stem_maxpool_supported() accepts, CN_ERR_UNSUPPORTED otherwise. */
#define CN_CONV_STEM_MAXPOOL 16
/* with CN_CONV_STEM_MAXPOOL: y (the pooled map) is written as an f32s tensor (out_pitch % 32 == 0,
 * 128-byte aligned) holding y * 2^-e -- the exponent folded into scale / shift by the caller -- and
 * side 0 of ctl.range receives max |y|: the consumers of the ResNet stem are f32s layers */
#define CN_CONV_STEM_Y_F32S 32

/* 1 when cn_conv2d accepts CN_CONV_STEM_MAXPOOL for this stem descriptor (7x7 / stride 2, 33..64
 * output channels, rows of 1..4 whole 128-pixel tiles, even Ho, batch * Ho large enough to fill
 * the chip with row strips), else 0.  Host-only, no GPU needed. */
int cn_stem_maxpool_supported(const cn_conv_desc *d);
/* 1 when cn_conv2d runs this stem descriptor with CN_CONV_STEM_F32S arithmetic (only then are
 * ctl.x_mul / ctl.range used: the fp32 stem kernels split nothing), else 0.  Host-only. */
int cn_stem_f32s_supported(const cn_conv_desc *d);
/* 1 when cn_conv2d runs this descriptor, without residual and unsplit, on the half form of the 16-channel 3x3
 * kernel (cn_conv16.hip) under the current tuning: dtype CN_DTYPE_F16, Cin = 16, Cout <= 32, 3x3 / pad 1 /
 * stride 1 or 2, half output (no CN_CONV_Y_PLAIN), Wo % 128 == 0, in_pitch % 8 == 0, out_pitch % 4 == 0, knob 65 on
 * and key 10 off; else 0.  Host-only. */
int cn_conv16_f16_supported(const cn_conv_desc *d);

/* Number of floats of the packed weight for (Cout,Cin,KH,KW). */
size_t cn_packed_conv_weight_floats(int Cout, int Cin, int KH, int KW);
/* (Cout,Cin,KH,KW) fp32 device tensor -> packed [KH*KW][Cout_pad32][Cin_pad] */
int cn_pack_conv_weight_f32(const float *w_oihw, float *w_packed, int Cout, int Cin,
                            int KH, int KW, void *stream);

int cn_conv2d_f32(const cn_conv_desc *desc, const float *x, const float *w_packed,
                  const float *scale, const float *shift, const float *residual,
                  float *y, void *stream);
/* dtype-generic forms (desc->dtype selects fp32 / fp16; NCHW head outputs and the stem's
 * NCHW image are always fp32; scale/shift are always fp32).
 * CN_DTYPE_F32S: 3x3 and (round 6) 1x1 kernels carry a second, fragment-ordered copy of the matrix behind
 * the row-ordered one ([tap][chunk][32-channel block][quarter][lane] x 16 bytes: what a lane of the
 * 32x32x16 MFMA holds, one contiguous 1 KiB per wave-load); cn_packed_conv_weight_elems counts both. */
size_t cn_packed_conv_weight_elems(int Cout, int Cin, int KH, int KW, int dtype);
int cn_pack_conv_weight(const float *w_oihw, void *w_packed, int Cout, int Cin, int KH, int KW,
                        int dtype, void *stream);
/* workspace: optional scratch for split-K (layers whose plain grid would leave most of the
 * 256 CUs idle: small maps with deep K); query with cn_conv2d_workspace_bytes, NULL/0 = never
 * split.  The split is deterministic (fixed partition, second-stage reduce, no atomics). */
size_t cn_conv2d_workspace_bytes(const cn_conv_desc *desc);
int cn_conv2d(const cn_conv_desc *desc, const void *x, const void *w_packed, const float *scale,
              const float *shift, const void *residual, void *y, void *workspace,
              size_t workspace_bytes, void *stream);
/* The output scatter must fit the map: oy_mul, ox_mul >= 1, oy_add, ox_add >= 0, (Ho-1)*oy_mul + oy_add < OH and
 * (Wo-1)*ox_mul + ox_add < OW, CN_ERR_SHAPE otherwise (nothing is launched; the queries answer 0).  A call whose
 * scatter is not the identity onto a (B, Ho, Wo) map runs on the implicit GEMM and is never K-split. */

/* Which kernel a cn_conv2d call runs and in which form: the arguments of cn_conv2d, the status cn_conv2d's host
 * checks would return (CN_ERR_UNSUPPORTED where no kernel takes the call), and *info.  Host-only: of the pointers
 * only null-ness and alignment count, none is dereferenced, nothing is launched.  The answer depends on the
 * cn_set_tuning keys as the call does.  On a status other than CN_OK *info is zero except route. */
#define CN_ROUTE_NONE 0
#define CN_ROUTE_STEM_POOL 1  /* stem + max-pool (CN_CONV_STEM_MAXPOOL) */
#define CN_ROUTE_STEM 2       /* LDS-window / persistent stem kernels; variant: CN_STEM_* */
#define CN_ROUTE_CONV16 3     /* 16-channel 3x3, fp32 */
#define CN_ROUTE_CONV16S 4    /* ... f32s arithmetic on plain tensors */
#define CN_ROUTE_CONV16H 5    /* ... half tensors */
#define CN_ROUTE_OFFCONV 6    /* offset / mask convolution; variant: teams per workgroup (1 or 2) */
#define CN_ROUTE_HALO 7       /* 3x3 / stride 1: variant CN_C3_PERSIST, or CN_C3_TILE with the CN_C3_* bits */
#define CN_ROUTE_S2P 8        /* persistent 3x3 / stride 2 */
#define CN_ROUTE_PROJ 9       /* 1x1 projection */
#define CN_ROUTE_IGEMM 10     /* implicit GEMM: m_tile pixels x n_tile channels, ksplit K slices */
/* variant of CN_ROUTE_STEM (0 on every other route but those named above) */
#define CN_STEM_NONE 0
#define CN_STEM_WINDOW 1
#define CN_STEM_PERSIST 2
#define CN_STEM_PERSIST_F32S 3
#define CN_STEM_16S 4
/* variant of CN_ROUTE_HALO: the persistent loader / consumer kernel, or the LDS-halo tile kernel with its form:
 * m_tile pixels (128 or 256) in rows of 16 or 32, n_tile channels, 4 or 8 waves */
#define CN_C3_PERSIST 1
#define CN_C3_TILE 2
#define CN_C3_TW32 0x10       /* tile rows of 32 pixels (else 16) */
#define CN_C3_WAVES8 0x20     /* eight waves per workgroup (else four) */
#define CN_C3_OCC4 0x40       /* the four-workgroups-per-CU form */
#define CN_C3_KSKIP 0x80      /* fp32: the empty K groups of the last chunk are skipped */
#define CN_C3_WREG 0x100      /* f32s: weights streamed into registers, no LDS weight tile */
#define CN_C3_PREFETCH(v) (((v) >> 12) & 3)   /* f32s, LDS weight tile: taps of weight prefetch (1..3) */
#define CN_C3_HREG 0x200      /* cn_heads3x3_1x1_route, f32s: the hidden layer stays in registers (4 x 1 waves), not in LDS (2 x 2) */
typedef struct cn_conv_route_info {
    int route;            /* CN_ROUTE_* */
    int n_tile, m_tile;   /* channels / pixels per workgroup tile: CN_ROUTE_HALO tile kernel and CN_ROUTE_IGEMM, else 0 */
    int ksplit;           /* K slices the call runs with (1: no split) */
    int want;             /* ... and those the layer wants: cn_conv2d_workspace_bytes = want * B*Ho*Wo * cout_pad32 * 4, 0 for want 1 */
    int variant;
    int grid_x, grid_y;   /* workgroups of the launch: CN_ROUTE_STEM, CN_ROUTE_OFFCONV, CN_ROUTE_HALO tile kernel; else 0 */
} cn_conv_route_info;
int cn_conv2d_route(const cn_conv_desc *d, const void *x, const void *w_packed, const float *scale,
                    const float *shift, const void *residual, void *y, void *workspace,
                    size_t workspace_bytes, void *stream, cn_conv_route_info *info);

/* ------------------------------------------------------------------------
 * ConvTranspose2d(kernel 4, stride 2, padding 1, bias=False) + BN(eval) + ReLU.
 * Replaces the up-sampling layers of resnet_dcn.py:228-235 / msra_resnet.py
 * (_make_deconv_layer).  Executed as the four output-parity 2x2 convolutions in
 * ONE launch.  w_iohw is torch's (Cin,Cout,4,4) ConvTranspose2d weight.
 * x (B,H,W,in_pitch) NHWC -> y (B,2H,2W,out_pitch) NHWC.
 * ------------------------------------------------------------------------ */
size_t cn_packed_deconv4x4s2_weight_floats(int Cin, int Cout);
/* dtype-generic forms (CN_DTYPE_F32 / CN_DTYPE_F32S; `flags`: CN_CONV_X_PLAIN / CN_CONV_Y_PLAIN).
 * CN_DTYPE_F16: half NHWC in and out (Cin % 8 == 0, in_pitch % 8 == 0, flags 0), fp32 scale / shift; the
 * packed weight is [parity 4][tap 4][Cout_pad32][Cin_pad64] halves and fits a buffer of
 * cn_packed_deconv4x4s2_weight_floats() floats like every other dtype's. */
int cn_pack_deconv4x4s2_weight(const float *w_iohw, void *w_packed, int Cin, int Cout, int dtype,
                               void *stream);
int cn_conv_transpose4x4s2(const void *x_nhwc, const void *w_packed, const float *scale,
                           const float *shift, void *y_nhwc, int B, int H, int W, int Cin, int Cout,
                           int in_pitch, int out_pitch, int relu, int dtype, int flags,
                           const cn_f32s_ctl *ctl, void *stream);
/* Which kernel a cn_conv_transpose4x4s2 call runs: its arguments, its status, and *info as cn_conv2d_route fills it.
 * CN_ROUTE_HALO with variant CN_C3_PERSIST or CN_C3_TILE | bits (n_tile 64 / 128, grid), or CN_ROUTE_IGEMM (the
 * implicit GEMM in parity form: Cout <= 32, an out_pitch that is no multiple of 4 or a y off 16 bytes, key 10) with
 * m_tile and n_tile.  ksplit = want = 1.  Host-only: no pointer is dereferenced, nothing is launched. */
int cn_conv_transpose4x4s2_route(const void *x_nhwc, const void *w_packed, const float *scale,
                                 const float *shift, void *y_nhwc, int B, int H, int W, int Cin, int Cout,
                                 int in_pitch, int out_pitch, int relu, int dtype, int flags,
                                 const cn_f32s_ctl *ctl, void *stream, cn_conv_route_info *info);
int cn_pack_deconv4x4s2_weight_f32(const float *w_iohw, float *w_packed, int Cin, int Cout,
                                   void *stream);
int cn_conv_transpose4x4s2_f32(const float *x_nhwc, const float *w_packed, const float *scale,
                               const float *shift, float *y_nhwc, int B, int H, int W, int Cin,
                               int Cout, int in_pitch, int out_pitch, int relu, void *stream);

/* 3x3 / stride-2 / pad-1 max pooling, NHWC (resnet_dcn.py:142). */
int cn_maxpool3x3s2_nhwc_f32(const float *x, float *y, int B, int H, int W, int C,
                             void *stream);
/* generic k x k / stride s max pooling NHWC (pose_dla_dcn.py:200 uses 2x2 s2) */
int cn_maxpool_nhwc_f32(const float *x, float *y, int B, int H, int W, int C, int k,
                        int s, int pad, void *stream);
/* the same with an f32s input tensor (in_dtype = CN_DTYPE_F32S, C % 32 == 0; CN_DTYPE_F32: as
 * above); the output is plain fp32 */
int cn_maxpool_nhwc(const void *x_nhwc, float *y_nhwc, int B, int H, int W, int C, int k, int s,
                    int pad, int in_dtype, void *stream);
/* f32s input of exponent e: out_mul = 2^e brings the pooled values back to real units */
int cn_maxpool_nhwc_scaled(const void *x_nhwc, float *y_nhwc, int B, int H, int W, int C, int k,
                           int s, int pad, int in_dtype, float out_mul, void *stream);
/* f32s in (pixel pitch in_pitch), f32s out (pixel pitch out_pitch -- y may be a channel slice of a wider
 * tensor, e.g. the concatenation buffer of pose_dla_dcn.py:157-165): y = split(max(window) * mul), mul a
 * power of two (the ratio of the two tensors' exponents); range (CN_RANGE_WORDS words, may be NULL)
 * side 0 receives max |y| */
int cn_maxpool_nhwc_f32s(const void *x, void *y, int B, int H, int W, int C, int in_pitch, int out_pitch,
                         int k, int s, int pad, float mul, uint32_t *range, void *stream);

/* half NHWC in (pixel pitch in_pitch), half NHWC out (pixel pitch out_pitch): general k / s / pad with -inf
 * padding as above; C, in_pitch and out_pitch multiples of 8 (16 bytes of halves per lane) */
int cn_maxpool_nhwc_f16(const void *x, void *y, int B, int H, int W, int C, int in_pitch, int out_pitch,
                        int k, int s, int pad, void *stream);

/* Depthwise ConvTranspose2d(C, C, kernel 2f, stride f, padding f/2, groups=C, bias=False)
 * -- the up-sampling of IDAUp (pose_dla_dcn.py:370-373) -- fused with the element-wise
 * add that follows it (IDAUp.forward, :385-386: node(layers[i] + layers[i-1])).
 * x (B,H,W,C) NHWC; w_taps [(2f)*(2f)][C] (tap-major: w_taps[ky*2f+kx][c] = w[c,0,ky,kx]);
 * add (B,fH,fW,C) or NULL; y (B,fH,fW,C). */
int cn_dw_conv_transpose_f32(const float *x, const float *w_taps, const float *add, float *y,
                             int B, int H, int W, int C, int f, void *stream);
/* Channel-slice copy between NHWC tensors of different pitch (torch.cat(.., 1) of
 * Root.forward, pose_dla_dcn.py:159). */
int cn_copy_channels_f32(const float *src, int src_pitch, float *dst, int dst_pitch,
                         size_t npix, int C, void *stream);
/* Half forms of the two: x / add / y (src / dst) address halves, 8 channels (16 bytes) per lane.
 * cn_dw_conv_transpose_f16: w_taps stays fp32 as above; halves are widened, the <= 4 products and `add` are
 * summed in fp32 and rounded to fp16 once at the store; C % 8 == 0, CN_ERR_UNSUPPORTED otherwise.
 * cn_copy_channels_f16: C, src_pitch and dst_pitch multiples of 8 and both pointers 16-byte aligned. */
int cn_dw_conv_transpose_f16(const void *x, const float *w_taps, const void *add, void *y,
                             int B, int H, int W, int C, int f, void *stream);
int cn_copy_channels_f16(const void *src, int src_pitch, void *dst, int dst_pitch,
                         size_t npix, int C, void *stream);
/* Canvas masks (--keep_res batches of mixed input sizes): image b of a batch owns the rectangle
 * rects_dev[b] of a common canvas, given in network-input pixels, half-open; a tensor at 1 / 2^shift of the
 * input keeps [y0 >> shift, y1 >> shift) x [x0 >> shift, x1 >> shift) of image b (clipped to H x W) and
 * everything else of its H x W is overwritten: with zero bytes in the NHWC form -- zero in plain fp32 and
 * in f32s alike -- and with `fill` in the NCHW form.  Store-only launches, one workgroup per (8 rows, image) -- rows of C x H in the NCHW form.
 * A rectangle that covers the tensor writes nothing; an empty or inverted one clears the image.  The
 * rectangles live in DEVICE memory (they travel with the batch's descriptors and survive a graph capture).
 * cn_mask_rects_f32: channels [c_off, c_off + C) of a (B, H, W, pitch) tensor of 4-byte elements, taken in
 * whole 32-channel groups (C is rounded up to the next group, cut at the pitch: a tensor narrower than a
 * group is cleared in whole pixels); pitch, c_off and the cleared width multiples of 4 and the first cleared
 * element 16-byte aligned, CN_ERR_ALIGN otherwise.  CN_ERR_NULL for a null tensor or table, CN_ERR_SHAPE for
 * sizes <= 0, c_off + C > pitch, B > 65535 or a shift outside 0 .. 30. */
typedef struct cn_rect { int32_t x0, y0, x1, y1; } cn_rect;
int cn_mask_rects_f32(void *t_nhwc, int B, int H, int W, int pitch, int c_off, int C,
                      const cn_rect *rects_dev, int shift, void *stream);
int cn_mask_rects_nchw_f32(float *t, int B, int C, int H, int W, const cn_rect *rects_dev,
                           int shift, float fill, void *stream);
/* cn_mask_rects_f16: the same rectangle rule on a (B, H, W, pitch) tensor of 2-byte elements (halves; +0.0 is
 * written); pitch, c_off and C count halves.  Channels [c_off, c_off + C) are taken in whole 8-CHANNEL groups
 * (16 bytes; C is rounded up to the next group, cut at the pitch) -- not the 32-channel groups of the fp32
 * entry: a half plan concatenates in place with members of 16 and 32 channels side by side in one buffer, and
 * a wider rounding would clear the neighbouring member.  pitch, c_off and the cleared width multiples of 8 and
 * the first cleared element 16-byte aligned, CN_ERR_ALIGN otherwise; CN_ERR_NULL / CN_ERR_SHAPE as above. */
int cn_mask_rects_f16(void *t_nhwc, int B, int H, int W, int pitch, int c_off, int C,
                      const cn_rect *rects_dev, int shift, void *stream);
/* cn_dcn_v2_forward_nhwc_f16 on a canvas batch: the same arguments, checks, route and forms, plus the batch's
 * rectangle table and the level of the tensor (rect_shift 0 .. 30, CN_ERR_SHAPE otherwise).  Image b's sampling
 * positions are formed relative to its rectangle's origin (rects_dev[b].x0 >> rect_shift, .y0 >> rect_shift,
 * clipped to the tensor) and moved back by whole pixels, so the bilinear fractions -- and every rounding behind
 * them -- are those of the image's own forward wherever its rectangle lies on the canvas.  What lies outside
 * the rectangle must be zero (cn_mask_rects_f16): it stands in for the samples the image's own forward drops.
 * A null table is cn_dcn_v2_forward_nhwc_f16, bit for bit. */
int cn_dcn_v2_forward_nhwc_f16_rects(const void *input_nhwc, const void *weight_packed, const float *bias,
                                     const float *offset_mask_nhwc, int om_pitch, const float *scale,
                                     const float *shift, void *output_nhwc, int out_pitch, int B, int Cin,
                                     int H, int W, int Cout, int mask_sigmoid, int relu, void *workspace,
                                     size_t workspace_bytes, const cn_rect *rects_dev, int rect_shift,
                                     void *stream);
/* Nearest x2 up-sampling + add of the skip branch (large_hourglass.py:102-109, 163-174). */
int cn_upsample2x_add_f32(const float *x, const float *add, float *y, int B, int H, int W,
                          int C, void *stream);
int cn_upsample2x_add_f16(const void *x, const void *add, void *y, int B, int H, int W, int C,
                          void *stream);

/* Fused detection heads.  The reference builds every head as
 *   nn.Sequential(Conv2d(F, head_conv, 3, padding=1, bias=True), ReLU, Conv2d(head_conv, C, 1))
 * (resnet_dcn.py:155-177, msra_resnet.py) and runs them one after the other on the same
 * feature map.  Here all heads are ONE launch: w1_packed is cn_pack_conv_weight_f32 of the
 * first convolutions concatenated along Cout, (n_heads*head_conv, F, 3, 3); bias1 the
 * concatenated biases; the hidden activations stay in LDS and each head's 1x1 convolution
 * runs as a second matrix-core GEMM in the same workgroup, writing the NCHW maps
 * (B, cout, H, W) that cn_ctdet_decode_f32 / cn_multi_pose_decode_f32 consume.
 * x is NHWC with row pitch in_pitch.  Built for n_heads <= 8 and head_conv = 64 (resnet_dcn.py),
 * or 128 / 192 / 256 (pose_dla_dcn.py:456-468, large_hourglass.py) with every cout <= 96: the
 * hidden layer is then processed in 64-channel slices whose 1x1 products accumulate in registers.
 * Anything else returns CN_ERR_UNSUPPORTED (the caller then issues cn_conv2d per convolution). */
typedef struct cn_head_out {
    const float *w;    /* (cout, head_conv) row-major == Conv2d(head_conv, cout, 1).weight */
    const float *bias; /* (cout) or NULL */
    float *y;          /* (B, cout, H, W) */
    int cout;
    int reserved;
    const float *oscale; /* (cout) or NULL: y = acc * oscale + bias -- undoes a per-row pre-scale of w
                            and the exponent of the hidden tile (f32s; see cn_f32s_ctl) */
    const void *w_frag;  /* optional (f32s, head_conv = 64, cout <= 96): the same matrix w as (high, low)
                            fp16 fragments, cn_pack_head_w2_f32s -- with it the heads run on the
                            persistent kernel (cn_conv3x3p.hip); NULL = the one-tile-per-workgroup kernel */
} cn_head_out;
/* w (cout, 64) row-major -> out (cn_packed_head_w2_bytes(cout) bytes, 16-byte aligned) */
size_t cn_packed_head_w2_bytes(int cout);
int cn_pack_head_w2_f32s(const float *w, void *out, int cout, void *stream);
int cn_heads3x3_1x1_f32(const float *x, int B, int H, int W, int Cin, int in_pitch,
                        const float *w1_packed, const float *bias1, int head_conv, int n_heads,
                        const cn_head_out *heads, void *stream);
/* dtype-generic form.  CN_DTYPE_F32S: x is an f32s tensor (or plain fp32 with CN_CONV_X_PLAIN),
 * w1_packed an f32s-packed weight whose per-row prescale factors come in scale1 (NULL = 1);
 * the hidden tile and the 1x1 weights are split inside the kernel; outputs are fp32 NCHW. */
int cn_heads3x3_1x1(const void *x, int B, int H, int W, int Cin, int in_pitch,
                    const void *w1_packed, const float *scale1, const float *bias1, int head_conv,
                    int n_heads, const cn_head_out *heads, int dtype, int flags,
                    const cn_f32s_ctl *ctl, void *stream);
/* Which kernel a cn_heads3x3_1x1 call runs: its arguments, its status, and *info as cn_conv2d_route fills it.
 * Always CN_ROUTE_HALO: variant CN_C3_PERSIST, or CN_C3_TILE | bits (CN_C3_HREG: the register form) with n_tile the
 * width of a hidden slice (64 or 128), m_tile 128 and the grid that is launched -- grid_y == 1 with more than one
 * head where cn_set_tuning key 24 folded the heads into grid_x.  ksplit = want = 1.  Host-only: heads[] is read as
 * the call's checks read it, of every pointer only null-ness and alignment count, nothing is launched. */
int cn_heads3x3_1x1_route(const void *x, int B, int H, int W, int Cin, int in_pitch,
                          const void *w1_packed, const float *scale1, const float *bias1, int head_conv,
                          int n_heads, const cn_head_out *heads, int dtype, int flags,
                          const cn_f32s_ctl *ctl, void *stream, cn_conv_route_info *info);

/* ------------------------------------------------------------------------
 * Pre-process on the device: BaseDetector.pre_process
 * (src/lib/detectors/base_detector.py:37-65) = cv2.resize (scale != 1) +
 * cv2.warpAffine(INTER_LINEAR, zero border) + (x/255 - mean)/std + HWC->CHW (+ flip concat).
 *
 * cn_warp_normalize_u8_f32: image (H, W, 3) uint8 on the device (row pitch in bytes),
 *   dst_to_src_2x3 = six HOST doubles: trans_input inverted the way cv::warpAffine inverts its M
 *   (centernet_amd/image.py invert_affine), out = (1 + flip_concat, 3, out_h, out_w) fp32 NCHW
 *   with out[1] = out[0] flipped along x (base_detector.py:59-60).  mean3 / std3: HOST floats.
 * cn_resize_bilinear_u8: cv2.resize(image, (out_w, out_h)), uint8 HWC -> dense uint8 HWC.
 * Arithmetic: OpenCV's uint8 INTER_LINEAR path -- fixed point, not float bilinear: warpAffine
 * samples at 1/32-pixel positions (AB_BITS = 10, INTER_BITS = 5) with 15-bit weights
 * (INTER_REMAP_COEF_BITS) and round-half-up, zero border; resize is separable with 11-bit
 * coefficients and its own uint8 vertical pass, a copy at equal size and the 2 x 2 mean at
 * exactly half size.  The published algorithm is restated with its constants in
 * oracle/pre_oracle.py (OpenCV is a third-party dependency that is absent here); these entry
 * points equal that restatement bit for bit.  Normalisation: float64, rounded once to fp32.
 * ------------------------------------------------------------------------ */
int cn_warp_normalize_u8_f32(const uint8_t *image_hwc, int H, int W, int pitch_bytes,
                             const double *dst_to_src_2x3, int out_h, int out_w,
                             const float *mean3, const float *std3, int flip_concat,
                             float *out_nchw, void *stream);
/* the same for N images of one geometry in ONE launch (frames of a video, a batch from the loader):
 * images image_stride_bytes apart, outputs dense (N, 3 | 6, out_h, out_w) */
int cn_warp_normalize_u8_f32_batch(const uint8_t *images_hwc, int N, size_t image_stride_bytes, int H, int W,
                                   int pitch_bytes, const double *dst_to_src_2x3, int out_h, int out_w,
                                   const float *mean3, const float *std3, int flip_concat,
                                   float *out_nchw, void *stream);
/* Mixed-size batches (a dataset, not a video): N images of their own sizes packed into ONE uint8 buffer,
 * one descriptor per image in DEVICE memory (it travels with the images on the caller's copy stream; N
 * matrices do not fit a kernel argument).  The layout is fixed, 8-byte aligned, 88 bytes. */
typedef struct cn_image_desc {
    uint64_t offset;       /* bytes from the start of the packed buffer to the image; any value, no alignment */
    int32_t H, W, pitch;   /* rows, columns, row pitch in bytes (>= 3 * W) */
    int32_t reserved;      /* 0 */
    double dst_to_src[6];  /* cn_warp_normalize_u8_f32_ragged: dst_to_src_2x3 of this image */
    double scale_x, scale_y;   /* cn_resize_bilinear_u8_ragged, the OUTPUT's descriptor: 1. / ((double)out_w /
                                  (double)in_w) and the same for y, formed on the host as cv::resize forms them */
} cn_image_desc;
/* cn_warp_normalize_u8_f32_ragged: cn_warp_normalize_u8_f32 of image n of `packed` as descs_dev[n] describes
 * it, n < N, in ONE launch; output dense (N, 3 | 6, out_h, out_w), the layout of the batch entry.  The same
 * arithmetic, bit for bit.  mean3 / std3: HOST floats.  H, W, pitch and offset are only known on the device:
 * the caller validates them before the upload (H, W in 1..32767, pitch >= 3 * W, the image inside the
 * buffer); an image with H <= 0 or W <= 0 is skipped.
 * cn_resize_bilinear_u8_ragged: cn_resize_bilinear_u8 of N images in one launch, image n from in_descs_dev[n]
 * of packed_in to out_descs_dev[n] of packed_out (H, W = the output size; pitch normally 3 * W); per image the
 * copy at equal size, the 2 x 2 mean at exactly half size, the separable 11-bit form otherwise, with the
 * output descriptor's scale_x / scale_y.  max_out_h / max_out_w: the largest output of the batch (the grid). */
int cn_warp_normalize_u8_f32_ragged(const uint8_t *packed, const cn_image_desc *descs_dev, int N, int out_h,
                                    int out_w, const float *mean3, const float *std3, int flip_concat,
                                    float *out_nchw, void *stream);
int cn_resize_bilinear_u8_ragged(const uint8_t *packed_in, const cn_image_desc *in_descs_dev, uint8_t *packed_out,
                                 const cn_image_desc *out_descs_dev, int N, int max_out_h, int max_out_w,
                                 void *stream);
/* The pre-process of a tile pyramid (run_tiles with levels; image.tile_box_normalize is its host restatement):
 * tile n is a (out_h, out_w) window at origin (y0, x0) of LEVEL `level` of its frame, the frame box-filtered by
 * f = 1 << level, computed straight from the frame -- no level image is stored, and the rounding happens once:
 *   v[c] = (sum over dy, dx in [0, f) of src[(y0 + y) * f + dy, (x0 + x) * f + dx, c] + (f * f >> 1)) >> (2 * level)
 *   out[n, c, y, x] = float32(((double)v[c] / 255.0 - mean[c]) / std[c])
 * Source positions outside [0, H) x [0, W) contribute 0 and the divisor stays f * f (a zero border, as the
 * warp's).  Level 0 is the pixel itself: cn_warp_normalize_u8_f32_ragged at the tile's translation, bit for bit;
 * level 1 on an even-sized frame: cn_resize_bilinear_u8 at exactly half size, then that warp, bit for bit.
 * One descriptor per tile in DEVICE memory, 32 bytes, 8-byte aligned.  output dense (N, 3, out_h, out_w).
 * mean3 / std3: HOST floats.  The descriptors are only known on the device: the caller validates them before
 * the upload (H, W in 1..32767, pitch >= 3 * W, level in 0..3, y0 / x0 in -32768..32767, the frame inside the
 * buffer; any offset and pitch, no alignment needed); a tile with H <= 0, W <= 0 or a level outside 0..3 is
 * skipped, its output untouched.  CN_ERR_NULL / CN_ERR_SHAPE as cn_warp_normalize_u8_f32_ragged returns them. */
typedef struct cn_tile_box_desc {
    uint64_t offset;       /* bytes from the start of the packed buffer to the tile's frame */
    int32_t H, W, pitch;   /* the frame: rows, columns, row pitch in bytes (>= 3 * W) */
    int32_t level;         /* 0..3: the frame box-filtered by 1 << level */
    int32_t y0, x0;        /* the tile's origin in level pixels */
} cn_tile_box_desc;
int cn_tile_box_normalize_u8_f32(const uint8_t *packed, const cn_tile_box_desc *descs_dev, int N, int out_h,
                                 int out_w, const float *mean3, const float *std3, float *out_nchw, void *stream);
/* ctdet_post_process + the per-class split (utils/post_process.py:83-100, utils/image.py:19-24,63-66,
 * detectors/ctdet.py:47-56) on the device.  dets (B, K, 6) raw detections in output-grid units (K <= 128);
 * to_source_2x3: the float64 inverse map of get_affine_transform(c, s, 0, out_size, inv=1) -- one for
 * all images (per_image = 0) or B of them on the device (per_image = 1; device pointer either way);
 * rows (B, K, 5): [x1, y1, x2, y2, score] in source pixels / scale, grouped by class, inside a class
 * in their original order; bounds (B, num_classes + 1): class j of image b = rows[b, bounds[b, j] :
 * bounds[b, j + 1]] (rows with a class outside [0, num_classes) lie behind bounds[b, num_classes]).
 * Bit-identical to the reference's float64 affine + float32 rounding. */
int cn_ctdet_post_process_f32(const float *dets, int B, int K, int num_classes, const double *to_source_2x3,
                              int per_image, float scale, float *rows, int32_t *bounds, void *stream);
/* The ctdet scale merge (CtdetDetector.merge_outputs, detectors/ctdet.py:58-73) on the device, bit for bit.
 * rows (S, B, K, 5) / bounds (S, B, num_classes + 1): cn_ctdet_post_process_f32's output of test scale s in
 * slice s.  Per image: per class the rows of all scales in scale order; when S > 1 or apply_nms, Gaussian
 * soft-NMS of every class (sigma 0.5, threshold 0.001, the arithmetic of cn_soft_nms_f32, the whole in-place
 * array kept as the reference keeps it); then, when the image has more than max_per_image rows, the rows
 * whose score is >= the max_per_image-th largest score (ties kept), in order.  out_rows (B, S*K, 5) /
 * out_bounds (B, num_classes + 1): the tail's format.  Row cap: S*K <= CN_MERGE_MAX_ROWS and num_classes
 * <= CN_MERGE_MAX_CLASSES, CN_ERR_SHAPE above (one workgroup holds an image's rows in LDS). */
#define CN_MERGE_MAX_ROWS 2048
#define CN_MERGE_MAX_CLASSES 1024
int cn_ctdet_merge_f32(const float *rows, const int32_t *bounds, int S, int B, int K, int num_classes,
                       int apply_nms, int max_per_image, float *out_rows, int32_t *out_bounds, void *stream);
/* The tile merge of run_tiles (post_process.ctdet_tiles_results on the device, bit for bit): the ctdet merge with
 * the T overlapping tiles of a frame in the place of test scales, for frames with more rows than one workgroup
 * holds.  rows (B*T, K, 5) / bounds (B*T, num_classes + 1): cn_ctdet_post_process_f32's output of tile t of
 * frame b in image b*T + t, rows in FRAME pixels.  cores_dev (T, 4) float32 on the device: [x_lo, y_lo, x_hi,
 * y_hi] of tile t's core with the margin applied, -inf / +inf at the frame's edges.  Per frame:
 *   a row of tile t survives when its centre cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f (float32) has
 *   x_lo <= cx < x_hi and y_lo <= cy < y_hi; per class the survivors of all tiles in tile order, each tile's
 *   rows in their order; when T > 1 or apply_nms, Gaussian soft-NMS of every class as cn_ctdet_merge_f32 runs
 *   it (the whole in-place array kept); then, when the frame has more than max_per_frame rows, the rows whose
 *   score is >= the max_per_frame-th largest score (duplicates counted, ties kept), in order.
 * out_rows (B, T*K, 5) / out_bounds (B, num_classes + 1): the format of cn_ctdet_merge_f32.  status (B) int32.
 * Three launches at most (group, soft-NMS per (frame, class), cut), no host synchronisation, no floating-point
 * atomics: the result is a function of the input.  The class-grouped rows lie in the workspace between the
 * launches (cn_ctdet_tiles_merge_workspace_bytes; 16-byte aligned, CN_ERR_ALIGN otherwise; CN_ERR_NULL without
 * one, CN_ERR_WORKSPACE for a short one).  Limits: K <= 128, T*K <= CN_TILES_MAX_ROWS, num_classes <=
 * CN_MERGE_MAX_CLASSES, CN_ERR_SHAPE above.  What bounds a frame is one class: a frame in which a class segment
 * has more than CN_MERGE_MAX_ROWS survivors (the LDS of one soft-NMS) is not merged -- status[b] != 0, its
 * bounds all zero, its rows undefined; every other frame has status[b] == 0 and its result (the convention of
 * cn_exdet_merge_f32). */
#define CN_TILES_MAX_ROWS 65536
size_t cn_ctdet_tiles_merge_workspace_bytes(int B, int T, int K, int num_classes);
int cn_ctdet_tiles_merge_f32(const float *rows, const int32_t *bounds, int B, int T, int K, int num_classes,
                             const float *cores_dev, int apply_nms, int max_per_frame, float *out_rows,
                             int32_t *out_bounds, int32_t *status, void *workspace, size_t workspace_bytes,
                             void *stream);
/* The merge of a tile pyramid (post_process.ctdet_pyramid_results on the device, bit for bit):
 * cn_ctdet_tiles_merge_f32 with a size gate per tile.  gates_dev (T, 2) float32 on the device: [lo, hi) of tile
 * t in frame pixels (tiles.pyramid_grid: one band per pyramid level, -inf / +inf at the ends).  With w = x2 - x1
 * and h = y2 - y1 in float32, a row with a NaN in w or h is dropped; otherwise s = max(w, h), and the row
 * survives when lo <= s < hi AND its centre lies in the tile's core.  Everything else -- the three launches, the
 * workspace (cn_ctdet_tiles_merge_gated_workspace_bytes, the same size), the limits, status and the return
 * codes -- is cn_ctdet_tiles_merge_f32's; CN_ERR_NULL without a gate table.  With every gate (-inf, +inf) and no
 * NaN size the result is cn_ctdet_tiles_merge_f32's. */
size_t cn_ctdet_tiles_merge_gated_workspace_bytes(int B, int T, int K, int num_classes);
int cn_ctdet_tiles_merge_gated_f32(const float *rows, const int32_t *bounds, int B, int T, int K, int num_classes,
                                   const float *cores_dev, const float *gates_dev, int apply_nms,
                                   int max_per_frame, float *out_rows, int32_t *out_bounds, int32_t *status,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* exdet task, the device tail of its frame pipe (detectors/exdet.py:51-81; reference exdet.py:86-123).
 * cn_exdet_post_process_f32: ExdetDetector.post_process, the `score > 0` filter and the per-class selection of
 * merge_outputs for one test scale of a batch.  dets (B, R, 14): the raw rows of cn_exct_decode_f32 /
 * cn_agnex_ct_decode_f32 [x1, y1, x2, y2, score, 8 extreme-point coordinates, class] of every FRAME -- R = 2000
 * with flip-test (the frame's 1000 rows, then its mirror image's: the reshape(2, -1, 14) of the reference),
 * 1000 without; R even, R <= CN_MERGE_MAX_ROWS, num_classes <= CN_MERGE_MAX_CLASSES, CN_ERR_SHAPE otherwise.
 * Per frame: the second half of the rows gets x1' = out_width - x2, x2' = out_width - x1 in float32 (without
 * flip-test too, as the reference does); both corners go through to_source_2x3 (float32 point -> float64
 * (t0*x + t1*y) + t2 -> float32; to_source_2x3 / per_image as for cn_ctdet_post_process_f32), then / scale
 * (> 0) in float32.  rows (B, R, 5): [x1, y1, x2, y2, score] of the rows with score > 0 whose class column
 * equals an integer in [0, num_classes) -- NaN scores and every other class value drop out -- grouped by
 * class, inside a class in input order (a stable sort: soft-NMS depends on the order); rows behind the last
 * bound are zero.  bounds (B, num_classes + 1) as for ctdet.  Bit-identical to the host tail.
 * cn_exdet_merge_f32: the rest of merge_outputs.  rows (S, B, R, 5) / bounds (S, B, num_classes + 1): the
 * entry above, test scale s in slice s.  Per frame: per class the rows of all scales in scale order, Gaussian
 * soft-NMS of every class ALWAYS (sigma 0.5, threshold 0.001; the task has no --nms condition; the whole
 * in-place array kept, as cn_ctdet_merge_f32 keeps it), then the max_per_image cut with ties kept.
 * out_rows (B, min(S*R, CN_MERGE_MAX_ROWS), 5) / out_bounds (B, num_classes + 1).  The row cap holds for the
 * rows that are present, S*R may be anything: a frame with more than CN_MERGE_MAX_ROWS rows over all scales
 * is not merged -- status[b] != 0, its bounds all zero, its rows undefined; every other frame has status[b]
 * == 0 and its result.  status (B) int32. */
int cn_exdet_post_process_f32(const float *dets, int B, int R, int num_classes, int out_width,
                              const double *to_source_2x3, int per_image, float scale, float *rows,
                              int32_t *bounds, void *stream);
int cn_exdet_merge_f32(const float *rows, const int32_t *bounds, int S, int B, int R, int num_classes,
                       int max_per_image, float *out_rows, int32_t *out_bounds, int32_t *status, void *stream);
/* multi_pose_post_process + the "/ scale" of MultiPoseDetector.post_process (utils/post_process.py:103-114,
 * detectors/multi_pose.py:62-72) on the device.  dets (B, K, 40): multi_pose_decode rows [x1, y1, x2, y2,
 * score, 17 x (x, y), class] in output-grid units (K <= 128, CN_ERR_UNSUPPORTED above); to_source_2x3,
 * per_image and scale (> 0) as for cn_ctdet_post_process_f32.  rows (B, K, 39): the two box corners and the
 * 17 joints through the inverse map (float32 point -> float64 (t0*x + t1*y) + t2 -> float32, then / scale in
 * float32), the score copied, the class dropped, the row order kept.  Bit-identical to the host tail. */
int cn_multi_pose_post_process_f32(const float *dets, int B, int K, const double *to_source_2x3, int per_image,
                                   float scale, float *rows, void *stream);
/* The multi_pose scale merge (MultiPoseDetector.merge_outputs, detectors/multi_pose.py:74-81) on the device,
 * bit for bit.  rows (S, B, K, 39): cn_multi_pose_post_process_f32's output of test scale s in slice s.
 * out_rows (B, S*K, 39): per image the rows of all scales in scale order (row s*K + k); when S > 1 or
 * apply_nms, after Gaussian soft-NMS (sigma 0.5, threshold 0.001) with the arithmetic and the row moves of
 * cn_soft_nms_f32 at stride 39 -- the argmax swap exchanges whole rows, a discarded row takes columns 0..4 of
 * the last live row and exchanges columns 5.. with it.  The WHOLE in-place array is returned, rows past the
 * kept count included, and there is no top-100 cut (the reference has none for this task).
 * Row cap: S*K <= CN_MERGE_MAX_ROWS, CN_ERR_SHAPE above. */
int cn_multi_pose_merge_f32(const float *rows, int S, int B, int K, int apply_nms, float *out_rows,
                            void *stream);
/* The tile merge of multi_pose run_tiles (post_process.multi_pose_tiles_results on the device, bit for bit).
 * rows (B*T, K, 39): cn_multi_pose_post_process_f32's output of tile t of frame b in image b*T + t, rows in FRAME
 * pixels.  cores_dev (T, 4) float32 on the device, as for cn_ctdet_tiles_merge_f32.  Per frame:
 *   a row of tile t survives when its box centre cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f (float32) has
 *   x_lo <= cx < x_hi and y_lo <= cy < y_hi and, unless min_score is NaN, score >= min_score (a NaN score fails);
 *   the survivors of all tiles in tile order, each tile's rows in their order; when T > 1 or apply_nms, Gaussian
 *   soft-NMS (sigma 0.5, threshold 0.001) with the arithmetic and the row moves of cn_soft_nms_f32 at stride 39,
 *   as cn_multi_pose_merge_f32 runs it -- the WHOLE in-place array is kept, rows past the kept count included
 *   (they can pass the cut: MultiPoseDetector.merge_outputs keeps them too, and one tile per frame thereby
 *   equals run_frames); then, when more than max_per_frame rows are left, the rows whose score is >= the
 *   max_per_frame-th largest score (duplicates counted, ties kept), in order.
 * out_rows (B, T*K, 39): the first out_counts[b] rows of frame b are its result, the rest is not written.
 * out_counts (B), status (B): int32.  ONE launch, one workgroup of sixteen waves per frame that shares the argmax
 * and the decay of every soft-NMS step when the frame has more than CN_POSE_TILES_ONE_WAVE_ROWS survivors (up to
 * there one wave runs the same steps without barriers, which is faster: profiles/run_tiles_pose.txt); no host
 * synchronisation, no floating-point atomics: the result is a function of the input.  The survivors live in dynamic LDS: per row 4 x 4 bytes of box, 4 of score, 4 of
 * decayed score, 2 of source row index, 2 of start-of-step position and one discard bit = 28.125 bytes,
 * CN_POSE_TILES_MAX_ROWS x 28.125 = 144000 bytes next to 9.6 KB of select histogram and reduction words, of the
 * 160 KB of a gfx950 workgroup.  A frame with more survivors is not merged: status[b] = 1, out_counts[b] = 0;
 * every other frame has status[b] = 0 and its result.  The workspace is unused by this form (16 bytes are
 * asked for) and checked as the ctdet entry checks it: CN_ERR_NULL without one, CN_ERR_WORKSPACE for a short
 * one, CN_ERR_ALIGN off 16 bytes.  Limits: K <= 128, T >= 1, T*K <= CN_TILES_MAX_ROWS, CN_ERR_SHAPE otherwise.  A
 * refused call launches nothing. */
#define CN_POSE_TILES_MAX_ROWS 5120
#define CN_POSE_TILES_ONE_WAVE_ROWS 256
size_t cn_multi_pose_tiles_merge_workspace_bytes(int B, int T, int K);
int cn_multi_pose_tiles_merge_f32(const float *rows, int B, int T, int K, const float *cores_dev, int apply_nms,
                                  int max_per_frame, float min_score, float *out_rows, int32_t *out_counts,
                                  int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int cn_resize_bilinear_u8(const uint8_t *image_hwc, int H, int W, int pitch_bytes, int out_h,
                          int out_w, uint8_t *out_hwc, void *stream);

/* ddd task (detectors/ddd.py:30-54, 75-88).
 * cn_warp_table_u8_f32_batch: cn_warp_normalize_u8_f32_batch's sampler (same fixed-point warpAffine, zero
 * border, dst_to_src_2x3 host doubles) with the normalisation taken from a DEVICE table of 3 x 256 floats,
 * out[n, c, y, x] = table[c][v]: the ddd class normalises with a float32 chain, (u8 / 255 - mean) / std,
 * and the caller builds the table with exactly those operations.  N frames of one geometry in one launch,
 * output dense (N, 3, out_h, out_w); no flip form (the task has no flip test). */
int cn_warp_table_u8_f32_batch(const uint8_t *images_hwc, int N, size_t image_stride_bytes, int H, int W,
                               int pitch_bytes, const double *dst_to_src_2x3, int out_h, int out_w,
                               const float *table_3x256, float *out_nchw, void *stream);
/* cn_warp_table_u8_f32_ragged: the same for N images of their own sizes in ONE launch, as
 * cn_warp_normalize_u8_f32_ragged takes them: image n at packed + descs_dev[n].offset with that descriptor's
 * H, W, pitch and dst_to_src (DEVICE memory; the caller validates them before the upload), an image with
 * H <= 0 or W <= 0 skipped (its output slice is not written).  cn_warp_table_u8_f32_batch's arithmetic and
 * table read, bit for bit; output dense (N, 3, out_h, out_w); no flip form. */
int cn_warp_table_u8_f32_ragged(const uint8_t *packed, const cn_image_desc *descs_dev, int N, int out_h,
                                int out_w, const float *table_3x256, float *out_nchw, void *stream);
/* ddd_post_process_2d + ddd_post_process_3d + DddDetector.merge_outputs (utils/post_process.py:24-79,
 * utils/ddd_utils.py:68-114, detectors/ddd.py:82-88) for a batch.  dets (B, K, row_floats): the raw rows of
 * cn_ddd_decode_f32 with wh, row_floats = 18 (16, the form without wh, -> CN_ERR_UNSUPPORTED: the
 * reference's 3-D stage cannot process it either; K <= 128, CN_ERR_UNSUPPORTED above).  to_source_2x3 /
 * per_image as for cn_ctdet_post_process_f32; calibs (B, 3, 4) float32 on the device, image b is lifted with
 * matrix b.  rows (B, K, 13): [alpha, x1, y1, x2, y2, h, w, l, x, y, z, rotation_y, score], grouped by
 * class, inside a class in their original order; bounds (B, num_classes + 1) as for ctdet (a class is a
 * float equal to an integer in [0, num_classes); other rows lie behind the last bound); kept (B,
 * num_classes): the number of leading rows of each class with score > peak_thresh -- the rows of a class
 * arrive in descending score order, so merge_outputs' cut is that prefix.
 * Arithmetic: the reference's types statement by statement (float64 point map for the centre and for the
 * (w, h) pair, translation included; float32 unproject, box and angle sums; no FMA contraction) and columns
 * 1..10 and 12 equal the host tail bit for bit.  The two arctan2 (get_alpha, the viewing ray of
 * alpha2rot_y) are float64 atan2 rounded once to float32: NumPy's float32 arctan2 is within one ulp of
 * that, so alpha and rotation_y agree with the host to a few 2^-22 (modulo 2 pi at the wrap). */
int cn_ddd_post_process_f32(const float *dets, int B, int K, int row_floats, int num_classes,
                            const double *to_source_2x3, int per_image, const float *calibs, float peak_thresh,
                            float *rows, int32_t *bounds, int32_t *kept, void *stream);

/* The same two operations on the HOST, for callers that keep BaseDetector.pre_process on host
 * cores (DataLoader workers; base_detector.py:37-65): identical integer arithmetic, results
 * equal the device kernels bit for bit.  channels <= 4; dst_to_src_2x3 as above. */
int cn_warp_affine_u8_host(const uint8_t *image_hwc, int h_in, int w_in, int channels,
                           const double *dst_to_src_2x3, int h_out, int w_out, uint8_t *out_hwc);
int cn_resize_linear_u8_host(const uint8_t *image_hwc, int h_in, int w_in, int channels, int h_out,
                             int w_out, uint8_t *out_hwc);

/* NV12 video frames -> BGR, in front of the pre-process entry points above (decoders deliver NV12; the
 * pre-process takes packed BGR).  A frame is H rows of luma, then H / 2 rows of interleaved (U, V) at half
 * resolution, every row pitch_bytes (>= W) apart, the chroma plane at pitch_bytes * H; H and W even.
 * Arithmetic: integer BT.601 limited range in 20-bit fixed point, as OpenCV documents COLOR_YUV2BGR_NV12 --
 *   yy = max(0, Y - 16) * 1220542
 *   B = clamp((yy + 2116026 (U - 128)                    + 2^19) >> 20, 0, 255)
 *   G = clamp((yy -  409993 (U - 128) - 852492 (V - 128) + 2^19) >> 20, 0, 255)
 *   R = clamp((yy + 1673527 (V - 128)                    + 2^19) >> 20, 0, 255)
 * with an arithmetic shift of int32 values; one (U, V) pair serves its 2 x 2 block (no chroma interpolation).
 * cn_nv12_to_bgr_u8_batch: N frames on the device, frame_stride_bytes apart (>= pitch_bytes * H * 3 / 2 when
 *   N > 1), to dense (N, H, W, 3) uint8 in one launch.  16-byte loads and stores where every row of both
 *   buffers is 16-byte aligned (pointers, pitch and frame stride multiples of 16, W % 16 == 0), byte accesses
 *   otherwise: any even W and any pitch work.  H, W <= 32767, N <= 65535; CN_ERR_SHAPE for odd or
 *   non-positive H or W, pitch_bytes < W, a short stride or sizes above those limits.
 * cn_nv12_to_bgr_u8_host: one frame on the HOST, the same integers; needs no device. */
int cn_nv12_to_bgr_u8_batch(const uint8_t *nv12, int N, size_t frame_stride_bytes, int H, int W, int pitch_bytes,
                            uint8_t *out_bgr_hwc, void *stream);
int cn_nv12_to_bgr_u8_host(const uint8_t *nv12, int H, int W, int pitch_bytes, uint8_t *out_bgr_hwc);

/* ((image / 255. - mean) / std).astype(float32) + HWC -> CHW of a 3-channel uint8 image on the HOST
 * (base_detector.py:56-58), numpy's float64 arithmetic, one rounding to float32. */
int cn_normalize_u8_chw_f32_host(const uint8_t *image_hwc, int h, int w, const float *mean3,
                                 const float *std3, float *out_chw);

/* Soft-NMS on a HOST array, in place (rows of `stride` floats: x1,y1,x2,y2,score,...).
 * Replaces external.nms.soft_nms / soft_nms_39 (src/lib/external/nms.pyx:77-275), used by
 * merge_outputs when --nms or multi-scale testing is on (detectors/ctdet.py:63-64).
 * method 0 = hard NMS, 1 = linear, 2 = gaussian.  Returns the kept count (>= 0) or < 0. */
int cn_soft_nms_f32(float *boxes_host, int n, int stride, float sigma, float Nt,
                    float threshold, int method);

/* Layout conversion at the API edge. */
int cn_nchw_to_nhwc_f32(const float *x, float *y, int B, int C, int H, int W,
                        int out_pitch, void *stream);
int cn_nhwc_to_nchw_f32(const float *x, float *y, int B, int C, int H, int W,
                        int in_pitch, void *stream);

/* ------------------------------------------------------------------------
 * ctdet decode: sigmoid -> 3x3 peak test -> per-class top-K -> global top-K
 *               -> wh/reg gather -> box assembly.
 *
 * Replaces: ctdet_decode(heat, wh, reg=None, cat_spec_wh=False, K=100)
 *   (models/decode.py:464-495) together with hm.sigmoid_() of
 *   detectors/ctdet.py:31 when apply_sigmoid != 0, i.e. _nms (decode.py:9-15),
 *   _topk (:103-119) and _transpose_and_gather_feat (models/utils.py:22-26).
 *
 * heat (B,C,H,W) NCHW: logits when apply_sigmoid, else post-sigmoid scores
 *   (what the reference function receives).
 * wh (B,2,H,W) or (B,2C,H,W) if cat_spec_wh; reg (B,2,H,W) or NULL.
 * dets (B,K,6) = [x1,y1,x2,y2,score,cls] sorted by score descending.
 * inds (B,K) int32 spatial index of each detection, may be NULL.
 * Tie order (unspecified by torch.topk): score desc, class asc, index asc.
 * Requires K <= 128 and K <= H*W (torch.topk raises for K > H*W).
 * ------------------------------------------------------------------------ */
size_t cn_ctdet_decode_workspace_bytes(int B, int C, int H, int W, int K);

int cn_ctdet_decode_f32(const float *heat, const float *wh, const float *reg,
                        int B, int C, int H, int W, int K, int cat_spec_wh,
                        int apply_sigmoid, float *dets, int32_t *inds,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Flag bits of the `apply_sigmoid` argument of cn_nms_topk_channel_f32 / cn_topk_f32:
 * bit 0 = apply the logistic first (detectors/ctdet.py:31); CN_DECODE_NO_PEAK_TEST = rank every
 * cell, i.e. the plain _topk_channel / _topk without the _nms in front. */
#define CN_DECODE_SIGMOID 1
#define CN_DECODE_NO_PEAK_TEST 512
/* Image-level top-K (cn_ctdet_decode_f32, cn_topk_f32) on planes of <= 128 x 128 cells is ONE kernel
 * launch that reads the heat-map once.  Its per-image state words live in the workspace, must be
 * zero on entry and are left at zero on exit; by default the call zeroes them itself (one small
 * fill in front of the kernel).  CN_DECODE_STATE_CLEAN: the caller owns this workspace exclusively,
 * zeroed it once after allocation (all of it) and has used it for nothing but calls of the same
 * entry point with the same (B, C, H, W, K) since -- the fill is skipped.
 * CN_DECODE_TWO_LAUNCHES selects the two-launch form (group maxima + threshold-pruned collect, the
 * form for larger planes) and 2048 the per-(class, band) select, for comparison; all forms are
 * bit-identical. */
#define CN_DECODE_STATE_CLEAN 4096
/* Byte offset and size, inside the workspace of cn_ctdet_decode_f32 / cn_topk_f32, of the per-image state
 * words of the one-launch form (0 bytes when the shape takes another form).  A CN_DECODE_STATE_CLEAN caller
 * re-zeroes (or checks) exactly this region after a failed or aborted call instead of trusting it. */
int cn_decode_state_region(int B, int C, int H, int W, int K, size_t *offset, size_t *bytes);
#define CN_DECODE_TWO_LAUNCHES 8192
#define CN_DECODE_PER_BAND 2048

/* _nms + _topk_channel (models/decode.py:9-15, 92-101) as one kernel: per
 * (b,c) plane the K best peaks; scores (B,C,K) desc, inds (B,C,K) int32. */
int cn_nms_topk_channel_f32(const float *heat, int B, int C, int H, int W, int K,
                            int apply_sigmoid, float *scores, int32_t *inds,
                            void *workspace, size_t workspace_bytes, void *stream);

/* _nms + _topk (models/decode.py:9-15, 103-119): global top-K over all classes of an image.
 * scores (B,K) desc, inds (B,K) = y*W+x, clses (B,K); ys = inds / W, xs = inds % W.
 * Workspace: cn_ctdet_decode_workspace_bytes. */
int cn_topk_f32(const float *heat, int B, int C, int H, int W, int K, int apply_sigmoid,
                float *scores, int32_t *inds, int32_t *clses, void *workspace,
                size_t workspace_bytes, void *stream);

/* The large-K forms of cn_ctdet_decode_f32 and cn_topk_f32 (cn_decode_large.hip): the same arguments, flags,
 * outputs and tie order, exact for 1 <= K <= CN_DECODE_LARGE_MAX_K (and K <= H*W), and the same rows bit for bit
 * where both take the call.  Two launches -- an exact select per (image, class, row band), then one workgroup per
 * image that selects among the bands' candidates, sorts and writes the rows -- with no state in the workspace:
 * nothing to zero, CN_DECODE_STATE_CLEAN is accepted and ignored, and the result does not depend on the order
 * in which workgroups run.  The workspace carries the candidates from the first launch to the second: calls that
 * may overlap (two streams) need a workspace each.  They allocate nothing and never wait for the device.  Meant for K > 128: below
 * that the entries above are faster.  Workspace: cn_ctdet_decode_large_workspace_bytes for both entries (0 where
 * the call would be refused for its shape or K).  Checks, in this order and before anything is launched: heat NULL
 * -> CN_ERR_NULL; B, K <= 0 or K > H*W -> CN_ERR_SHAPE; K > CN_DECODE_LARGE_MAX_K, W > 4096, C*H*W >= 2^31, or B or
 * C > 65535 (they are grid dimensions) -> CN_ERR_UNSUPPORTED; heat not 16-byte aligned with W % 4 == 0 -> CN_ERR_ALIGN; an output or the workspace NULL
 * -> CN_ERR_NULL; workspace not 16-byte aligned -> CN_ERR_ALIGN; workspace too small -> CN_ERR_WORKSPACE. */
#define CN_DECODE_LARGE_MAX_K 1024
/* ... and where cn_ctdet_decode_f32 / cn_topk_f32 stop, for a caller that routes between the two: */
#define CN_DECODE_MAX_K 128
size_t cn_ctdet_decode_large_workspace_bytes(int B, int C, int H, int W, int K);
int cn_ctdet_decode_large_f32(const float *heat, const float *wh, const float *reg,
                              int B, int C, int H, int W, int K, int cat_spec_wh,
                              int apply_sigmoid, float *dets, int32_t *inds,
                              void *workspace, size_t workspace_bytes, void *stream);
int cn_topk_large_f32(const float *heat, int B, int C, int H, int W, int K, int apply_sigmoid,
                      float *scores, int32_t *inds, int32_t *clses, void *workspace,
                      size_t workspace_bytes, void *stream);

/* The gather-only ctdet heads at the decoded centres (cn_heads_at.hip).  ctdet_decode reads `wh` and `reg`
 * only at the K winning cells of an image (decode.py:472-486), so a caller that does not need the dense
 * maps runs the fused heads for `hm` alone, cn_topk_f32 on it (with the logistic and the peak test:
 * scores, inds, clses) and then this ONE launch: for every (b, k) and each deferred head
 *   ReLU(conv3x3(feat, w1) + bias1) at cell inds[b, k] (padding 1), then the 1x1 (two outputs per head),
 * and the box arithmetic of cn_ctdet_decode_f32: dets (B, K, 6) = [x1, y1, x2, y2, score, cls].
 * feat: NHWC with row pitch `pitch` channels; dtype CN_DTYPE_F32S (real = stored * feat_mul, feat_mul the
 *   tensor's 2^e; pitch a multiple of 32) or CN_DTYPE_F32 (plain floats; feat_mul ignored).  Cin % 32 == 0.
 * n_heads: 1 = wh only (the centre is then cell + 0.5), 2 = wh, reg.  hidden: 64, 128, 192 or 256.
 * w1_packed: cn_pack_cell_heads_w1 of the first convolutions concatenated along Cout,
 *   (n_heads * hidden, Cin, 3, 3) -- the ORIGINAL fp32 weights, not split and not pre-scaled;
 *   bias1 (n_heads * hidden); w2 (n_heads, 2, hidden); bias2 (n_heads, 2) or NULL.
 * Plain fp32 FMA throughout: no range words, nothing clamps.  head_vals: optional (B, K, 2 * n_heads), the
 * raw head outputs [w, h, (reg_x, reg_y)].  A cell index outside the map gives a NaN box, never an
 * out-of-bounds read.  Asynchronous on `stream`, no workspace, no allocation; the same cell may repeat. */
/* cn_pack_cell_heads_w1: w (N, Cin, 3, 3) -> out (9 * Cin / 4, N, 4) floats, 16-byte aligned; N a multiple of
 * 64 up to 768 (three 256-wide heads), Cin % 32 == 0. */
int cn_pack_cell_heads_w1(const float *w, float *out, int N, int Cin, void *stream);
int cn_ctdet_heads_at_cells_f32(const void *feat, int B, int H, int W, int Cin, int pitch, int dtype,
                                float feat_mul, const float *scores, const int32_t *inds,
                                const int32_t *clses, int K, const float *w1_packed, const float *bias1,
                                int hidden, int n_heads, const float *w2, const float *bias2, float *dets,
                                float *head_vals, void *stream);

/* The same launch for the multi_pose task: multi_pose_decode gathers `wh`, `hps` and `reg` at the K centres
 * only (decode.py:506-519), so a caller that does not need those dense maps leaves them out of the fused
 * heads launch, runs cn_topk_f32 on `hm` and then this ONE launch, which evaluates the deferred heads at the
 * B x K cells and writes stage A of cn_multi_pose_decode_f32:
 *   dets (B, K, 5 + 2J + 1) = [x1, y1, x2, y2, score, 2J kps, cls],
 *   kps[2j] = hps[2j] + xi, kps[2j + 1] = hps[2j + 1] + yi (the un-offset integer centre, decode.py:508-509),
 *   xs = xi + reg_x (xi + 0.5 without reg), box = xs -+ w / 2, ys -+ h / 2; one float32 rounding per step.
 * Feature, dtype, alignment and `inds` rules are those of cn_ctdet_heads_at_cells_f32 (a cell outside the map
 * gives a NaN row that keeps score and class; a repeated cell is computed again with the same bits).
 * n_heads: 2 = wh, hps; 3 = wh, hps, reg (this order).  J: joints, 1 .. 17; hps has 2J outputs.
 * hidden: 64, 128, 192 or 256, the same for all heads (n_heads * hidden <= 768).
 * w1_packed / bias1: as above, (n_heads * hidden) rows.  w2 (2 + 2J [+ 2], hidden): the 1x1 rows of the heads
 * concatenated in head order; bias2 (2 + 2J [+ 2]) or NULL.  head_vals: optional (B, K, 2 + 2J [+ 2]), the raw
 * head outputs in head order.  Plain fp32 FMA, no range words, nothing clamps.  Asynchronous on `stream`, no
 * workspace, no allocation, capturable. */
int cn_multi_pose_heads_at_cells_f32(const void *feat, int B, int H, int W, int Cin, int pitch, int dtype,
                                     float feat_mul, const float *scores, const int32_t *inds,
                                     const int32_t *clses, int K, const float *w1_packed, const float *bias1,
                                     int hidden, int n_heads, int J, const float *w2, const float *bias2,
                                     float *dets, float *head_vals, void *stream);

/* The same launch for the ddd task: ddd_decode gathers `dep`, `rot`, `dim`, `wh` and `reg` at the K centres only
 * (decode.py:426-462), so a caller that does not need those dense maps runs the fused heads for `hm` alone,
 * cn_topk_f32 on it and then this ONE launch, which evaluates the deferred heads at the B x K cells and writes the
 * rows of cn_ddd_decode_f32:
 *   dets (B, K, 18) = [xs, ys, score, rot x8, depth, dim x3, wh x2, cls], (B, K, 16) without wh;
 *   xs = xi + reg_x (xi + 0.5 without reg); rot, dim, wh copied; depth copied, or with CN_DECODE_DDD_RAW_DEPTH in
 *   `flags` 1 / (sigmoid(dep) + 1e-6) - 1 -- the same bits as cn_ddd_decode_f32 with that flag on these values.
 * The heads are, in this order, dep (1 output), rot (8), dim (3)[, wh (2) if has_wh][, reg (2) if has_reg], all with
 * `hidden` (64, 128, 192 or 256) hidden channels.  They are evaluated in `n_groups` (1 .. 5) groups of consecutive
 * heads, one workgroup per (image, 16 cells, group): group g takes the next groups[g].n_heads (1 .. 3,
 * n_heads * hidden <= 768) heads of the list, and the groups together take every head once.  Each group has its
 * own weights, laid out as for cn_ctdet_heads_at_cells_f32: w1_packed = cn_pack_cell_heads_w1 of the group's
 * first convolutions concatenated along Cout, bias1 (n_heads * hidden), w2 (sum of the group's outputs, hidden),
 * bias2 (sum of the group's outputs) or NULL.  Every column of a row depends on one head, so the result does
 * not depend on the grouping and is the same from run to run.
 * Feature, dtype, alignment and `inds` rules are those of cn_ctdet_heads_at_cells_f32 (a cell outside the map gives
 * NaN in every head-derived column and in head_vals; score and class are still written).  head_vals: optional
 * (B, K, 12 [+ 2] [+ 2]), the raw (untransformed) head outputs in head order.  Plain fp32 FMA, no range words,
 * nothing clamps.  Asynchronous on `stream`, no workspace, no allocation, capturable. */
typedef struct cn_cell_head_group {
    const float *w1_packed;
    const float *bias1;
    const float *w2;
    const float *bias2;
    int n_heads;
    int reserved;
} cn_cell_head_group;
int cn_ddd_heads_at_cells_f32(const void *feat, int B, int H, int W, int Cin, int pitch, int dtype,
                              float feat_mul, const float *scores, const int32_t *inds, const int32_t *clses,
                              int K, int hidden, int n_groups, const cn_cell_head_group *groups, int has_wh,
                              int has_reg, int flags, float *dets, float *head_vals, void *stream);

/* _transpose_and_gather_feat (models/utils.py:12-26): out[b,k,c] = feat[b,c,inds[b,k]] for an
 * NCHW map, without the reference's full-tensor permute().contiguous(). */
int cn_gather_feat_f32(const float *feat, const int32_t *inds, float *out, int B, int C, int H,
                       int W, int K, void *stream);

/* ddd_decode(heat, rot, depth, dim, wh=None, reg=None, K=40) (models/decode.py:426-462):
 * dets (B,K,16) = [xs, ys, score, rot x8, depth, dim x3, cls], or (B,K,18) with wh x2 before
 * cls when wh != NULL.  heat is post-sigmoid unless apply_sigmoid; depth is passed as the
 * caller prepared it (the detector applies 1/(sigmoid(dep)+1e-6)-1 first, detectors/ddd.py:55) unless
 * CN_DECODE_DDD_RAW_DEPTH is set. */
size_t cn_ddd_decode_workspace_bytes(int B, int C, int H, int W, int K);
/* Flag bit of cn_ddd_decode_f32's `apply_sigmoid`: `depth` is the head's RAW map and the K gathered values
 * are transformed here, 1 / (logistic(v) + 1e-6f) - 1 in float32 with the library's logistic, instead of
 * an element-wise pass over the whole map in front of the call. */
#define CN_DECODE_DDD_RAW_DEPTH 16384
int cn_ddd_decode_f32(const float *heat, const float *rot, const float *depth, const float *dim,
                      const float *wh, const float *reg, int B, int C, int H, int W, int K,
                      int apply_sigmoid, float *dets, void *workspace, size_t workspace_bytes,
                      void *stream);

/* Edge aggregation in front of exct_decode when aggr_weight > 0 (models/decode.py:17-90, :136-140):
 * out = _h_aggregate(heat, aggr_weight) (horizontal = 1: t_heat, b_heat) or _v_aggregate (horizontal =
 * 0: l_heat, r_heat); heat, out (B, C, H, W), out != heat.  Bit-identical to the reference's float32
 * arithmetic. */
int cn_exct_aggregate_f32(const float *heat, float *out, int B, int C, int H, int W, int horizontal,
                          float aggr_weight, void *stream);
/* exct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr.., K=40, scores_thresh=0.1,
 *             center_thresh=0.1, aggr_weight=0.0, num_dets=1000)   (models/decode.py:273-424)
 * for aggr_weight == 0: dets (B, num_dets, 14) = [l_x, t_y, r_x, b_y, score, t_x, t_y, l_x, l_y,
 * b_x, b_y, r_x, r_y, cls].  The four regression maps are used only when all are given
 * (decode.py:372-373).  Heat-maps are post-sigmoid.  K <= 64, num_dets <= 1024.
 * Tie order of equal scores (unspecified by torch.topk): candidate index ascending.
 * The `apply_sigmoid` argument carries flags: bit 0 (the logistic) is not supported here;
 * CN_EXCT_CLAMP_ONE = the edge maps may exceed 1 (they are aggregated maps, cn_exct_aggregate_f32):
 * after the 3x3 peak test the surviving values are clamped to 1 before the top-K, as the reference
 * does (decode.py:302-305: `t_heat[t_heat > 1] = 1` behind `_nms`); runs one more pass per edge map. */
#define CN_EXCT_CLAMP_ONE 2
size_t cn_exct_decode_workspace_bytes(int B, int C, int H, int W, int K);
int cn_exct_decode_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                       const float *r_heat, const float *ct_heat, const float *t_regr,
                       const float *l_regr, const float *b_regr, const float *r_regr, int B, int C,
                       int H, int W, int K, float scores_thresh, float center_thresh, int num_dets,
                       int apply_sigmoid, float *dets, void *workspace, size_t workspace_bytes,
                       void *stream);
/* agnex_ct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr.., K=40, scores_thresh=0.1,
 *                 center_thresh=0.1, aggr_weight=0.0, num_dets=1000)   (models/decode.py:121-271), the
 * class-agnostic form behind --agnostic_ex (detectors/exdet.py:26): the four edge maps are (B, 1, H, W), the
 * centre map (B, C, H, W); a grouping is scored against the per-cell MAXIMUM of the centre map over the classes
 * (torch.max(ct_heat, dim=1), decode.py:164), there is no class rule, and a detection's class is the arg-max
 * (first on ties) at the box centre.  Same row layout, limits, tie order and `flags` (CN_EXCT_CLAMP_ONE) as
 * cn_exct_decode_f32; the scores are that function's over single-channel maps, bit for bit. */
size_t cn_agnex_ct_decode_workspace_bytes(int B, int C, int H, int W, int K);
int cn_agnex_ct_decode_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                           const float *r_heat, const float *ct_heat, const float *t_regr,
                           const float *l_regr, const float *b_regr, const float *r_regr, int B, int C,
                           int H, int W, int K, float scores_thresh, float center_thresh, int num_dets,
                           int flags, float *dets, void *workspace, size_t workspace_bytes,
                           void *stream);
/* The streaming forms of the two decodes above: same arguments, same rows bit for bit (same scores, same tie
 * order: score descending, candidate index ascending), for 1 <= K <= 128 (K^4 <= 2^28 candidate indices) and
 * num_dets <= 1024 -- the reference's --K default of 100 included.  The K^4 candidate scores are never stored:
 * the exact top num_dets is a radix select over the 64-bit (score, ~index) keys whose every step scores the
 * candidates again from the four top-K lists (per key digit a count launch over (t, l) slabs and a
 * one-workgroup-per-image pick launch, then a collect launch and a sort + row launch; a fixed launch sequence,
 * steps an image no longer needs return at once).  Workspace: the top-K workspace, the twelve lists, the one
 * clamped map of CN_EXCT_CLAMP_ONE and under 1 MiB of select state per image, which the call zeroes itself.
 * No host synchronisation; capturable in a graph.  Refusals as the stored forms': CN_ERR_NULL, CN_ERR_SHAPE
 * (num_dets <= 0, K <= 0, num_dets > K^4), CN_ERR_UNSUPPORTED (K > 128, num_dets > 1024, other flags),
 * CN_ERR_WORKSPACE -- all before anything is launched.  CN_EXCT_STORED_MAX_K / CN_EXCT_STREAM_MAX_K: the largest K
 * of the stored and of the streaming forms. */
#define CN_EXCT_STORED_MAX_K 64
#define CN_EXCT_STREAM_MAX_K 128
size_t cn_exct_decode_stream_workspace_bytes(int B, int C, int H, int W, int K);
int cn_exct_decode_stream_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                              const float *r_heat, const float *ct_heat, const float *t_regr,
                              const float *l_regr, const float *b_regr, const float *r_regr, int B, int C,
                              int H, int W, int K, float scores_thresh, float center_thresh, int num_dets,
                              int apply_sigmoid, float *dets, void *workspace, size_t workspace_bytes,
                              void *stream);
size_t cn_agnex_ct_decode_stream_workspace_bytes(int B, int C, int H, int W, int K);
int cn_agnex_ct_decode_stream_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                                  const float *r_heat, const float *ct_heat, const float *t_regr,
                                  const float *l_regr, const float *b_regr, const float *r_regr, int B, int C,
                                  int H, int W, int K, float scores_thresh, float center_thresh, int num_dets,
                                  int flags, float *dets, void *workspace, size_t workspace_bytes,
                                  void *stream);

/* ------------------------------------------------------------------------
 * multi_pose decode.
 * Replaces: multi_pose_decode(heat, wh, kps, reg, hm_hp, hp_offset, K)
 *   (models/decode.py:497-571).  dets (B,K,4+1+2J+1).
 * ------------------------------------------------------------------------ */
size_t cn_multi_pose_decode_workspace_bytes(int B, int C, int H, int W, int J, int K);

int cn_multi_pose_decode_f32(const float *heat, const float *wh, const float *kps,
                             const float *reg, const float *hm_hp,
                             const float *hp_offset, int B, int C, int H, int W,
                             int J, int K, int apply_sigmoid, float *dets,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Stages B and C of cn_multi_pose_decode_f32 on rows that already hold stage A (from that function without
 * hm_hp, or from cn_multi_pose_heads_at_cells_f32): _nms + _topk_channel on hm_hp (B, J, H, W) -- one or two
 * launches, by the band plan -- then the joint match (decode.py:528-569) with the dense hp_offset (B, 2, H, W)
 * or NULL (candidate + 0.5); dets (B, K, 5 + 2J + 1) is updated in place.  cn_multi_pose_decode_f32 runs the
 * same internal function, so the two give the same bits.  flags: CN_DECODE_SIGMOID = hm_hp holds logits.
 * K <= 128.  Workspace: cn_multi_pose_decode_workspace_bytes(B, 1, H, W, J, K) suffices. */
int cn_multi_pose_match_f32(const float *hm_hp, const float *hp_offset, int B, int J, int H, int W, int K,
                            int flags, float *dets, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CENTERNET_AMD_H */
