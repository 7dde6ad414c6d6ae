// cn_pre.hip -- BaseDetector.pre_process on the device and on the host.
//
// Replaces the host sequence of src/lib/detectors/base_detector.py:37-65:
//   resized = cv2.resize(image, (new_w, new_h))                         [scale != 1 only]
//   inp     = cv2.warpAffine(resized, trans_input, (inp_w, inp_h), flags=cv2.INTER_LINEAR)
//   inp     = ((inp / 255. - mean) / std).astype(np.float32)            (float64 arithmetic)
//   images  = inp.transpose(2, 0, 1)[None]; optional flip concat (:59-60)
// so that a uint8 frame (0.79 MB at 512x512) crosses PCIe instead of the fp32 tensor (3.1 MB)
// and the warp does not run on a host core.
//
// This is byte work and the bar is bit-exactness with what the reference computes, i.e. with
// OpenCV's uint8 INTER_LINEAR path -- a FIXED-POINT algorithm, not float bilinear (published in
// modules/imgproc/src/imgwarp.cpp and resize.cpp; restated with its constants in
// oracle/pre_oracle.py, which is the definition these kernels are tested against bit for bit):
//   warpAffine: source position of a destination pixel in 1/32 pixel,
//       X = (rn((m1*y + m2) * 1024) + 16 + rn((m0*x) * 1024)) >> 5      (same for Y with m3..m5;
//       m = the inverted matrix, double arithmetic, rn = round-half-even to int)
//     tap (X >> 5, Y >> 5), fractions fx = X & 31, fy = Y & 31, int16 weights
//       [(32-fy)(32-fx), (32-fy)fx, fy(32-fx), fy*fx] * 32   (sum 2^15; fraction (0,0): [32767,0,0,1]),
//     taps outside the image = 0, dst = clamp((sum + 2^14) >> 15).
//   resize (INTER_LINEAR): same size = copy; exactly half size = (a+b+c+d+2) >> 2; otherwise
//     separable with 11-bit coefficients rn((1-f)*2048), rn(f*2048), f from
//     float((d + 0.5)*scale - 0.5), exact horizontal pass and the uint8 vertical pass
//     (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.
// Normalisation: ((v/255.) - mean)/std in float64, rounded once to float32 (numpy's arithmetic
// for a uint8 array and float32 mean / std arrays).  No FMA contraction anywhere.
#include "cn_common.h"
#include <cstdlib>

// hipcc defaults to -ffp-contract=fast-honor-pragmas, and HIP's __dmul_rn/__dadd_rn are inline
// header functions compiled under that default (their results still fuse after inlining), so
// the arithmetic below is written with plain operators under an explicit contract(off).
#pragma clang fp contract(off)

namespace {

constexpr int AB_BITS = 10, INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS, COEF_BITS = 15;

struct WarpArgs {
    const uint8_t *img;  // (H, W, 3) uint8, row pitch in bytes
    int H, W, pitch;
    double m[6];         // dst -> src (already inverted the way cv::warpAffine inverts it)
    int oh, ow;
    double mean[3], stdv[3];
    float *out;          // (1|2, 3, oh, ow) per image
    int flip;
    size_t img_stride, out_stride;   // bytes / floats from one image of a batch to the next (blockIdx.z)
};

// four int16-range weights of a 1/32-pixel fraction pair (initInterTab2D, INTER_LINEAR, fixed point)
__host__ __device__ inline void frac_weights(int fx, int fy, int w[4])
{
    if ((fx | fy) == 0) {      // 1.0 * 32768 saturates to 32767; the table's fix-up puts the 1 on tap 3
        w[0] = 32767; w[1] = 0; w[2] = 0; w[3] = 1;
        return;
    }
    w[0] = (INTER_TAB - fy) * (INTER_TAB - fx) * 32;
    w[1] = (INTER_TAB - fy) * fx * 32;
    w[2] = fy * (INTER_TAB - fx) * 32;
    w[3] = fy * fx * 32;
}

__host__ __device__ inline int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one destination pixel of cv::warpAffine (uint8, C channels interleaved): v[c] = 0..255
template <int C>
__host__ __device__ inline void warp_pixel(const uint8_t *img, int H, int W, size_t pitch, const double *m,
                                           int x, int y, int rx0, int ry0, int v[C])
{
    // rx0 / ry0 = rn((m1*y + m2)*1024) + 16, rn((m4*y + m5)*1024) + 16: per row, from the caller
#ifdef __HIP_DEVICE_COMPILE__
    const int ad = __double2int_rn((m[0] * (double)x) * 1024.0);
    const int bd = __double2int_rn((m[3] * (double)x) * 1024.0);
#else
    const int ad = (int)__builtin_nearbyint((m[0] * (double)x) * 1024.0);
    const int bd = (int)__builtin_nearbyint((m[3] * (double)x) * 1024.0);
#endif
    const int X = (rx0 + ad) >> (AB_BITS - INTER_BITS), Y = (ry0 + bd) >> (AB_BITS - INTER_BITS);
    const int sx = clamp_i(X >> INTER_BITS, -32768, 32767), sy = clamp_i(Y >> INTER_BITS, -32768, 32767);
    int w[4];
    frac_weights(X & (INTER_TAB - 1), Y & (INTER_TAB - 1), w);
    const bool x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
    const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H;
    const uint8_t *r0 = img + (size_t)clamp_i(sy, 0, H - 1) * pitch;
    const uint8_t *r1 = img + (size_t)clamp_i(sy + 1, 0, H - 1) * pitch;
    const int c0 = clamp_i(sx, 0, W - 1) * C, c1 = clamp_i(sx + 1, 0, W - 1) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int t00 = (x0 && y0) ? r0[c0 + c] : 0, t01 = (x1 && y0) ? r0[c1 + c] : 0;
        const int t10 = (x0 && y1) ? r1[c0 + c] : 0, t11 = (x1 && y1) ? r1[c1 + c] : 0;
        const int s = t00 * w[0] + t01 * w[1] + t10 * w[2] + t11 * w[3];
        v[c] = clamp_i((s + (1 << (COEF_BITS - 1))) >> COEF_BITS, 0, 255);
    }
}

__host__ __device__ inline int row_base(const double *m, int a, int b, int y)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __double2int_rn((m[a] * (double)y + m[b]) * 1024.0) + (1 << AB_BITS) / INTER_TAB / 2;
#else
    return (int)__builtin_nearbyint((m[a] * (double)y + m[b]) * 1024.0) + (1 << AB_BITS) / INTER_TAB / 2;
#endif
}

__global__ void warp_normalize_kernel(const WarpArgs a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.ow) return;
    int v[3];
    const uint8_t *img = a.img + (size_t)blockIdx.z * a.img_stride;
    float *out = a.out + (size_t)blockIdx.z * a.out_stride;
    warp_pixel<3>(img, a.H, a.W, (size_t)a.pitch, a.m, x, y, row_base(a.m, 1, 2, y), row_base(a.m, 4, 5, y), v);
    const size_t plane = (size_t)a.oh * a.ow;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double n = ((double)v[c] / 255.0 - a.mean[c]) / a.stdv[c];
        const float f = (float)n;
        out[c * plane + (size_t)y * a.ow + x] = f;
        if (a.flip) out[(3 + c) * plane + (size_t)y * a.ow + (a.ow - 1 - x)] = f;
    }
}

// ---- cv::resize INTER_LINEAR, uint8 ----------------------------------------------------------
struct ResizeArgs {
    const uint8_t *img;
    int H, W, pitch, oh, ow;
    double scale_x, scale_y;   // 1. / (out / in), as resize.cpp forms them
    int mode;                  // 0 = linear, 1 = exactly half size (2x2 mean)
    uint8_t *out;              // (oh, ow, 3) dense
};

// left tap and the two 11-bit coefficients of destination index d (resize.cpp xofs/ialpha, yofs/ibeta)
__host__ __device__ inline void axis_coef(int d, double scale, int n_in, bool clamp_fraction, int *s, int *c0, int *c1)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int i = (int)__builtin_floorf(f);
    f = f - (float)i;
    if (clamp_fraction) {
        if (i < 0) { f = 0.f; i = 0; }
        if (i >= n_in - 1) { f = 0.f; i = n_in - 1; }
    }
    const float g = 1.f - f;
#ifdef __HIP_DEVICE_COMPILE__
    *c0 = __float2int_rn(g * 2048.f);
    *c1 = __float2int_rn(f * 2048.f);
#else
    *c0 = (int)__builtin_nearbyintf(g * 2048.f);
    *c1 = (int)__builtin_nearbyintf(f * 2048.f);
#endif
    *s = i;
}

template <int C>
__host__ __device__ inline void resize_pixel(const uint8_t *img, int H, int W, size_t pitch, double scx,
                                             double scy, int mode, int x, int y, int v[C])
{
    if (mode == 1) {
        const uint8_t *r0 = img + (size_t)(2 * y) * pitch + (size_t)(2 * x) * C, *r1 = r0 + pitch;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (r0[c] + r0[C + c] + r1[c] + r1[C + c] + 2) >> 2;
        return;
    }
    int sx, a0, a1, sy, b0, b1;
    axis_coef(x, scx, W, true, &sx, &a0, &a1);
    axis_coef(y, scy, H, false, &sy, &b0, &b1);
    const uint8_t *r0 = img + (size_t)clamp_i(sy, 0, H - 1) * pitch;
    const uint8_t *r1 = img + (size_t)clamp_i(sy + 1, 0, H - 1) * pitch;
    const int c0 = sx * C, c1 = clamp_i(sx + 1, 0, W - 1) * C;   // a1 = 0 wherever sx + 1 is outside
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int S0 = r0[c0 + c] * a0 + r0[c1 + c] * a1;
        const int S1 = r1[c0 + c] * a0 + r1[c1 + c] * a1;
        v[c] = clamp_i((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, 0, 255);
    }
}

__global__ void resize_u8_kernel(const ResizeArgs a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.ow) return;
    int v[3];
    resize_pixel<3>(a.img, a.H, a.W, (size_t)a.pitch, a.scale_x, a.scale_y, a.mode, x, y, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out[((size_t)y * a.ow + x) * 3 + c] = (uint8_t)v[c];
}

}  // namespace

extern "C" int cn_warp_normalize_u8_f32(const uint8_t *image_hwc, int H, int W, int pitch_bytes,
                                        const double *dst_to_src_2x3, int out_h, int out_w,
                                        const float *mean3, const float *std3, int flip_concat,
                                        float *out_nchw, void *stream)
{
    return cn_warp_normalize_u8_f32_batch(image_hwc, 1, 0, H, W, pitch_bytes, dst_to_src_2x3, out_h, out_w,
                                          mean3, std3, flip_concat, out_nchw, stream);
}

extern "C" int cn_warp_normalize_u8_f32_batch(const uint8_t *images_hwc, int N, size_t image_stride_bytes,
                                              int H, int W, int pitch_bytes, const double *dst_to_src_2x3,
                                              int out_h, int out_w, const float *mean3, const float *std3,
                                              int flip_concat, float *out_nchw, void *stream)
{
    const uint8_t *image_hwc = images_hwc;
    if (!image_hwc || !dst_to_src_2x3 || !mean3 || !std3 || !out_nchw) return CN_ERR_NULL;
    if (H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || pitch_bytes < 3 * W || out_h > 65535 ||
        H > 32767 || W > 32767 || N <= 0 || N > 65535)
        return CN_ERR_SHAPE;
    if (N > 1 && image_stride_bytes < (size_t)pitch_bytes * (size_t)H) return CN_ERR_SHAPE;
    WarpArgs a = {};
    a.img = image_hwc; a.H = H; a.W = W; a.pitch = pitch_bytes; a.oh = out_h; a.ow = out_w;
    for (int i = 0; i < 6; ++i) a.m[i] = dst_to_src_2x3[i];
    for (int c = 0; c < 3; ++c) {
        if (std3[c] == 0.f) return CN_ERR_SHAPE;
        a.mean[c] = (double)mean3[c];
        a.stdv[c] = (double)std3[c];
    }
    a.out = out_nchw; a.flip = flip_concat ? 1 : 0;
    a.img_stride = image_stride_bytes;
    a.out_stride = (size_t)(a.flip ? 6 : 3) * out_h * out_w;
    dim3 grid(cn_cdiv(out_w, 128), out_h, N);
    hipLaunchKernelGGL(warp_normalize_kernel, grid, dim3(128), 0, (hipStream_t)stream, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_resize_bilinear_u8(const uint8_t *image_hwc, int H, int W, int pitch_bytes,
                                     int out_h, int out_w, uint8_t *out_hwc, void *stream)
{
    if (!image_hwc || !out_hwc) return CN_ERR_NULL;
    if (H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || pitch_bytes < 3 * W || out_h > 65535) return CN_ERR_SHAPE;
    if (H == out_h && W == out_w) {      // cv::resize: same size = copy
        return hipMemcpy2DAsync(out_hwc, (size_t)3 * W, image_hwc, (size_t)pitch_bytes, (size_t)3 * W, H,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? CN_OK : CN_ERR_LAUNCH;
    }
    ResizeArgs a = {};
    a.img = image_hwc; a.H = H; a.W = W; a.pitch = pitch_bytes; a.oh = out_h; a.ow = out_w;
    a.scale_x = 1.0 / ((double)out_w / (double)W);
    a.scale_y = 1.0 / ((double)out_h / (double)H);
    a.mode = (H == 2 * out_h && W == 2 * out_w) ? 1 : 0;
    a.out = out_hwc;
    dim3 grid(cn_cdiv(out_w, 128), out_h);
    hipLaunchKernelGGL(resize_u8_kernel, grid, dim3(128), 0, (hipStream_t)stream, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// ---- mixed-size batches: N images of their own sizes, packed in one uint8 buffer, one launch ----
// The geometry of image blockIdx.z comes from its cn_image_desc in device memory (it travels with the
// frames on the copy stream); the pixel arithmetic is warp_pixel / row_base / resize_pixel above.
namespace {

struct RaggedWarpArgs {
    int oh, ow;
    double mean[3], stdv[3];
    float *out;          // (N, 3|6, oh, ow)
    int flip;
    size_t out_stride;
};

__global__ void warp_normalize_ragged_kernel(const uint8_t *__restrict__ packed,
                                             const cn_image_desc *__restrict__ descs, const RaggedWarpArgs a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    // uniform over the workgroup: one read through the const __restrict__ pointer, kept in scalar registers
    const cn_image_desc d = descs[blockIdx.z];
    if (x >= a.ow || d.H <= 0 || d.W <= 0) return;
    int v[3];
    float *out = a.out + (size_t)blockIdx.z * a.out_stride;
    warp_pixel<3>(packed + d.offset, d.H, d.W, (size_t)d.pitch, d.dst_to_src, x, y,
                  row_base(d.dst_to_src, 1, 2, y), row_base(d.dst_to_src, 4, 5, y), v);
    const size_t plane = (size_t)a.oh * a.ow;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double n = ((double)v[c] / 255.0 - a.mean[c]) / a.stdv[c];
        const float f = (float)n;
        out[c * plane + (size_t)y * a.ow + x] = f;
        if (a.flip) out[(3 + c) * plane + (size_t)y * a.ow + (a.ow - 1 - x)] = f;
    }
}

__global__ void resize_u8_ragged_kernel(const uint8_t *__restrict__ packed_in,
                                        const cn_image_desc *__restrict__ in_descs,
                                        uint8_t *__restrict__ packed_out,
                                        const cn_image_desc *__restrict__ out_descs)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    const cn_image_desc s = in_descs[blockIdx.z], d = out_descs[blockIdx.z];
    if (x >= d.W || y >= d.H || s.H <= 0 || s.W <= 0) return;
    const uint8_t *img = packed_in + s.offset;
    uint8_t *o = packed_out + d.offset + (size_t)y * d.pitch + (size_t)x * 3;
    if (s.H == d.H && s.W == d.W) {      // cv::resize: same size = copy
        const uint8_t *p = img + (size_t)y * s.pitch + (size_t)x * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = p[c];
        return;
    }
    int v[3];
    resize_pixel<3>(img, s.H, s.W, (size_t)s.pitch, d.scale_x, d.scale_y,
                    (s.H == 2 * d.H && s.W == 2 * d.W) ? 1 : 0, x, y, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
}

}  // namespace

extern "C" int cn_warp_normalize_u8_f32_ragged(const uint8_t *packed, const cn_image_desc *descs_dev, int N,
                                               int out_h, int out_w, const float *mean3, const float *std3,
                                               int flip_concat, float *out_nchw, void *stream)
{
    if (!packed || !descs_dev || !mean3 || !std3 || !out_nchw) return CN_ERR_NULL;
    if (out_h <= 0 || out_w <= 0 || out_h > 65535 || N <= 0 || N > 65535) return CN_ERR_SHAPE;
    RaggedWarpArgs a = {};
    a.oh = out_h; a.ow = out_w;
    for (int c = 0; c < 3; ++c) {
        if (std3[c] == 0.f) return CN_ERR_SHAPE;
        a.mean[c] = (double)mean3[c];
        a.stdv[c] = (double)std3[c];
    }
    a.out = out_nchw; a.flip = flip_concat ? 1 : 0;
    a.out_stride = (size_t)(a.flip ? 6 : 3) * out_h * out_w;
    dim3 grid(cn_cdiv(out_w, 128), out_h, N);
    hipLaunchKernelGGL(warp_normalize_ragged_kernel, grid, dim3(128), 0, (hipStream_t)stream, packed, descs_dev, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_resize_bilinear_u8_ragged(const uint8_t *packed_in, const cn_image_desc *in_descs_dev,
                                            uint8_t *packed_out, const cn_image_desc *out_descs_dev, int N,
                                            int max_out_h, int max_out_w, void *stream)
{
    if (!packed_in || !in_descs_dev || !packed_out || !out_descs_dev) return CN_ERR_NULL;
    if (max_out_h <= 0 || max_out_w <= 0 || max_out_h > 65535 || N <= 0 || N > 65535) return CN_ERR_SHAPE;
    dim3 grid(cn_cdiv(max_out_w, 128), max_out_h, N);
    hipLaunchKernelGGL(resize_u8_ragged_kernel, grid, dim3(128), 0, (hipStream_t)stream, packed_in, in_descs_dev,
                       packed_out, out_descs_dev);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// ---- the same two operations on the HOST (callers that keep BaseDetector.pre_process on host
// cores, e.g. DataLoader workers: base_detector.py:37-65): the integer algorithms above, pixel by
// pixel in C; channels <= 4.
template <int C>
static void warp_host(const uint8_t *img, int h_in, int w_in, const double *m, int h_out, int w_out, uint8_t *out)
{
    // the per-column terms rn(m0*x*1024), rn(m3*x*1024) once per call (cv::warpAffine's adelta /
    // bdelta tables), so that the pixel loop is integer-only; interior pixels (all four taps on
    // the image) skip the border tests.  Same integers as warp_pixel<C>.
    int *adelta = (int *)malloc((size_t)2 * w_out * sizeof(int));
    if (!adelta) {   // out of memory: the plain per-pixel form
        for (int y = 0; y < h_out; ++y) {
            const int rx0 = row_base(m, 1, 2, y), ry0 = row_base(m, 4, 5, y);
            for (int x = 0; x < w_out; ++x) {
                int v[C];
                warp_pixel<C>(img, h_in, w_in, (size_t)w_in * C, m, x, y, rx0, ry0, v);
                for (int c = 0; c < C; ++c) out[((size_t)y * w_out + x) * C + c] = (uint8_t)v[c];
            }
        }
        return;
    }
    int *bdelta = adelta + w_out;
    for (int x = 0; x < w_out; ++x) {
        adelta[x] = (int)__builtin_nearbyint((m[0] * (double)x) * 1024.0);
        bdelta[x] = (int)__builtin_nearbyint((m[3] * (double)x) * 1024.0);
    }
    const size_t pitch = (size_t)w_in * C;
    for (int y = 0; y < h_out; ++y) {
        const int rx0 = row_base(m, 1, 2, y), ry0 = row_base(m, 4, 5, y);
        uint8_t *orow = out + (size_t)y * w_out * C;
        for (int x = 0; x < w_out; ++x) {
            const int X = (rx0 + adelta[x]) >> (AB_BITS - INTER_BITS), Y = (ry0 + bdelta[x]) >> (AB_BITS - INTER_BITS);
            const int sx = clamp_i(X >> INTER_BITS, -32768, 32767), sy = clamp_i(Y >> INTER_BITS, -32768, 32767);
            int w[4];
            frac_weights(X & (INTER_TAB - 1), Y & (INTER_TAB - 1), w);
            if (sx >= 0 && sx + 1 < w_in && sy >= 0 && sy + 1 < h_in) {
                const uint8_t *p0 = img + (size_t)sy * pitch + (size_t)sx * C, *p1 = p0 + pitch;
                for (int c = 0; c < C; ++c) {
                    const int sum = p0[c] * w[0] + p0[C + c] * w[1] + p1[c] * w[2] + p1[C + c] * w[3];
                    orow[x * C + c] = (uint8_t)clamp_i((sum + (1 << (COEF_BITS - 1))) >> COEF_BITS, 0, 255);
                }
                continue;
            }
            const bool x0 = sx >= 0 && sx < w_in, x1 = sx + 1 >= 0 && sx + 1 < w_in;
            const bool y0 = sy >= 0 && sy < h_in, y1 = sy + 1 >= 0 && sy + 1 < h_in;
            const uint8_t *r0 = img + (size_t)clamp_i(sy, 0, h_in - 1) * pitch;
            const uint8_t *r1 = img + (size_t)clamp_i(sy + 1, 0, h_in - 1) * pitch;
            const int c0 = clamp_i(sx, 0, w_in - 1) * C, c1 = clamp_i(sx + 1, 0, w_in - 1) * C;
            for (int c = 0; c < C; ++c) {
                const int t00 = (x0 && y0) ? r0[c0 + c] : 0, t01 = (x1 && y0) ? r0[c1 + c] : 0;
                const int t10 = (x0 && y1) ? r1[c0 + c] : 0, t11 = (x1 && y1) ? r1[c1 + c] : 0;
                const int sum = t00 * w[0] + t01 * w[1] + t10 * w[2] + t11 * w[3];
                orow[x * C + c] = (uint8_t)clamp_i((sum + (1 << (COEF_BITS - 1))) >> COEF_BITS, 0, 255);
            }
        }
    }
    free(adelta);
}

extern "C" int cn_warp_affine_u8_host(const uint8_t *img, int h_in, int w_in, int channels,
                                      const double *dst_to_src_2x3, int h_out, int w_out, uint8_t *out)
{
    if (!img || !dst_to_src_2x3 || !out) return CN_ERR_NULL;
    if (h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0 || channels <= 0 || channels > 4 ||
        h_in > 32767 || w_in > 32767)
        return CN_ERR_SHAPE;
    switch (channels) {
    case 1: warp_host<1>(img, h_in, w_in, dst_to_src_2x3, h_out, w_out, out); break;
    case 2: warp_host<2>(img, h_in, w_in, dst_to_src_2x3, h_out, w_out, out); break;
    case 3: warp_host<3>(img, h_in, w_in, dst_to_src_2x3, h_out, w_out, out); break;
    default: warp_host<4>(img, h_in, w_in, dst_to_src_2x3, h_out, w_out, out); break;
    }
    return CN_OK;
}

template <int C>
static void resize_host(const uint8_t *img, int h_in, int w_in, int h_out, int w_out, uint8_t *out)
{
    const double scx = 1.0 / ((double)w_out / (double)w_in), scy = 1.0 / ((double)h_out / (double)h_in);
    const int mode = (h_in == 2 * h_out && w_in == 2 * w_out) ? 1 : 0;
    for (int y = 0; y < h_out; ++y)
        for (int x = 0; x < w_out; ++x) {
            int v[C];
            resize_pixel<C>(img, h_in, w_in, (size_t)w_in * C, scx, scy, mode, x, y, v);
            for (int c = 0; c < C; ++c) out[((size_t)y * w_out + x) * C + c] = (uint8_t)v[c];
        }
}

extern "C" int cn_resize_linear_u8_host(const uint8_t *img, int h_in, int w_in, int channels, int h_out,
                                        int w_out, uint8_t *out)
{
    if (!img || !out) return CN_ERR_NULL;
    if (h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0 || channels <= 0 || channels > 4) return CN_ERR_SHAPE;
    if (h_in == h_out && w_in == w_out) {
        __builtin_memcpy(out, img, (size_t)h_in * w_in * channels);
        return CN_OK;
    }
    switch (channels) {
    case 1: resize_host<1>(img, h_in, w_in, h_out, w_out, out); break;
    case 2: resize_host<2>(img, h_in, w_in, h_out, w_out, out); break;
    case 3: resize_host<3>(img, h_in, w_in, h_out, w_out, out); break;
    default: resize_host<4>(img, h_in, w_in, h_out, w_out, out); break;
    }
    return CN_OK;
}


// ---------------------------------------------------------------------------
// ddd task, the batched pre-process: cn_warp_table_u8_f32_batch -- the ddd class normalises with a
// FLOAT32 chain, (u8 / 255 - mean) / std (detectors/ddd.py:45-46), not the float64-then-round of
// warp_normalize_kernel.  A uint8 level has 256 values, so the caller builds the 3 x 256 results with
// exactly those float32 operations once and the kernel looks them up: same sampler, same zero border,
// out = table[c][v].
// ---------------------------------------------------------------------------
namespace {
struct WarpTableArgs {
    const uint8_t *img;
    int H, W, pitch;
    double m[6];
    int oh, ow;
    const float *table;  // (3, 256) on the device
    float *out;          // (N, 3, oh, ow)
    size_t img_stride, out_stride;
};

__global__ void warp_table_kernel(const WarpTableArgs a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.ow) return;
    int v[3];
    const uint8_t *img = a.img + (size_t)blockIdx.z * a.img_stride;
    float *out = a.out + (size_t)blockIdx.z * a.out_stride;
    warp_pixel<3>(img, a.H, a.W, (size_t)a.pitch, a.m, x, y, row_base(a.m, 1, 2, y), row_base(a.m, 4, 5, y), v);
    const size_t plane = (size_t)a.oh * a.ow;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane + (size_t)y * a.ow + x] = a.table[c * 256 + v[c]];
}
}  // namespace

extern "C" int cn_warp_table_u8_f32_batch(const uint8_t *images_hwc, int N, size_t image_stride_bytes, int H, int W,
                                          int pitch_bytes, const double *dst_to_src_2x3, int out_h, int out_w,
                                          const float *table_3x256, float *out_nchw, void *stream)
{
    if (!images_hwc || !dst_to_src_2x3 || !table_3x256 || !out_nchw) return CN_ERR_NULL;
    if (H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || pitch_bytes < 3 * W || out_h > 65535 ||
        H > 32767 || W > 32767 || N <= 0 || N > 65535)
        return CN_ERR_SHAPE;
    if (N > 1 && image_stride_bytes < (size_t)pitch_bytes * (size_t)H) return CN_ERR_SHAPE;
    WarpTableArgs a = {};
    a.img = images_hwc; a.H = H; a.W = W; a.pitch = pitch_bytes; a.oh = out_h; a.ow = out_w;
    for (int i = 0; i < 6; ++i) a.m[i] = dst_to_src_2x3[i];
    a.table = table_3x256; a.out = out_nchw;
    a.img_stride = image_stride_bytes;
    a.out_stride = (size_t)3 * out_h * out_w;
    dim3 grid(cn_cdiv(out_w, 128), out_h, N);
    hipLaunchKernelGGL(warp_table_kernel, grid, dim3(128), 0, (hipStream_t)stream, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// ---- the same for a mixed-size batch (KITTI's images come in several sizes): the geometry of image
// blockIdx.z from its cn_image_desc, as warp_normalize_ragged_kernel reads it; warp_table_kernel's
// arithmetic and its table read.
namespace {
__global__ void warp_table_ragged_kernel(const uint8_t *__restrict__ packed, const cn_image_desc *__restrict__ descs,
                                         const float *__restrict__ table, float *__restrict__ out_nchw,
                                         const int oh, const int ow)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    // uniform over the workgroup: one read through the const __restrict__ pointer, kept in scalar registers
    const cn_image_desc d = descs[blockIdx.z];
    if (x >= ow || d.H <= 0 || d.W <= 0) return;
    int v[3];
    const size_t plane = (size_t)oh * ow;
    float *out = out_nchw + (size_t)blockIdx.z * 3 * plane;
    warp_pixel<3>(packed + d.offset, d.H, d.W, (size_t)d.pitch, d.dst_to_src, x, y,
                  row_base(d.dst_to_src, 1, 2, y), row_base(d.dst_to_src, 4, 5, y), v);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane + (size_t)y * ow + x] = table[c * 256 + v[c]];
}
}  // namespace

extern "C" int cn_warp_table_u8_f32_ragged(const uint8_t *packed, const cn_image_desc *descs_dev, int N,
                                           int out_h, int out_w, const float *table_3x256,
                                           float *out_nchw, void *stream)
{
    if (!packed || !descs_dev || !table_3x256 || !out_nchw) return CN_ERR_NULL;
    if (out_h <= 0 || out_w <= 0 || out_h > 65535 || N <= 0 || N > 65535) return CN_ERR_SHAPE;
    dim3 grid(cn_cdiv(out_w, 128), out_h, N);
    hipLaunchKernelGGL(warp_table_ragged_kernel, grid, dim3(128), 0, (hipStream_t)stream, packed, descs_dev,
                       table_3x256, out_nchw, out_h, out_w);
    CN_CHECK_LAUNCH();
    return CN_OK;
}


// ---------------------------------------------------------------------------
// NV12 video frames (what hardware and software decoders deliver: a full-resolution Y plane of H rows,
// then H / 2 rows of interleaved U, V at half resolution, both with the same row pitch) -> dense BGR
// uint8 (H, W, 3), in front of the pre-process above.  Integer BT.601 limited range in 20-bit fixed point,
// the arithmetic OpenCV documents for COLOR_YUV2BGR_NV12; one (U, V) pair serves its 2 x 2 block, no chroma
// interpolation:
//   yy = max(0, Y - 16) * 1220542
//   B = clamp((yy + 2116026 (U - 128)                    + 2^19) >> 20)
//   G = clamp((yy -  409993 (U - 128) - 852492 (V - 128) + 2^19) >> 20)
//   R = clamp((yy + 1673527 (V - 128)                    + 2^19) >> 20)
// (arithmetic shift; |every intermediate| < 2^30).  A pure streaming kernel, 1.5 bytes in and 3 bytes out per
// pixel: a thread converts 2 rows x 16 pixels -- one 16-byte load of each Y row and one of the 8 (U, V)
// pairs under them, three 16-byte stores per row -- where the frame allows it: every row of both buffers
// 16-byte aligned, which on the dense output side needs W % 16 == 0 (the widths video comes in).  Any other
// even W, pitch or pointer takes the same 2 x 16 groups byte by byte, the last group of a row partial.
// ---------------------------------------------------------------------------
namespace {

constexpr int NV12_ROUND = 1 << 19, NV12_SHIFT = 20, NV12_VEC = 16;

// the chroma terms of one (U, V) pair, rounding constant included: c[0..2] for B, G, R
__host__ __device__ inline void nv12_chroma(int U, int V, int c[3])
{
    c[0] = 2116026 * (U - 128) + NV12_ROUND;
    c[1] = -409993 * (U - 128) - 852492 * (V - 128) + NV12_ROUND;
    c[2] = 1673527 * (V - 128) + NV12_ROUND;
}

// one pixel: its luma and its block's chroma terms -> B | G << 8 | R << 16
__host__ __device__ inline uint32_t nv12_pixel(int Y, const int c[3])
{
    // clamp((v) >> 20, 0, 255) written as clamp(v, 0, 2^28 - 1) >> 20, the same integer for every v.  In the
    // first form hipcc (ROCm 7.2, gfx950) selects v_ashr_pk_u8_i32 for two neighbouring channels and ORs its
    // result into the output word as if the upper half of the register were zero; on the MI355X bytes 2 and
    // 3 of the word came out wrong (tests/test_gpu_nv12.py, the 16-byte form, is the guard; the listing and
    // how to re-check it: profiles/nv12_frames_ab.txt section 4).
    const int yy = (Y > 16 ? Y - 16 : 0) * 1220542, top = (256 << NV12_SHIFT) - 1;
    const uint32_t b = (uint32_t)clamp_i(yy + c[0], 0, top) >> NV12_SHIFT;
    const uint32_t g = (uint32_t)clamp_i(yy + c[1], 0, top) >> NV12_SHIFT;
    const uint32_t r = (uint32_t)clamp_i(yy + c[2], 0, top) >> NV12_SHIFT;
    return b | (g << 8) | (r << 16);
}

// `count` (even) pixels of two rows, byte by byte: y0 / y1 the two luma rows, uv the pairs under them
__host__ __device__ inline void nv12_rows_bytes(const uint8_t *y0, const uint8_t *y1, const uint8_t *uv, int count,
                                                uint8_t *o0, uint8_t *o1)
{
    for (int i = 0; i < count; i += 2) {
        int c[3];
        nv12_chroma(uv[i], uv[i + 1], c);
        for (int k = 0; k < 2; ++k) {
            const uint32_t p0 = nv12_pixel(y0[i + k], c), p1 = nv12_pixel(y1[i + k], c);
            for (int ch = 0; ch < 3; ++ch) {
                o0[(i + k) * 3 + ch] = (uint8_t)(p0 >> (8 * ch));
                o1[(i + k) * 3 + ch] = (uint8_t)(p1 >> (8 * ch));
            }
        }
    }
}

struct Nv12Args {
    const uint8_t *nv12;
    uint8_t *out;            // (N, H, W, 3) dense
    int H, W, pitch;
    int groups_x;            // 16-pixel groups of a row (the last one may be partial)
    int groups;              // groups_x * (H / 2): one thread each
    int wide;                // every row of both buffers is 16-byte aligned
    size_t frame_stride;
};

// 16 pixels of one row from their luma word by word and the 8 chroma triples -> the row's 48 output bytes
__host__ __device__ inline void nv12_row16(const uint4 y, const int c[8][3], uint4 o[3])
{
    const uint32_t yw[4] = {y.x, y.y, y.z, y.w};
    uint32_t px[16], w[12];
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = nv12_pixel((int)((yw[i >> 2] >> (8 * (i & 3))) & 255u), c[i >> 1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {      // four 3-byte pixels = three words
        w[3 * q + 0] = px[4 * q] | (px[4 * q + 1] << 24);
        w[3 * q + 1] = (px[4 * q + 1] >> 8) | (px[4 * q + 2] << 16);
        w[3 * q + 2] = (px[4 * q + 2] >> 16) | (px[4 * q + 3] << 8);
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) o[v] = make_uint4(w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]);
}

// 16 pixels of two rows with 16-byte accesses: all five pointers 16-byte aligned
__host__ __device__ inline void nv12_rows_wide(const uint8_t *y0, const uint8_t *y1, const uint8_t *uv, uint8_t *o0,
                                               uint8_t *o1)
{
    const uint4 ya = *reinterpret_cast<const uint4 *>(y0), yb = *reinterpret_cast<const uint4 *>(y1);
    const uint4 cw = *reinterpret_cast<const uint4 *>(uv);
    const uint32_t uvw[4] = {cw.x, cw.y, cw.z, cw.w};
    int c[8][3];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const uint32_t pair = uvw[p >> 1] >> (16 * (p & 1));
        nv12_chroma((int)(pair & 255u), (int)((pair >> 8) & 255u), c[p]);
    }
    uint4 r0[3], r1[3];
    nv12_row16(ya, c, r0);
    nv12_row16(yb, c, r1);
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        reinterpret_cast<uint4 *>(o0)[v] = r0[v];
        reinterpret_cast<uint4 *>(o1)[v] = r1[v];
    }
}

__global__ void __launch_bounds__(256) nv12_to_bgr_kernel(const Nv12Args a)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.groups) return;
    const int yp = g / a.groups_x, x0 = (g - yp * a.groups_x) * NV12_VEC;
    const uint8_t *frame = a.nv12 + (size_t)blockIdx.y * a.frame_stride;
    const uint8_t *y0 = frame + (size_t)(2 * yp) * a.pitch + x0, *y1 = y0 + a.pitch;
    const uint8_t *uv = frame + (size_t)(a.H + yp) * a.pitch + x0;
    uint8_t *o0 = a.out + (((size_t)blockIdx.y * a.H + 2 * yp) * a.W + x0) * 3, *o1 = o0 + (size_t)a.W * 3;
    if (!a.wide) {       // (uniform over the launch; wide implies W % 16 == 0: no partial group)
        nv12_rows_bytes(y0, y1, uv, a.W - x0 < NV12_VEC ? a.W - x0 : NV12_VEC, o0, o1);
        return;
    }
    nv12_rows_wide(y0, y1, uv, o0, o1);
}

// argument rules shared by the device and the host entry (the limits of the warp entry points)
inline int nv12_check(const void *nv12, const void *out, int H, int W, int pitch_bytes)
{
    if (!nv12 || !out) return CN_ERR_NULL;
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1) || pitch_bytes < W || H > 32767 || W > 32767) return CN_ERR_SHAPE;
    return CN_OK;
}

}  // namespace

extern "C" int cn_nv12_to_bgr_u8_batch(const uint8_t *nv12, int N, size_t frame_stride_bytes, int H, int W,
                                       int pitch_bytes, uint8_t *out_bgr_hwc, void *stream)
{
    const int rc = nv12_check(nv12, out_bgr_hwc, H, W, pitch_bytes);
    if (rc != CN_OK) return rc;
    if (N <= 0 || N > 65535) return CN_ERR_SHAPE;
    if (N > 1 && frame_stride_bytes < (size_t)pitch_bytes * (size_t)H * 3 / 2) return CN_ERR_SHAPE;
    Nv12Args a = {};
    a.nv12 = nv12; a.out = out_bgr_hwc; a.H = H; a.W = W; a.pitch = pitch_bytes;
    a.groups_x = cn_cdiv(W, NV12_VEC);
    a.groups = a.groups_x * (H / 2);        // <= 2048 * 16383
    a.frame_stride = frame_stride_bytes;
    a.wide = (((uintptr_t)nv12 | (uintptr_t)out_bgr_hwc | (uintptr_t)pitch_bytes | (uintptr_t)W |
               (N > 1 ? (uintptr_t)frame_stride_bytes : 0)) & 15) == 0;
    dim3 grid(cn_cdiv(a.groups, 256), N);
    hipLaunchKernelGGL(nv12_to_bgr_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// the same for one frame on the HOST (tests, tools, the frame pipe's hand-back routes): nv12_pixel's integers
extern "C" int cn_nv12_to_bgr_u8_host(const uint8_t *nv12, int H, int W, int pitch_bytes, uint8_t *out_bgr_hwc)
{
    const int rc = nv12_check(nv12, out_bgr_hwc, H, W, pitch_bytes);
    if (rc != CN_OK) return rc;
    for (int y = 0; y < H; y += 2) {
        const uint8_t *y0 = nv12 + (size_t)y * pitch_bytes;
        uint8_t *o0 = out_bgr_hwc + (size_t)y * W * 3;
        nv12_rows_bytes(y0, y0 + pitch_bytes, nv12 + (size_t)(H + y / 2) * pitch_bytes, W, o0, o0 + (size_t)W * 3);
    }
    return CN_OK;
}
