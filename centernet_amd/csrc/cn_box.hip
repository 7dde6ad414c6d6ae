// cn_box.hip -- the pre-process of a tile pyramid (run_tiles with levels):
// cn_tile_box_normalize_u8_f32, one launch per chunk of the tile batch.
//
// Tile n is a (oh, ow) window at (y0, x0) of level l of its frame, the frame box-filtered by f = 1 << l.  The
// filter is DIRECT from the frame (f x f source pixels per output pixel, one rounding, a zero border with the
// divisor kept at f * f), not a cascade of half-size steps, and no level image is stored:
//   v[c] = (sum of the f x f source bytes of channel c + (f * f >> 1)) >> (2 * l)
//   out  = float32(((double)v[c] / 255.0 - mean[c]) / std[c])            (warp_normalize_kernel's line)
// image.tile_box_normalize is the host restatement these kernels are tested against bit for bit.
//
// This is byte streaming: a level-l tile reads oh * ow * 4^l * 3 bytes and writes oh * ow * 12.  Every thread
// owns 16 source pixels of a source row -- 48 contiguous bytes, three 16-byte loads when the address is
// 16-byte aligned and the 16 pixels lie inside the frame, 48 checked byte loads otherwise (frame edges, odd
// pitch / offset / origin) -- for the f source rows of ONE output row, i.e. 16 >> l output pixels whose partial
// sums stay in registers.  Neighbouring lanes own neighbouring 48-byte pieces, so a wave reads 3 KiB of a
// source row per step.  A uint8 level has 256 values per channel: each workgroup forms the 3 x 256 normalised
// values once in LDS (the float64 division is the dearest instruction sequence here) and looks them up.
#include "cn_common.h"

// as cn_pre.hip: the normalisation is written with plain operators under an explicit contract(off)
#pragma clang fp contract(off)

namespace {

constexpr int BOX_THREADS = 256, BOX_SRC = 16;     // source pixels per thread and source row

struct BoxArgs {
    int oh, ow;
    double mean[3], stdv[3];
    float *out;          // (N, 3, oh, ow)
};

// the 48 bytes of source pixels [X, X + 16) of row sy as 12 little-endian words; outside the frame: 0
__device__ __forceinline__ void box_load(const uint8_t *__restrict__ img, int H, int W, size_t pitch, int sy, int X,
                                         uint32_t w[12])
{
    if (sy < 0 || sy >= H || X >= W || X + BOX_SRC <= 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = 0u;
        return;
    }
    const uint8_t *row = img + (size_t)sy * pitch;
    if (X >= 0 && X + BOX_SRC <= W && (reinterpret_cast<uintptr_t>(row + (ptrdiff_t)X * 3) & 15u) == 0) {
        const uint4 *p = reinterpret_cast<const uint4 *>(row + (ptrdiff_t)X * 3);
        const uint4 a = p[0], b = p[1], c = p[2];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
        return;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k] = 0u;
#pragma unroll
    for (int p = 0; p < BOX_SRC; ++p) {
        const int sx = X + p;
        if (sx < 0 || sx >= W) continue;
        const uint8_t *s = row + (size_t)sx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int j = p * 3 + c;
            w[j >> 2] |= (uint32_t)s[c] << (8 * (j & 3));
        }
    }
}

template <int LEVEL>
__device__ __forceinline__ void box_tile(const uint8_t *__restrict__ img, const cn_tile_box_desc &d, const BoxArgs &a,
                                         const float *__restrict__ table, float *__restrict__ out, int idx)
{
    constexpr int F = 1 << LEVEL, G = BOX_SRC >> LEVEL;      // output pixels per thread
    const int nk = (a.ow + G - 1) / G;
    const int y = idx / nk, k = idx - y * nk;
    if (y >= a.oh) return;
    const int xo = k * G;
    int acc[G * 3];
#pragma unroll
    for (int e = 0; e < G * 3; ++e) acc[e] = 0;
    const int X = (d.x0 + xo) * F, Y = (d.y0 + y) * F;
    for (int dy = 0; dy < F; ++dy) {
        uint32_t w[12];
        box_load(img, d.H, d.W, (size_t)d.pitch, Y + dy, X, w);
#pragma unroll
        for (int j = 0; j < BOX_SRC * 3; ++j)
            acc[(j / 3 / F) * 3 + j % 3] += (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
    const size_t plane = (size_t)a.oh * a.ow;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = table[c * 256 + ((acc[g * 3 + c] + (F * F >> 1)) >> (2 * LEVEL))];
        float *o = out + c * plane + (size_t)y * a.ow + xo;
        if (G >= 4 && xo + G <= a.ow && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
#pragma unroll
            for (int g = 0; g + 3 < G; g += 4)
                *reinterpret_cast<cn_f32x4 *>(o + g) = cn_f32x4{v[g], v[g + 1], v[g + 2], v[g + 3]};
        } else {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (xo + g < a.ow) o[g] = v[g];
        }
    }
}

// grid (work items of a level-3 tile / BOX_THREADS, N): a tile of a finer level has fewer items, its surplus
// workgroups leave at once.  The descriptor is uniform over the workgroup.
__global__ __launch_bounds__(BOX_THREADS) void tile_box_normalize_kernel(const uint8_t *__restrict__ packed,
                                                                         const cn_tile_box_desc *__restrict__ descs,
                                                                         const BoxArgs a)
{
    __shared__ float table[3 * 256];
    const cn_tile_box_desc d = descs[blockIdx.y];
    if (d.H <= 0 || d.W <= 0 || d.level < 0 || d.level > 3) return;
    const int G = BOX_SRC >> d.level;
    const int items = a.oh * ((a.ow + G - 1) / G);
    if ((int)(blockIdx.x * BOX_THREADS) >= items) return;
    for (int e = threadIdx.x; e < 3 * 256; e += BOX_THREADS) {
        const int c = e >> 8;
        const double n = ((double)(e & 255) / 255.0 - a.mean[c]) / a.stdv[c];
        table[e] = (float)n;
    }
    __syncthreads();
    const int idx = blockIdx.x * BOX_THREADS + threadIdx.x;
    if (idx >= items) return;
    const uint8_t *img = packed + d.offset;
    float *out = a.out + (size_t)blockIdx.y * 3 * a.oh * a.ow;
    switch (d.level) {
    case 0: box_tile<0>(img, d, a, table, out, idx); break;
    case 1: box_tile<1>(img, d, a, table, out, idx); break;
    case 2: box_tile<2>(img, d, a, table, out, idx); break;
    default: box_tile<3>(img, d, a, table, out, idx); break;
    }
}

}  // namespace

extern "C" int cn_tile_box_normalize_u8_f32(const uint8_t *packed, const cn_tile_box_desc *descs_dev, int N, int out_h,
                                            int out_w, const float *mean3, const float *std3, float *out_nchw,
                                            void *stream)
{
    if (!packed || !descs_dev || !mean3 || !std3 || !out_nchw) return CN_ERR_NULL;
    if (out_h <= 0 || out_w <= 0 || out_h > 65535 || out_w > 65535 || N <= 0 || N > 65535) return CN_ERR_SHAPE;
    BoxArgs a = {};
    a.oh = out_h; a.ow = out_w;
    for (int c = 0; c < 3; ++c) {
        if (std3[c] == 0.f) return CN_ERR_SHAPE;
        a.mean[c] = (double)mean3[c];
        a.stdv[c] = (double)std3[c];
    }
    a.out = out_nchw;
    const long long items = (long long)out_h * cn_cdiv(out_w, BOX_SRC >> 3);      // the coarsest level's
    if (items > 0x7fffffffLL - BOX_THREADS) return CN_ERR_SHAPE;                   // (the kernel counts them in int)
    dim3 grid((unsigned)((items + BOX_THREADS - 1) / BOX_THREADS), N);
    hipLaunchKernelGGL(tile_box_normalize_kernel, grid, dim3(BOX_THREADS), 0, (hipStream_t)stream, packed, descs_dev,
                       a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
