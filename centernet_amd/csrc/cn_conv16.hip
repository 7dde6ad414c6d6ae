// cn_conv16.hip -- 3x3 convolution (pad 1, stride 1 or 2) of a 16-channel NHWC map into 16 or
// 32 channels: DLA's level0 / level1 (pose_dla_dcn.py:237-240, `_make_conv_level`, 16 -> 16 at
// full resolution and 16 -> 32 at half), the only layers of the zoo whose channel counts are
// below one MFMA tile of the generic kernels (2-4x of their work was padding).
//
// K = 9 taps x 16 channels = 144 exactly: v_mfma_f32_16x16x4_f32 (M = 16 pixels, N = 16 output
// channels, K = 4), the four lane quarters taking channels 4q..4q+3 of one tap, so ONE
// ds_read_b128 per (tap, 16-pixel block) feeds four MFMAs and 16 consecutive pixels x 64 bytes
// form one contiguous, conflict-free 1 KiB LDS read.  The lane's 36 (x2) weights stay in
// registers.  Persistent workgroups (two per CU) walk 128-pixel row tiles; the 3-row input
// window of the next tile is fetched into registers during the MFMAs of the current one.
// The op is balanced between the matrix pipe and HBM (AI = 36 FLOP/B for 16 -> 16).
#include "cn_internal.h"

namespace {

constexpr int NT = 256;
constexpr int BM = 128;
constexpr int CI = 16;

struct C16Args {
    const float *x, *w;  // x: NHWC pitch in_pitch; w: packed [tap][cout_pad][32]
    const float *scale, *shift;
    float *y;
    int H, W, Ho, Wo, Cout, cout_pad, in_pitch, out_pitch, relu;
};

template <int NBLK, int S>
__global__ __launch_bounds__(NT) void conv16_kernel(const C16Args a, int total_tiles)
{
    constexpr int WX = (BM - 1) * S + 3;           // window columns
    constexpr int NQ = 3 * WX * (CI / 4);          // float4 elements of the window
    constexpr int PQ = (NQ + NT - 1) / NT;         // per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cn_f32x4 *win = reinterpret_cast<cn_f32x4 *>(smem);  // [3][WX][4] float4

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int tpr = a.Wo / BM;

    // weights of this lane: n = nb*16 + l15, input channels 4*lq .. 4*lq+3 of every tap
    float wreg[NBLK][9][4];
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int n = min(nb * 16 + l15, a.cout_pad - 1);
            const cn_f32x4 v = *reinterpret_cast<const cn_f32x4 *>(
                a.w + ((size_t)(t * a.cout_pad + n) * 32 + 4 * lq));
#pragma unroll
            for (int s = 0; s < 4; ++s) wreg[nb][t][s] = (nb * 16 + l15 < a.Cout) ? v[s] : 0.f;
        }
    float sc[NBLK], sf[NBLK];
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb) {
        const int n = nb * 16 + l15;
        sc[nb] = (a.scale && n < a.Cout) ? a.scale[n] : 1.f;
        sf[nb] = (a.shift && n < a.Cout) ? a.shift[n] : 0.f;
        asm volatile("" : "+v"(sc[nb]), "+v"(sf[nb]));  // settle before the tile loop
    }

    cn_f32x4 v[PQ];
    unsigned vmask = 0;
    auto prefetch = [&](int tile) {
        const int xt = tile % tpr;
        const int rowid = tile / tpr;  // b*Ho + oy
        const int b = rowid / a.Ho, oy = rowid - b * a.Ho;
        const int iy0 = oy * S - 1, ix0 = xt * BM * S - 1;
        const char *xb = reinterpret_cast<const char *>(a.x + (size_t)b * a.H * a.W * a.in_pitch);
        unsigned mk = 0;
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int i = tid + u * NT;
            const int row = i / (WX * 4), rem = i - row * (WX * 4);
            const int col = rem >> 2, c4 = rem & 3;
            const int iy = iy0 + row, ix = ix0 + col;
            const bool ok = i < NQ && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const unsigned off = ok ? (unsigned)(((iy * a.W + ix) * a.in_pitch + c4 * 4) * 4) : 0u;
            v[u] = *reinterpret_cast<const cn_f32x4 *>(xb + off);
            mk |= ok ? (1u << u) : 0u;
        }
        vmask = mk;
    };
    auto store_window = [&]() {
        const cn_f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int i = tid + u * NT;
            if (i < NQ) win[i] = ((vmask >> u) & 1u) ? v[u] : z;
        }
    };

    const float *abase[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
        abase[mb] = reinterpret_cast<const float *>(win) + (wave * 32 + mb * 16 + l15) * S * CI + 4 * lq;

    int tile = blockIdx.x;
    if (tile < total_tiles) prefetch(tile);
    for (; tile < total_tiles; tile += gridDim.x) {
        store_window();
        __syncthreads();
        const int next = tile + gridDim.x;
        if (next < total_tiles) prefetch(next);

        cn_f32x4 acc[2][NBLK];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < NBLK; ++nb) acc[mb][nb] = cn_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = ((t / 3) * WX + (t % 3)) * CI;  // compile-time immediate
            cn_f32x4 af[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) af[mb] = *reinterpret_cast<const cn_f32x4 *>(abase[mb] + off);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NBLK; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[mb][s], wreg[nb][t][s],
                                                                           acc[mb][nb], 0, 0, 0);
        }
        // D: col = lane & 15 (cout), rows 4*(lane >> 4) + r (pixels)
        const int xt = tile % tpr;
        const int rowid = tile / tpr;
        float *yb = a.y + ((size_t)rowid * a.Wo + (size_t)xt * BM) * a.out_pitch;
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb) {
            const int n = nb * 16 + l15;
            if (n < a.Cout) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = wave * 32 + mb * 16 + 4 * lq + r;
                        float t = acc[mb][nb][r] * sc[nb] + sf[nb];
                        if (a.relu) t = fmaxf(t, 0.f);
                        yb[(size_t)m * a.out_pitch + n] = t;
                    }
            }
        }
        __syncthreads();
    }
}

template <int NBLK, int S>
int launch_c16(const C16Args &a, int B, hipStream_t st)
{
    constexpr int WX = (BM - 1) * S + 3;
    constexpr size_t lds = (size_t)3 * WX * CI * sizeof(float);
    const long total = (long)B * a.Ho * (a.Wo / BM);
    const int wgs = (int)(total < 512 ? total : 512);  // two resident workgroups per CU
    CN_SET_MAX_LDS_ONCE((conv16_kernel<NBLK, S>), lds);
    hipLaunchKernelGGL((conv16_kernel<NBLK, S>), dim3(wgs), dim3(NT), lds, st, a, (int)total);
    CN_CHECK_LAUNCH();
    return CN_OK;
}


// ---- f32s form (round 3).  The fp32 kernel above is balanced between HBM and the fp32 matrix pipe
// (16 -> 16 at 512^2, B = 32: 77 GFLOP against 157 TFLOP/s = 0.49 ms, measured 0.48); computing the
// products as (high, low) fp16 pairs on v_mfma_f32_16x16x32_f16 -- three instructions of 16 cycles
// per 32-deep K step instead of eight of 32 cycles -- leaves the layer to its 1.07 GB of traffic.
// K = 9 taps x 16 channels is walked as five steps of two taps (the tenth half-step multiplies
// zero weights): lane group q = lane >> 4 of the 16x16x32 instruction holds k = 8q .. 8q+7, i.e.
// tap 2u + (q >> 1), channels 8 (q & 1) .. + 7.  The window sits in LDS as two fp16 planes
// (32 bytes per pixel each: 16 consecutive pixels x {half 0, half 1} = 16 distinct bank groups per
// ds_read_b128 group at stride 1), split ONCE while it is staged (x * x_mul, range word fed there);
// the lane's weights are pre-split registers (40 per 16 output channels).  Output: plain fp32.
typedef _Float16 c16_f16x8 __attribute__((ext_vector_type(8)));

struct C16sArgs {
    const float *x;
    const void *w;       // f32s-packed [tap][cout_pad][128-byte group of 32 channels: 32 high | 32 low halves]
    const float *scale, *shift;
    float *y;
    int H, W, Ho, Wo, Cout, cout_pad, in_pitch, out_pitch, relu;
    float x_mul;
    uint32_t *range;
};

template <int NBLK, int S>
__global__ __launch_bounds__(NT, 2) void conv16s_kernel(const C16sArgs a, int total_tiles)
{
    constexpr int WX = (BM - 1) * S + 3;           // window columns
    constexpr int NQ = 3 * WX * (CI / 4);          // float4 elements of the window
    constexpr int PQ = (NQ + NT - 1) / NT;         // per thread
    constexpr int PLANE = 3 * WX * 32;             // bytes of one fp16 plane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *win_hi = smem, *win_lo = smem + PLANE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int tpr = a.Wo / BM;
    const float x_mul = a.x_mul;

    // weights of this lane: n = nb*16 + l15; step u: tap 2u + (lq >> 1), channels 8 (lq & 1) ..
    c16_f16x8 wh[NBLK][5], wl[NBLK][5];
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int t = 2 * u + (lq >> 1);
            const int n = min(nb * 16 + l15, a.cout_pad - 1);
            const char *g = reinterpret_cast<const char *>(a.w) + ((size_t)(min(t, 8) * a.cout_pad + n)) * 128 + 16 * (lq & 1);
            const bool ok = t < 9 && nb * 16 + l15 < a.Cout;
            const c16_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            wh[nb][u] = ok ? *reinterpret_cast<const c16_f16x8 *>(g) : z;
            wl[nb][u] = ok ? *reinterpret_cast<const c16_f16x8 *>(g + 64) : z;
        }
    float sc[NBLK], sf[NBLK];
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb) {
        const int n = nb * 16 + l15;
        sc[nb] = (a.scale && n < a.Cout) ? a.scale[n] : 1.f;
        sf[nb] = (a.shift && n < a.Cout) ? a.shift[n] : 0.f;
        asm volatile("" : "+v"(sc[nb]), "+v"(sf[nb]));  // settle before the tile loop
    }

    cn_f32x4 v[PQ];
    unsigned vmask = 0;
    float rng_in = 0.f;
    auto prefetch = [&](int tile) {
        const int xt = tile % tpr;
        const int rowid = tile / tpr;  // b*Ho + oy
        const int b = rowid / a.Ho, oy = rowid - b * a.Ho;
        const int iy0 = oy * S - 1, ix0 = xt * BM * S - 1;
        const char *xb = reinterpret_cast<const char *>(a.x + (size_t)b * a.H * a.W * a.in_pitch);
        unsigned mk = 0;
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int i = tid + u * NT;
            const int row = i / (WX * 4), rem = i - row * (WX * 4);
            const int col = rem >> 2, c4 = rem & 3;
            const int iy = iy0 + row, ix = ix0 + col;
            const bool ok = i < NQ && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const unsigned off = ok ? (unsigned)(((iy * a.W + ix) * a.in_pitch + c4 * 4) * 4) : 0u;
            v[u] = *reinterpret_cast<const cn_f32x4 *>(xb + off);
            mk |= ok ? (1u << u) : 0u;
        }
        vmask = mk;
    };
    auto store_window = [&]() {
        const cn_f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int i = tid + u * NT;
            if (i < NQ) {
                const cn_f32x4 xs = ((vmask >> u) & 1u) ? v[u] * x_mul : z;   // real -> stored units
                cn_rng_upd4(rng_in, xs);
                cn_f16x4v hi, lo;
                cn_split4(xs, hi, lo);
                // element i = (pixel i >> 2, channel quad i & 3): 8 bytes in each plane
                *reinterpret_cast<cn_f16x4v *>(win_hi + (size_t)i * 8) = hi;
                *reinterpret_cast<cn_f16x4v *>(win_lo + (size_t)i * 8) = lo;
            }
        }
    };

    // A fragment of (16-pixel block mb, step u): pixel + tap offset, 16 bytes of half (lq & 1)
    unsigned aoff[2][5];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int t = min(2 * u + (lq >> 1), 8);   // (the tenth half-step re-reads tap 8: its weights are zero)
            aoff[mb][u] = (unsigned)(((wave * 32 + mb * 16 + l15) * S + (t / 3) * WX + (t % 3)) * 32 + 16 * (lq & 1));
        }

    int tile = blockIdx.x;
    if (tile < total_tiles) prefetch(tile);
    for (; tile < total_tiles; tile += gridDim.x) {
        store_window();
        __syncthreads();
        const int next = tile + gridDim.x;
        if (next < total_tiles) prefetch(next);

        cn_f32x4 acc[2][NBLK];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < NBLK; ++nb) acc[mb][nb] = cn_f32x4{0.f, 0.f, 0.f, 0.f};
        c16_f16x8 ah[2][5], al[2][5];
#pragma unroll
        for (int u = 0; u < 5; ++u)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                ah[mb][u] = *reinterpret_cast<const c16_f16x8 *>(win_hi + aoff[mb][u]);
                al[mb][u] = *reinterpret_cast<const c16_f16x8 *>(win_lo + aoff[mb][u]);
            }
        // every fragment is in registers before the first MFMA (operand hazard note, cn_conv.hip)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 5; ++u)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < NBLK; ++nb) {
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mb][u], wh[nb][u], acc[mb][nb], 0, 0, 0);
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mb][u], wl[nb][u], acc[mb][nb], 0, 0, 0);
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mb][u], wh[nb][u], acc[mb][nb], 0, 0, 0);
                }
        // D: col = lane & 15 (cout), rows 4*(lane >> 4) + r (pixels)
        const int xt = tile % tpr;
        const int rowid = tile / tpr;
        float *yb = a.y + ((size_t)rowid * a.Wo + (size_t)xt * BM) * a.out_pitch;
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb) {
            const int n = nb * 16 + l15;
            if (n < a.Cout) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = wave * 32 + mb * 16 + 4 * lq + r;
                        float t = acc[mb][nb][r] * sc[nb] + sf[nb];
                        if (a.relu) t = fmaxf(t, 0.f);
                        yb[(size_t)m * a.out_pitch + n] = t;
                    }
            }
        }
        __syncthreads();
    }
    if (a.range) cn_rng_commit(a.range, 1, rng_in);
}

template <int NBLK, int S>
int launch_c16s(const C16sArgs &a, int B, hipStream_t st)
{
    constexpr int WX = (BM - 1) * S + 3;
    constexpr size_t lds = (size_t)2 * 3 * WX * 32;
    const long total = (long)B * a.Ho * (a.Wo / BM);
    const int wgs = (int)(total < 512 ? total : 512);  // two resident workgroups per CU
    CN_SET_MAX_LDS_ONCE((conv16s_kernel<NBLK, S>), lds);
    hipLaunchKernelGGL((conv16s_kernel<NBLK, S>), dim3(wgs), dim3(NT), lds, st, a, (int)total);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// ---- half form (CN_DTYPE_F16 tensors on both sides): the simpler sibling of the f32s form.  Same geometry
// (256 threads, persistent workgroups over 128-pixel row tiles, 3-row window in LDS, next window fetched into
// registers during the MFMAs, K = five steps of two taps), but ONE fp16 plane of 32 bytes per pixel -- staged
// with plain 16-byte loads and 16-byte LDS stores, element i of the window at byte 16 i: 4 staging registers
// of 16 bytes per thread at stride 1, 7 at stride 2 -- and one MFMA per (step, pixel block, channel block).
// Operand roles are swapped against the two kernels above: the WEIGHTS are the A operand (M = 16 output
// channels) and the pixels the B operand (N = 16 pixels), so D holds, per lane, channels 4 (lane >> 4) .. + 3 of
// pixel lane & 15: a lane stores 8 bytes and a 16-pixel block's 64 lanes cover 512 contiguous bytes at
// Cout = 16 (the other roles would give sixteen scattered 2-byte stores).  The weight is the packed weight of
// the general half kernels ([tap][cout_pad][64 halves], channels 16 .. 63 zero): the first 32 bytes of a row.
// Stride 2: the 64-byte pixel stride gives two-way bank conflicts on the fragment reads; accepted (one plane;
// DESIGN 3.3b has the measurement).  Barriers: __syncthreads() only.
struct C16hArgs {
    const _Float16 *x;
    const void *w;
    const float *scale, *shift;
    _Float16 *y;
    int H, W, Ho, Wo, Cout, cout_pad, in_pitch, out_pitch, relu, vec_out;
};

template <int NBLK, int S>
__global__ __launch_bounds__(NT, 2) void conv16h_kernel(const C16hArgs a, int total_tiles)
{
    constexpr int WX = (BM - 1) * S + 3;           // window columns
    constexpr int NQ = 3 * WX * 2;                 // 16-byte elements of the window: (row, column, channel half)
    constexpr int PQ = (NQ + NT - 1) / NT;         // per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int tpr = a.Wo / BM;

    // A operand: output channel n = nb*16 + l15; step u: tap 2u + (lq >> 1), input channels 8 (lq & 1) .. + 7
    c16_f16x8 wf[NBLK][5];
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int t = 2 * u + (lq >> 1);
            const int n = min(nb * 16 + l15, a.cout_pad - 1);
            const char *g = reinterpret_cast<const char *>(a.w) + ((size_t)(min(t, 8) * a.cout_pad + n)) * 128 + 16 * (lq & 1);
            const bool ok = t < 9 && nb * 16 + l15 < a.Cout;
            const c16_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            wf[nb][u] = ok ? *reinterpret_cast<const c16_f16x8 *>(g) : z;
        }
    // D rows of this lane: channels nb*16 + 4 lq + r
    float sc[NBLK][4], sf[NBLK][4];
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nb * 16 + 4 * lq + r;
            sc[nb][r] = (a.scale && n < a.Cout) ? a.scale[n] : 1.f;
            sf[nb][r] = (a.shift && n < a.Cout) ? a.shift[n] : 0.f;
            asm volatile("" : "+v"(sc[nb][r]), "+v"(sf[nb][r]));  // settle before the tile loop
        }

    c16_f16x8 v[PQ];
    unsigned vmask = 0;
    auto prefetch = [&](int tile) {
        const int xt = tile % tpr;
        const int rowid = tile / tpr;  // b*Ho + oy
        const int b = rowid / a.Ho, oy = rowid - b * a.Ho;
        const int iy0 = oy * S - 1, ix0 = xt * BM * S - 1;
        const char *xb = reinterpret_cast<const char *>(a.x + (size_t)b * a.H * a.W * a.in_pitch);
        unsigned mk = 0;
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int i = tid + u * NT;
            const int row = i / (WX * 2), rem = i - row * (WX * 2);
            const int col = rem >> 1, h = rem & 1;
            const int iy = iy0 + row, ix = ix0 + col;
            const bool ok = i < NQ && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const unsigned off = ok ? (unsigned)(((iy * a.W + ix) * a.in_pitch + h * 8) * 2) : 0u;
            v[u] = *reinterpret_cast<const c16_f16x8 *>(xb + off);
            mk |= ok ? (1u << u) : 0u;
        }
        vmask = mk;
    };
    auto store_window = [&]() {
        const c16_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < PQ; ++u) {
            const int i = tid + u * NT;
            if (i < NQ) *reinterpret_cast<c16_f16x8 *>(smem + (size_t)i * 16) = ((vmask >> u) & 1u) ? v[u] : z;
        }
    };

    // B fragment of (16-pixel block mb, step u): pixel + tap offset, 16 bytes of channel half (lq & 1)
    unsigned boff[2][5];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int t = min(2 * u + (lq >> 1), 8);   // (the tenth half-step re-reads tap 8: its weights are zero)
            boff[mb][u] = (unsigned)(((wave * 32 + mb * 16 + l15) * S + (t / 3) * WX + (t % 3)) * 32 + 16 * (lq & 1));
        }

    int tile = blockIdx.x;
    if (tile < total_tiles) prefetch(tile);
    for (; tile < total_tiles; tile += gridDim.x) {
        store_window();
        __syncthreads();
        const int next = tile + gridDim.x;
        if (next < total_tiles) prefetch(next);

        cn_f32x4 acc[2][NBLK];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < NBLK; ++nb) acc[mb][nb] = cn_f32x4{0.f, 0.f, 0.f, 0.f};
        c16_f16x8 bf[2][5];
#pragma unroll
        for (int u = 0; u < 5; ++u)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) bf[mb][u] = *reinterpret_cast<const c16_f16x8 *>(smem + boff[mb][u]);
        // every fragment is in registers before the first MFMA (operand hazard note, cn_conv.hip)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 5; ++u)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < NBLK; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nb][u], bf[mb][u], acc[mb][nb], 0, 0, 0);
        // D: col = lane & 15 (pixel), rows 4*(lane >> 4) + r (output channels): fp32 epilogue, one rounding
        const int xt = tile % tpr;
        const int rowid = tile / tpr;
        _Float16 *yb = a.y + ((size_t)rowid * a.Wo + (size_t)xt * BM) * a.out_pitch;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            _Float16 *yp = yb + (size_t)(wave * 32 + mb * 16 + l15) * a.out_pitch;
#pragma unroll
            for (int nb = 0; nb < NBLK; ++nb) {
                const int n0 = nb * 16 + 4 * lq;
                cn_f16x4v o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = acc[mb][nb][r] * sc[nb][r] + sf[nb][r];
                    if (a.relu) t = fmaxf(t, 0.f);
                    o[r] = (_Float16)t;
                }
                if (a.vec_out && n0 + 3 < a.Cout)
                    *reinterpret_cast<cn_f16x4v *>(yp + n0) = o;
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < a.Cout) yp[n0 + r] = o[r];
            }
        }
        __syncthreads();
    }
}

template <int NBLK, int S>
int launch_c16h(const C16hArgs &a, int B, hipStream_t st)
{
    constexpr int WX = (BM - 1) * S + 3;
    constexpr size_t lds = (size_t)3 * WX * 32;    // 12 480 bytes at stride 1, 24 672 at stride 2
    const long total = (long)B * a.Ho * (a.Wo / BM);
    const int wgs = (int)(total < 512 ? total : 512);  // two resident workgroups per CU
    CN_SET_MAX_LDS_ONCE((conv16h_kernel<NBLK, S>), lds);
    hipLaunchKernelGGL((conv16h_kernel<NBLK, S>), dim3(wgs), dim3(NT), lds, st, a, (int)total);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace

// Is the layer of this file's form?  (the caller has checked: 3x3 / pad 1 / dilation 1, NHWC both sides, no
// residual; fp32 tensors, or f32s arithmetic with plain input and plain output)
bool cn_conv16_takes(const ConvCall &c)
{
    if (c.Cin != CI || c.Cout > 32 || (c.stride != 1 && c.stride != 2) || c.Wo % BM != 0 || (c.in_pitch & 3))
        return false;
    if (c.Ho != (c.H + 2 - 3) / c.stride + 1 || c.Wo != (c.W + 2 - 3) / c.stride + 1) return false;
    if ((long)c.H * c.W * c.in_pitch >= (1L << 29)) return false;  // 32-bit byte offsets per image
    // f32s, stride 2 (level1) was measured slower in this form than on the fp32 kernel (0.476 vs 0.245 ms:
    // a 257-column window = 52 staging registers next to 80 fragment + 80 weight registers, 2-way
    // bank conflicts at the 64-byte pixel stride): not built
    return c.dtype == CN_DTYPE_F32 || c.stride == 1;
}

template <typename Args>
static Args c16_args(const ConvCall &c)
{
    Args a;
    a.x = (const float *)c.x; a.scale = c.scale; a.shift = c.shift; a.y = (float *)c.y;
    a.H = c.H; a.W = c.W; a.Ho = c.Ho; a.Wo = c.Wo; a.Cout = c.Cout; a.cout_pad = c.cout_pad;
    a.in_pitch = c.in_pitch; a.out_pitch = c.out_pitch; a.relu = c.relu;
    return a;
}

int cn_conv3x3_c16(const ConvCall &c, hipStream_t st)
{
    if (!cn_conv16_takes(c)) return CN_ERR_UNSUPPORTED;
    C16Args a = c16_args<C16Args>(c);
    a.w = (const float *)c.w;
    if (c.Cout <= 16)
        return c.stride == 1 ? launch_c16<1, 1>(a, c.B, st) : launch_c16<1, 2>(a, c.B, st);
    return c.stride == 1 ? launch_c16<2, 1>(a, c.B, st) : launch_c16<2, 2>(a, c.B, st);
}

// f32s form: plain fp32 input (split while it is staged: ctl->x_mul, range word side 1), f32s-packed
// weight (cn_pack_conv_weight, CN_DTYPE_F32S: 128-byte groups, channels 16..31 zero), plain fp32
// output.  Stride 1 only (cn_conv16_takes).
int cn_conv3x3_c16s(const ConvCall &c, hipStream_t st)
{
    if (!cn_conv16_takes(c)) return CN_ERR_UNSUPPORTED;
    C16sArgs a = c16_args<C16sArgs>(c);
    a.w = c.w;
    a.x_mul = (c.ctl && c.ctl->x_mul != 0.f) ? c.ctl->x_mul : 1.f;
    a.range = c.ctl ? c.ctl->range : nullptr;
    return c.Cout <= 16 ? launch_c16s<1, 1>(a, c.B, st) : launch_c16s<2, 1>(a, c.B, st);
}

// Half form: is the layer one it runs?  (the caller has checked: CN_DTYPE_F16, 3x3 / pad 1 / dilation 1, plain
// geometry, NHWC both sides, no residual, no K split)
bool cn_conv16h_takes(const ConvCall &c)
{
    if (c.dtype != CN_DTYPE_F16 || c.out_plain || c.Cin != CI || c.Cout > 32 || (c.stride != 1 && c.stride != 2) || c.Wo % BM != 0)
        return false;
    if ((c.in_pitch & 7) || (c.out_pitch & 3)) return false;   // 16-byte loads; 8-byte stores where y is aligned
    if (c.Ho != (c.H + 2 - 3) / c.stride + 1 || c.Wo != (c.W + 2 - 3) / c.stride + 1) return false;
    return (long)c.H * c.W * c.in_pitch < (1L << 30);          // 32-bit byte offsets per image
}

// half input, the general half kernels' packed weight (cn_pack_conv_weight, CN_DTYPE_F16), fp32 scale / shift,
// half output at out_pitch
int cn_conv3x3_c16h(const ConvCall &c, hipStream_t st)
{
    if (!cn_conv16h_takes(c) || c.residual || c.ksplit != 1) return CN_ERR_UNSUPPORTED;
    C16hArgs a;
    a.x = (const _Float16 *)c.x; a.w = c.w; a.scale = c.scale; a.shift = c.shift; a.y = (_Float16 *)c.y;
    a.H = c.H; a.W = c.W; a.Ho = c.Ho; a.Wo = c.Wo; a.Cout = c.Cout; a.cout_pad = c.cout_pad;
    a.in_pitch = c.in_pitch; a.out_pitch = c.out_pitch; a.relu = c.relu; a.vec_out = c.vec_out;
    if (c.Cout <= 16)
        return c.stride == 1 ? launch_c16h<1, 1>(a, c.B, st) : launch_c16h<1, 2>(a, c.B, st);
    return c.stride == 1 ? launch_c16h<2, 1>(a, c.B, st) : launch_c16h<2, 2>(a, c.B, st);
}
