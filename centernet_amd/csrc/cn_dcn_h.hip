// cn_dcn_h.hip -- fused modulated deformable convolution (DCNv2) forward, fp16 compute mode (CN_DTYPE_F16),
// with the input staged as an LDS WINDOW: the half analogue of the register-sampling form (cn_dcn2.hip), on the
// geometry of cn_dcn_window.h -- 8 x 16 pixel tiles, +-3 px reach inside a 16 x 24 pixel window, the far path
// for samples beyond it, the XCD-aware tile order (dcnw_tile).
//
// A 64-channel chunk of halves is 128 bytes per window pixel, exactly the 32 floats of the f32s window, so the
// window layout is cn_dcn2.hip's (144-byte pixels, 3584-byte rows: bank-conflict free for undisplaced samples)
// with K = 64 per window instead of 32: half the window swaps and half the input bytes per output.
//   * lane (l31, h) of a wave is output pixel 32 * wave + l31 and channels 16 kk + 8 h .. + 7 of the chunk for
//     the four K steps kk: ONE 16-byte read per corner and K step (16 ds_read_b128 per sample and chunk);
//   * arithmetic: the four corners are read as halves, blended and multiplied by the mask in fp32, rounded ONCE
//     to fp16 and used directly as the 32x32x16 MFMA's B operand -- no A tile, no column buffer; fp32 accumulate;
//   * the weights are the MFMA's A operand, streamed from the packed fp16 weight (cn_pack_conv_weight,
//     [tap][cout_pad][cin_pad64] halves: a lane's four 16-byte loads of a K chunk lie in one 128-byte line of its
//     output channel's row); L2-resident, as in the halo kernel;
//   * the epilogue is fp32, y = relu?((acc + bias) * scale + shift), staged per wave and stored as whole 16-byte
//     groups of 8 halves: one rounding at the store.
// No K split in this form: grids too small for the chip go to the gather form and its tap split (dcn_route).
// Every barrier is a __syncthreads() with nothing in flight across it (the window is filled through registers,
// not by LDS-DMA), so the raw-barrier audit does not apply.
#include "cn_dcn_window.h"

namespace {

struct DcnHArgs {
    const _Float16 *x;         // (B, H, W, Cin) halves
    const _Float16 *w;         // packed [tap][cout_pad][cin_pad] halves, cin_pad = Cin (a multiple of 64)
    const float *bias, *scale, *shift, *om;
    _Float16 *y;
    int B, H, W, Cin, Cout, om_pitch, mask_sigmoid, relu;
    int cout_pad, nchunk, tiles_x, tiles_y, out_pitch;
    const cn_rect *rects;      // canvas batches: the images' own origins (DcnCall), or null
    int rect_shift;
};

__device__ __forceinline__ float dh_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }   // the gather form's

constexpr int H_NT = 256;
constexpr int H_WROW = DCNW_PIXB / 4 + 4;        // 36 floats per window pixel (128 B + 16 B pad)
constexpr int H_WLINE = DCNW_WX * H_WROW + 32;   // 896 floats = 3584 bytes per window row (see cn_dcn2.hip R_WLINE)
constexpr size_t H_WBYTES = (size_t)DCNW_WY * H_WLINE * 4;              // 57344
constexpr size_t H_LDS = H_WBYTES + (size_t)9 * DCNW_PM * 16;           // + 18432 = 75776: two workgroups per CU

__device__ __forceinline__ cn_f32x4 dh_blend(const cn_f32x4 r1, const cn_f32x4 r2, const cn_f32x4 r3, const cn_f32x4 r4,
                                             float w1, float w2, float w3, float w4, float mk)
{
    // corners as halves -> fp32 blend (dcn_v2_im2col_cuda.cu:43-45) -> mask (:174) -> one rounding to fp16
    const dcnw_f16x8 h1 = __builtin_bit_cast(dcnw_f16x8, r1), h2 = __builtin_bit_cast(dcnw_f16x8, r2);
    const dcnw_f16x8 h3 = __builtin_bit_cast(dcnw_f16x8, r3), h4 = __builtin_bit_cast(dcnw_f16x8, r4);
    dcnw_f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float s = (float)h1[e] * w1 + (float)h2[e] * w2 + (float)h3[e] * w3 + (float)h4[e] * w4;
        o[e] = (_Float16)(s * mk);
    }
    return __builtin_bit_cast(cn_f32x4, o);
}

template <int BN>
__global__ __launch_bounds__(H_NT, 2) void dcn_half_kernel(const DcnHArgs a)
{
    constexpr int NB = BN / 32;
    constexpr int LDC = BN + 4;
    static_assert((size_t)4 * 32 * LDC * 4 <= H_LDS, "epilogue staging");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *Win = reinterpret_cast<float *>(smem);
    cn_i32x4 *Rec = reinterpret_cast<cn_i32x4 *>(smem + H_WBYTES);         // [9][DCNW_PM]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int H = a.H, W = a.W;
    const DcnwTile tile = dcnw_tile(a.tiles_x, a.tiles_y);
    const int b = tile.b, ty0 = tile.ty0, tx0 = tile.tx0, wy0 = tile.wy0, wx0 = tile.wx0;
    const int n0 = blockIdx.y * BN;
    const cn_f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const unsigned pix_bytes = (unsigned)a.Cin * 2u;
    const unsigned img_base = (unsigned)(b * H) * (unsigned)W;
    const dcnw_glb_char *xg = (const dcnw_glb_char *)a.x;
    const dcnw_lds_char *win_lds = (const dcnw_lds_char *)smem;

    // ---- window of one 64-channel chunk: 3072 16-byte pieces, 12 per thread; 8 lanes = one pixel's 128 bytes;
    // pixels outside the image are zeros
    constexpr int NP = DCNW_WPIX * 8 / H_NT;
    cn_f32x4 rw[NP];
    unsigned okbits = 0u;
    auto fill_load = [&](int chunk) {
        okbits = 0u;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = p * H_NT + tid;
            const int wp = i >> 3, q = i & 7;
            const int wy = wp / DCNW_WX, wx = wp - wy * DCNW_WX;
            const int iy = wy0 + wy, ix = wx0 + wx;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            okbits |= ok ? (1u << p) : 0u;
            const unsigned off = ok ? (img_base + (unsigned)(iy * W + ix)) * pix_bytes + (unsigned)chunk * 128u + 16u * q : 0u;
            rw[p] = *reinterpret_cast<const dcnw_glb_f32x4 *>(xg + off);
        }
    };
    auto fill_store = [&]() {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = p * H_NT + tid;
            const cn_f32x4 v = ((okbits >> p) & 1u) ? rw[p] : zero4;
            const int wp = i >> 3, wy = wp / DCNW_WX;
            *reinterpret_cast<cn_f32x4 *>(Win + wy * H_WLINE + (wp - wy * DCNW_WX) * H_WROW + (i & 7) * 4) = v;
        }
    };

    // ---- prologue: offsets / masks of the tile (all loads requested before the first record is formed), the
    // window of chunk 0 behind them, then the sampling records of all nine taps (dcn_v2_im2col_cuda.cu:151-176)
    {
        constexpr int NR = (9 * DCNW_PM + H_NT - 1) / H_NT;   // 5 (the last trip half full)
        float off_h[NR], off_w[NR], mkv[NR];
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int i = min(p * H_NT + tid, 9 * DCNW_PM - 1);
            const int tap = i / DCNW_PM, m = i - tap * DCNW_PM;
            const int oy = ty0 + (m >> 4), ox = tx0 + (m & 15);
            const float *om = a.om + (size_t)((b * H + oy) * W + ox) * a.om_pitch;
            off_h[p] = om[2 * tap];
            off_w[p] = om[2 * tap + 1];
            mkv[p] = om[18 + tap];
        }
        fill_load(0);
        // canvas batches: positions relative to the image's own origin (y0, x0), so that the fractions round as in
        // the image's own forward; (0, 0) otherwise -- the arithmetic it always was
        int y0 = 0, x0 = 0;
        if (a.rects) {
            const cn_rect rc = a.rects[b];
            y0 = min(max(rc.y0 >> a.rect_shift, 0), a.H);
            x0 = min(max(rc.x0 >> a.rect_shift, 0), a.W);
        }
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int i = p * H_NT + tid;
            const int tap = i / DCNW_PM, m = i - tap * DCNW_PM;
            const int oy = ty0 + (m >> 4), ox = tx0 + (m & 15);
            float mk = mkv[p];
            if (a.mask_sigmoid) mk = dh_sigmoid(mk);    // dcn_v2.py:67
            const int ki = tap / 3, kj = tap - ki * 3;
            const float h_im = (float)(oy - y0 - 1 + ki) + off_h[p];
            const float w_im = (float)(ox - x0 - 1 + kj) + off_w[p];
            cn_i32x4 rec = {0, 0, 0, 0};
            if (h_im > -1.f - (float)y0 && w_im > -1.f - (float)x0 && h_im < (float)(H - y0) &&
                w_im < (float)(W - x0)) {   // :165
                const float hf = floorf(h_im), wf = floorf(w_im);
                const int yl = (int)hf + y0, xl = (int)wf + x0;
                rec[0] = __float_as_int(h_im - hf);
                rec[1] = __float_as_int(w_im - wf);
                rec[2] = __float_as_int(mk);
                rec[3] = (yl & 0xffff) | (int)((uint32_t)(xl & 0xffff) << 16);
            } else {
                rec[3] = (oy & 0xffff) | (int)((uint32_t)(ox & 0xffff) << 16);   // mask = 0, corner in the window
            }
            if (i < 9 * DCNW_PM) Rec[i] = rec;
        }
        fill_store();
    }
    __syncthreads();                               // records and the window of chunk 0 visible

    const int m = wave * 32 + l31;                 // this lane's pixel of the tile
    const int nb0 = n0 >> 5;
    const int ncb = a.cout_pad >> 5;
    cn_f32x16 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // one sampling record decoded: corner weights (zero where the corner is off the map,
    // dcn_v2_im2col_cuda.cu:30-45), mask, top-left corner, and whether the four corners lie inside the window
    struct Samp { float w1, w2, w3, w4, mk; int yl, xl; bool inwin; };
    auto decode = [&](const cn_i32x4 r) -> Samp {
        // by value through locals (casts on a vector ELEMENT expression: see cn_dcn2.hip)
        const int r0 = r[0], r1 = r[1], r2 = r[2];
        const uint32_t pk = (uint32_t)r[3];
        const float lh = __int_as_float(r0), lw = __int_as_float(r1);
        Samp s;
        s.mk = __int_as_float(r2);
        s.yl = (int)(short)(pk & 0xffffu);
        s.xl = (int)(short)(pk >> 16);
        const float hh = 1.f - lh, hw = 1.f - lw;
        const bool yl_ok = s.yl >= 0, xl_ok = s.xl >= 0;
        const bool yh_ok = s.yl + 1 <= H - 1, xh_ok = s.xl + 1 <= W - 1;
        s.w1 = (yl_ok && xl_ok) ? hh * hw : 0.f;
        s.w2 = (yl_ok && xh_ok) ? hh * lw : 0.f;
        s.w3 = (yh_ok && xl_ok) ? lh * hw : 0.f;
        s.w4 = (yh_ok && xh_ok) ? lh * lw : 0.f;
        s.inwin = (unsigned)(s.yl - wy0) <= (unsigned)(DCNW_WY - 2) && (unsigned)(s.xl - wx0) <= (unsigned)(DCNW_WX - 2);
        return s;
    };
    // the sixteen window reads of a sample: K step kk of this lane is the 16 bytes at 32 kk + 16 h of a pixel
    // (a lane whose sample lies beyond the window's reach reads its own pixel's position; the values are replaced
    // from global memory when the sample is blended)
    cn_f32x4 c1[4], c2[4], c3[4], c4[4];
    auto request_corners = [&](const Samp &s) {
        const int wyl = s.inwin ? s.yl - wy0 : (m >> 4) + 1 + DCNW_RCH;
        const int wxl = s.inwin ? s.xl - wx0 : (m & 15) + 1 + DCNW_RCH;
        const dcnw_lds_f32x4 *c0 = reinterpret_cast<const dcnw_lds_f32x4 *>(
            win_lds + (unsigned)(wyl * H_WLINE + wxl * H_WROW + 4 * h) * 4u);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            c1[kk] = c0[2 * kk];
            c2[kk] = c0[H_WROW / 4 + 2 * kk];
            c3[kk] = c0[H_WLINE / 4 + 2 * kk];
            c4[kk] = c0[H_WLINE / 4 + H_WROW / 4 + 2 * kk];
        }
    };

    for (int chunk = 0; chunk < a.nchunk; ++chunk) {
        if (chunk != 0) {
            __syncthreads();                       // every wave is done with the previous window
            fill_load(chunk);
            fill_store();
            __syncthreads();
        }
        const unsigned cb = (unsigned)chunk * 128u;
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            // weights of this (tap, chunk): the MFMA's A operand, output channel 32 (nb0 + j) + l31, straight
            // from the packed rows (rows past cout_pad are clamped: their channels are never stored)
            dcnw_f16x8 wf[NB][4];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int nrow = min(nb0 + j, ncb - 1) * 32 + l31;
                const char *g = reinterpret_cast<const char *>(a.w) +
                                ((size_t)(t * a.cout_pad + nrow) * a.Cin + (size_t)chunk * 64 + 8 * h) * 2;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) wf[j][kk] = *reinterpret_cast<const dcnw_f16x8 *>(g + kk * 32);
            }
            const Samp cur = decode(Rec[t * DCNW_PM + m]);
            request_corners(cur);
            cn_f32x4 sf[4];
            if (cur.inwin) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    sf[kk] = dh_blend(c1[kk], c2[kk], c3[kk], c4[kk], cur.w1, cur.w2, cur.w3, cur.w4, cur.mk);
            } else {
                // beyond the window's reach: the four corners from global memory (clamped addresses; off-map
                // corners carry zero weight)
                const int y0 = max(cur.yl, 0), y1 = min(cur.yl + 1, H - 1);
                const int x0 = max(cur.xl, 0), x1 = min(cur.xl + 1, W - 1);
                const dcnw_glb_char *g = xg + cb + 16u * h;
                const unsigned o1 = (img_base + (unsigned)(y0 * W + x0)) * pix_bytes;
                const unsigned o2 = (img_base + (unsigned)(y0 * W + x1)) * pix_bytes;
                const unsigned o3 = (img_base + (unsigned)(y1 * W + x0)) * pix_bytes;
                const unsigned o4 = (img_base + (unsigned)(y1 * W + x1)) * pix_bytes;
                cn_f32x4 g1[4], g2[4], g3[4], g4[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    g1[kk] = *reinterpret_cast<const dcnw_glb_f32x4 *>(g + o1 + 32 * kk);
                    g2[kk] = *reinterpret_cast<const dcnw_glb_f32x4 *>(g + o2 + 32 * kk);
                    g3[kk] = *reinterpret_cast<const dcnw_glb_f32x4 *>(g + o3 + 32 * kk);
                    g4[kk] = *reinterpret_cast<const dcnw_glb_f32x4 *>(g + o4 + 32 * kk);
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    sf[kk] = dh_blend(g1[kk], g2[kk], g3[kk], g4[kk], cur.w1, cur.w2, cur.w3, cur.w4, cur.mk);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j][kk], __builtin_bit_cast(dcnw_f16x8, sf[kk]),
                                                                    acc[j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
        }
    }

    // ---- epilogue: y = relu?((acc + bias) * scale + shift) in fp32.  Each wave stages its 32 pixels x BN
    // channels in its own LDS region (the window and records are dead) and stores whole 16-byte groups of halves.
    // acc[j][r]: output channel 32 j + (r & 3) + 8 (r >> 2) + 4 h of pixel l31.
    __syncthreads();
    float *Cs = reinterpret_cast<float *>(smem) + wave * 32 * LDC;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const cn_f32x4 v = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
            *reinterpret_cast<cn_f32x4 *>(Cs + l31 * LDC + 32 * j + 8 * g + 4 * h) = v;
        }
    constexpr int C8 = BN / 8;               // lanes per pixel row
    constexpr int RPP = 64 / C8;             // pixel rows per pass of the wave
    const int cq = lane % C8, rr = lane / C8;
    const int n = n0 + cq * 8;
    float bs[8], sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bool ok = (n + e) < a.Cout;
        bs[e] = (a.bias && ok) ? a.bias[n + e] : 0.f;
        sc[e] = (a.scale && ok) ? a.scale[n + e] : 1.f;
        sh[e] = (a.shift && ok) ? a.shift[n + e] : 0.f;
    }
    // (the staging region is wave-private and was written by this wave's own lanes: no barrier)
#pragma unroll
    for (int it = 0; it < 32 / RPP; ++it) {
        const int row = it * RPP + rr;
        const int mm = wave * 32 + row;
        const size_t off = (size_t)((b * H + ty0 + (mm >> 4)) * W + tx0 + (mm & 15));
        if (n + 8 <= a.Cout) {               // Cout is a multiple of 8: a group is whole or absent
            const cn_f32x4 v0 = *reinterpret_cast<const cn_f32x4 *>(Cs + row * LDC + cq * 8);
            const cn_f32x4 v1 = *reinterpret_cast<const cn_f32x4 *>(Cs + row * LDC + cq * 8 + 4);
            dcnw_f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float tt = ((e < 4 ? v0[e & 3] : v1[e & 3]) + bs[e]) * sc[e] + sh[e];
                o[e] = (_Float16)(a.relu ? fmaxf(tt, 0.f) : tt);
            }
            *reinterpret_cast<dcnw_f16x8 *>(a.y + off * a.out_pitch + n) = o;
        }
    }
}

template <int BN>
int dcn_half_launch(const DcnHArgs &a, unsigned grid_y, hipStream_t st)
{
    CN_SET_MAX_LDS_ONCE(dcn_half_kernel<BN>, H_LDS);
    const dim3 grid((unsigned)(a.B * a.tiles_x * a.tiles_y), grid_y, 1);
    hipLaunchKernelGGL(dcn_half_kernel<BN>, grid, dim3(H_NT), H_LDS, st, a);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace

// Shapes the half window form takes: maps of whole 8 x 16 pixel tiles, whole 64-channel chunks, Cout a multiple
// of 8 (16-byte groups of halves out) and >= 33, 32-bit byte offsets into x (2-byte elements), 16-bit corner
// coordinates in a record.
bool cn_dcn_half_window_takes(const DcnCall &c)
{
    if (c.dtype != CN_DTYPE_F16) return false;
    if ((c.H & 7) || (c.W & 15) || (c.Cin & 63)) return false;
    if ((c.Cout & 7) || c.Cout <= 32 || (c.out_pitch & 7) || !cn_aligned16(c.y) || !cn_aligned16(c.x)) return false;
    if (c.H > 32767 || c.W > 32767) return false;
    return (size_t)c.B * c.H * c.W * c.Cin * 2 < ((size_t)1 << 32);
}

int cn_dcn_window_f16(const DcnCall &c, const DcnPlan &p, hipStream_t st)
{
    if (p.form != DCNH_WINDOW || p.ksplit != 1) return CN_ERR_UNSUPPORTED;
    DcnHArgs a = {};
    a.x = reinterpret_cast<const _Float16 *>(c.x); a.w = reinterpret_cast<const _Float16 *>(c.w);
    a.bias = c.bias; a.scale = c.scale; a.shift = c.shift; a.om = c.om; a.y = reinterpret_cast<_Float16 *>(c.y);
    a.B = c.B; a.H = c.H; a.W = c.W; a.Cin = c.Cin; a.Cout = c.Cout; a.om_pitch = c.om_pitch;
    a.mask_sigmoid = c.mask_sigmoid; a.relu = c.relu;
    a.cout_pad = (c.Cout + 31) / 32 * 32;
    a.nchunk = c.Cin / 64;
    a.tiles_x = c.W / DCNW_TX; a.tiles_y = c.H / DCNW_TY;
    a.out_pitch = c.out_pitch;
    a.rects = c.rects; a.rect_shift = c.rect_shift;
    return p.bn == 64 ? dcn_half_launch<64>(a, p.grid_y, st) : dcn_half_launch<128>(a, p.grid_y, st);
}
