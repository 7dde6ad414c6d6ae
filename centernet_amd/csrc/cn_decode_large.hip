// cn_decode_large.hip -- the image-level top-K of a heat-map for K up to CN_DECODE_LARGE_MAX_K = 1024 (dense
// scenes, the candidates of multi-scale testing): cn_ctdet_decode_large_f32 and cn_topk_large_f32, the large-K
// forms of cn_ctdet_decode_f32 and cn_topk_f32 (cn_decode.hip, K <= 128).  Same semantics, bit for bit where both
// take the call: optional logistic (sigmoidf_ref), 3x3 peak test on the scores with exact equality, heat * keep
// with -0 -> +0, zeros of suppressed cells take part when an image has fewer than K positive peaks, tie order
// score descending, class ascending, index ascending, rows assembled by emit_row (cn_decode_emit.h: the float
// operations of emit_rows).
//
// Two launches, no state words, no atomics on global memory -- the result cannot depend on the order in which
// workgroups arrive, and the workspace needs no preparation (CN_DECODE_STATE_CLEAN is accepted and means nothing):
//   large_band_kernel   one workgroup per (image, class, row band of <= 8192 cells): the band and its halo rows
//                       into LDS (logistic applied once), the key of heat * keep of every cell of the band into a
//                       second LDS array, then the exact radix_select of the band's min(K, cells) best keys, which
//                       go UNSORTED into the band's own slot of the candidate buffer (B * C * bands * K keys).
//                       The image's K best are among them: a band cannot contribute more than its own K best.
//   large_merge_kernel  one workgroup of 1024 threads per image: radix_select of the K best among the image's
//                       candidate keys, streamed from global memory; the K keys into LDS, a workgroup-wide
//                       1024-key bitonic sort (one key per thread: strides below 64 by wave shuffles, above
//                       through LDS), one row per thread.
// How many keys a slot holds is a function of the geometry (min(K, cells of the band)): nothing is counted in
// global memory.  The keys are distinct (the index is part of the key), so the sort is a strict total order.
#include "cn_internal.h"
#include "cn_select.h"
#include "cn_decode_emit.h"

namespace {

constexpr int LK_MAX = CN_DECODE_LARGE_MAX_K;
constexpr int LK_BAND_CELLS = 8192;   // cells of a band: tile + keys + select state stay under ~76 KB of LDS
static_assert(LK_MAX == NTM, "the merge sorts one key per thread");
static_assert(KMAX == CN_DECODE_MAX_K, "the header states the limit of the K <= 128 entries");

struct LargePlan {
    int rc;          // CN_OK, or why the call has no plan
    int R, nbands;   // rows per band, bands per plane
    size_t lds;      // dynamic LDS of large_band_kernel
    size_t total;    // workspace bytes: the candidate keys
};

// keys of band `band` of a plane: what its slot holds
__device__ __forceinline__ int band_keys(int band, int R, int H, int W, int K)
{
    return min(K, min(R, H - band * R) * W);
}

// grid (nbands, C, B), block NT, dynamic LDS = SelShared | tile (R+2)*W floats | keys R*W words
__global__ __launch_bounds__(NT) void large_band_kernel(const float *__restrict__ heat, int C, int H, int W, int K,
                                                        int R, int flags, u64 *__restrict__ cand)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    float *tile = reinterpret_cast<float *>(smem + sizeof(SelShared));
    uint32_t *ckey = reinterpret_cast<uint32_t *>(tile + (size_t)(R + 2) * W);

    const int tid = threadIdx.x;
    const int band = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int nbands = gridDim.x;
    const int r0 = band * R;
    const int rows = min(R, H - r0);
    const int n_band = rows * W;
    const int trows = rows + 2;
    const float *plane = heat + ((size_t)b * C + c) * (size_t)H * W;
    const float NEG_INF = -__builtin_huge_valf();
    const bool nonms = (flags & CN_DECODE_NO_PEAK_TEST) != 0;
    const bool sig = (flags & CN_DECODE_SIGMOID) != 0;

    // ---- rows r0-1 .. r0+rows into LDS, the logistic applied once; rows outside the map are -inf (decode.py:12)
    if ((W & 3) == 0) {
        const int w4 = W >> 2;
        const int nq = trows * w4;
        for (int q = tid; q < nq; q += NT) {
            const int tr = q / w4;
            const int c4 = q - tr * w4;
            const int gy = r0 - 1 + tr;
            cn_f32x4 v = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
            if (gy >= 0 && gy < H) {
                v = *reinterpret_cast<const cn_f32x4 *>(plane + (size_t)gy * W + c4 * 4);
                if (sig) {
                    v.x = sigmoidf_ref(v.x);
                    v.y = sigmoidf_ref(v.y);
                    v.z = sigmoidf_ref(v.z);
                    v.w = sigmoidf_ref(v.w);
                }
            }
            *reinterpret_cast<cn_f32x4 *>(tile + tr * W + c4 * 4) = v;
        }
    } else {
        const int ne = trows * W;
        for (int q = tid; q < ne; q += NT) {
            const int tr = q / W;
            const int x = q - tr * W;
            const int gy = r0 - 1 + tr;
            float v = NEG_INF;
            if (gy >= 0 && gy < H) {
                v = plane[(size_t)gy * W + x];
                if (sig) v = sigmoidf_ref(v);
            }
            tile[tr * W + x] = v;
        }
    }
    __syncthreads();

    // ---- the key of heat * keep of every cell of the band (decode.py:9-15; -0.0 -> +0.0), once
    for (int e = tid; e < n_band; e += NT) {
        const int y = e / W, x = e - y * W;
        const float *row = tile + (y + 1) * W + x;
        const float v = row[0];
        float m = fmaxf(fmaxf(row[-W], row[W]), v);
        if (x > 0) m = fmaxf(fmaxf(m, row[-1]), fmaxf(row[-W - 1], row[W - 1]));
        if (x < W - 1) m = fmaxf(fmaxf(m, row[1]), fmaxf(row[-W + 1], row[W + 1]));
        ckey[e] = f2key(((nonms || m == v) ? v : 0.0f) + 0.0f);
    }
    __syncthreads();

    // ---- the band's kb best keys, exactly, unsorted into its slot
    const uint32_t base = (uint32_t)c * (uint32_t)(H * W) + (uint32_t)(r0 * W);
    const int kb = min(K, n_band);
    auto for_each = [&](auto &&f) {
        for (int e = tid; e < n_band; e += NT) {
            const uint32_t kk = ckey[e];
            f(((u64)kk << 32) | (u64)(0xFFFFFFFFu - (base + (uint32_t)e)), kk == KEY_ZERO);
        }
    };
    u64 prefix, mask;
    radix_select<NT>(for_each, (uint32_t)kb, sh, prefix, mask);
    __syncthreads();
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
    u64 *slot = cand + ((((size_t)b * C + c) * nbands) + band) * (size_t)K;
    for_each([&](u64 k, bool) {
        if ((k & mask) >= prefix) {
            const uint32_t pos = atomicAdd(&sh.cnt, 1u);
            if (pos < (uint32_t)kb) slot[pos] = k;
        }
    });
}

// grid B, block NTM, dynamic LDS = SelShared
template <int MODE>
__global__ __launch_bounds__(NTM) void large_merge_kernel(const u64 *__restrict__ cand, int C, int nbands, int R,
                                                          int H, int W, int K, const EmitArgs ea)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    __shared__ u64 skey[LK_MAX];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int nslot = C * nbands;   // (C * H * W < 2^31)
    const u64 *kimg = cand + (size_t)b * nslot * K;
    // slot-major: P = the power of two that holds K; the workgroup walks NTM / P slots at a time, a thread keeps
    // its position in the slot (no division per key)
    const int lg = K <= 1 ? 0 : 32 - __clz(K - 1);   // P = 1 << lg, K <= P <= NTM
    const int pos = tid & ((1 << lg) - 1), s0 = tid >> lg, sstep = NTM >> lg;

    auto for_each = [&](auto &&f) {
        if (pos >= K) return;
        for (int s = s0; s < nslot; s += sstep) {
            if (pos < band_keys(nbands == 1 ? 0 : s % nbands, R, H, W, K)) {
                const u64 k = kimg[(size_t)s * K + pos];
                f(k, (uint32_t)(k >> 32) == KEY_ZERO);
            }
        }
    };
    u64 prefix, mask;
    radix_select<NTM>(for_each, (uint32_t)K, sh, prefix, mask);
    __syncthreads();
    if (tid == 0) sh.cnt = 0;
    skey[tid] = 0;   // pad keys sort last
    __syncthreads();
    for_each([&](u64 k, bool) {
        if ((k & mask) >= prefix) {
            const uint32_t pos = atomicAdd(&sh.cnt, 1u);
            if (pos < (uint32_t)LK_MAX) skey[pos] = k;
        }
    });
    __syncthreads();

    // ---- bitonic sort, descending, one key per thread
    u64 v = skey[tid];
    for (int k = 2; k <= LK_MAX; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            u64 o;
            if (j >= CN_WAVE) {
                __syncthreads();   // (everyone has read the previous exchange)
                skey[tid] = v;
                __syncthreads();
                o = skey[tid ^ j];
            } else {
                const uint32_t olo = __shfl_xor((uint32_t)v, j);
                const uint32_t ohi = __shfl_xor((uint32_t)(v >> 32), j);
                o = ((u64)ohi << 32) | olo;
            }
            const bool desc = (tid & k) == 0;
            const bool lower = (tid & j) == 0;
            const bool take_max = (lower == desc);
            v = take_max ? (v > o ? v : o) : (v > o ? o : v);
        }
    }
    if (tid < K) emit_row<MODE>(v, tid, b, H, W, K, C, ea);
}

// the one place that says whether a call is taken, its band geometry and its workspace
LargePlan large_route(int B, int C, int H, int W, int K)
{
    LargePlan p = {};
    p.rc = CN_ERR_SHAPE;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return p;
    if ((long)K > (long)H * W) return p;   // torch.topk: k out of range
    p.rc = CN_ERR_UNSUPPORTED;
    if (K > LK_MAX) return p;
    if ((long)C * H * W >= (1L << 31)) return p;        // 32-bit cell indices in the keys
    if (W > 4096 || C > 65535 || B > 65535) return p;   // (a row of the band in LDS; grid dimensions)
    int R = LK_BAND_CELLS / W;
    if (R < 1) R = 1;
    if (R > H) R = H;
    p.R = R;
    p.nbands = cn_cdiv(H, R);
    p.lds = sizeof(SelShared) + (size_t)(R + 2) * W * sizeof(float) + (size_t)R * W * sizeof(uint32_t);
    if (p.lds > 160 * 1024) return p;
    p.total = cn_align_up((size_t)B * C * p.nbands * K * sizeof(u64), 256);
    p.rc = CN_OK;
    return p;
}

template <int MODE>
int large_run(const float *heat, int B, int C, int H, int W, int K, int flags, const EmitArgs &ea, void *workspace,
              size_t workspace_bytes, void *stream)
{
    if (!heat) return CN_ERR_NULL;
    const LargePlan p = large_route(B, C, H, W, K);
    if (p.rc != CN_OK) return p.rc;
    if (((W & 3) == 0) && !cn_aligned16(heat)) return CN_ERR_ALIGN;
    const bool missing = MODE == MODE_CTDET ? (!ea.wh || !ea.dets) : (!ea.out_scores || !ea.inds_out || !ea.cls_out);
    if (missing || !workspace) return CN_ERR_NULL;
    if (!cn_aligned16(workspace)) return CN_ERR_ALIGN;
    if (workspace_bytes < p.total) return CN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    u64 *cand = (u64 *)workspace;
    CN_SET_MAX_LDS_ONCE(large_band_kernel, 160 * 1024);
    hipLaunchKernelGGL(large_band_kernel, dim3(p.nbands, C, B), dim3(NT), p.lds, st, heat, C, H, W, K, p.R, flags,
                       cand);
    CN_CHECK_LAUNCH();
    hipLaunchKernelGGL(large_merge_kernel<MODE>, dim3(B), dim3(NTM), sizeof(SelShared), st, cand, C, p.nbands, p.R,
                       H, W, K, ea);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace

extern "C" size_t cn_ctdet_decode_large_workspace_bytes(int B, int C, int H, int W, int K)
{
    const LargePlan p = large_route(B, C, H, W, K);
    return p.rc == CN_OK ? p.total : 0;
}

extern "C" int cn_ctdet_decode_large_f32(const float *heat, const float *wh, const float *reg, int B, int C, int H,
                                         int W, int K, int cat_spec_wh, int apply_sigmoid, float *dets,
                                         int32_t *inds, void *workspace, size_t workspace_bytes, void *stream)
{
    EmitArgs ea = {};
    ea.wh = wh;
    ea.reg = reg;
    ea.cat_spec_wh = cat_spec_wh;
    ea.dets = dets;
    ea.inds_out = inds;
    return large_run<MODE_CTDET>(heat, B, C, H, W, K, apply_sigmoid, ea, workspace, workspace_bytes, stream);
}

extern "C" int cn_topk_large_f32(const float *heat, int B, int C, int H, int W, int K, int apply_sigmoid,
                                 float *scores, int32_t *inds, int32_t *clses, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    EmitArgs ea = {};
    ea.out_scores = scores;
    ea.inds_out = inds;
    ea.cls_out = clses;
    return large_run<MODE_TOPK>(heat, B, C, H, W, K, apply_sigmoid, ea, workspace, workspace_bytes, stream);
}
