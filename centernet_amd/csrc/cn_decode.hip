// cn_decode.hip -- the top-K of a heat-map for gfx950: sigmoid -> 3x3 peak test -> exact top-K -> the rows
// of the K winners (ctdet boxes, _topk / _topk_channel lists, multi_pose stage-A rows).
//
// Reference behaviour being replaced (src/lib of the reference):
//   hm.sigmoid_()                      detectors/ctdet.py:31
//   _nms                               models/decode.py:9-15
//   _topk_channel / _topk              models/decode.py:92-119
//   _transpose_and_gather_feat         models/utils.py:22-26
//   ctdet_decode                       models/decode.py:464-495
//
// Three forms compute the same K rows, bit for bit (tests/test_gpu_decode.py):
//   one launch     plane_select_merge_kernel: planes of at most 128 x 128 cells, a workgroup holds one
//                  (image, class) plane in registers; the image's last plane to arrive selects and emits.
//   two launches   group_max_kernel + collect_merge_kernel: any plane size; group maxima give an image
//                  threshold, the planes collect the cells that reach it, the last arriver selects and emits.
//   per band       nms_topk_kernel per (image, class, row band) leaves the band's K best as candidates,
//                  merge_topk_kernel selects among them and emits.  With one band per plane the channel
//                  lists are already final: the merge is skipped (the direct form).
// The image-level forms rank ALL classes of an image and exist for MODE_CTDET and MODE_TOPK only.
//
// Host side: every entry fills a TopkCall (cn_internal.h).  topk_route() is the one place that says which
// form a call takes, its band geometry and every workspace offset -- the workspace and state-region
// queries read the same plan -- and topk_run() is the one place that checks, routes and launches.  The
// select machinery is in cn_select.h; pose matching and the ddd / exct / agnex decoders, which reach the
// top-K through topk_run() and cn_topk_f32, are in cn_decode_tasks.hip.
//
// Order of equal scores (torch.topk leaves it unspecified): score descending, then class ascending, then
// spatial index ascending -- the 64-bit key makes that a strict total order, so the result is deterministic.
#include "cn_internal.h"
#include "cn_select.h"

namespace {

// (sigmoidf_ref: cn_common.h -- one definition of the logistic for every decode form and the flip average)

constexpr int CAND_CAP = 4096;  // compacted positive peaks per band (uint16 tile offsets)

// ---------------------------------------------------------------------------
// The per-band select: per (image, class, row-band): sigmoid + 3x3 peak test + top-K
// grid (nbands, C, B), block NT, dynamic LDS = SelShared | tile (R+2)*W floats | peak list
//
// Fast path: the peak test (four cells per step, horizontal 3-max shared between the three
// rows) appends the tile offsets of the POSITIVE peaks -- about a ninth of the cells -- to a
// compact LDS list with one wave-aggregated atomic per step; the exact radix select then
// touches only that list.  If a band holds fewer than K positive peaks, or more than the
// list can hold (constant maps, tiny maps, negative "heat"), the kernel falls back to a
// full scan that re-evaluates the peak test per element, so every input is still exact.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void nms_topk_kernel(const float *__restrict__ heat, int C, int H,
                                                      int W, int K, int R, int flags,
                                                      float *__restrict__ cand_score,
                                                      int32_t *__restrict__ cand_idx)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    float *tile = reinterpret_cast<float *>(smem + sizeof(SelShared));

    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1);
    const int band = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int nbands = gridDim.x;
    const int r0 = band * R;
    const int rows = min(R, H - r0);  // rows of this band
    const int n_band = rows * W;
    const int trows = rows + 2;
    uint16_t *clist = reinterpret_cast<uint16_t *>(tile + (size_t)(R + 2) * W);
    const float *plane = heat + ((size_t)b * C + c) * (size_t)H * W;
    const float NEG_INF = -__builtin_huge_valf();
    // ablation bits for tools/bench_decode.py (never set through the Python API)
    const bool dbg_noselect = (flags & 256) != 0;
    const bool dbg_nonms = (flags & CN_DECODE_NO_PEAK_TEST) != 0;  // plain topk
    const bool dbg_slow = (flags & 1024) != 0;
    const int apply_sigmoid = flags & CN_DECODE_SIGMOID;
    if (tid == 0) sh.ncand = 0;

    // ---- stage rows r0-1 .. r0+rows (rows+2 rows) into LDS, sigmoid applied once
    const bool vec = (W & 3) == 0;
    if (vec) {
        const int w4 = W >> 2;
        const int nq = trows * w4;
        constexpr int U = 8;  // global loads in flight per thread before the first use
        for (int q0 = tid; q0 < nq; q0 += U * NT) {
            cn_f32x4 v[U];
            int dst[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = q0 + u * NT;
                dst[u] = -1;
                v[u].x = v[u].y = v[u].z = v[u].w = NEG_INF;
                if (q < nq) {
                    const int tr = q / w4;
                    const int c4 = q - tr * w4;
                    const int gy = r0 - 1 + tr;
                    dst[u] = tr * W + c4 * 4;
                    if (gy >= 0 && gy < H) {
                        v[u] = *reinterpret_cast<const cn_f32x4 *>(plane + (size_t)gy * W + c4 * 4);
                    } else {
                        dst[u] |= 0x40000000;  // halo row outside the image: keep -inf
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (dst[u] < 0) continue;
                cn_f32x4 t = v[u];
                if (apply_sigmoid && !(dst[u] & 0x40000000)) {
                    t.x = sigmoidf_ref(t.x);
                    t.y = sigmoidf_ref(t.y);
                    t.z = sigmoidf_ref(t.z);
                    t.w = sigmoidf_ref(t.w);
                }
                *reinterpret_cast<cn_f32x4 *>(tile + (dst[u] & 0x3FFFFFFF)) = t;
            }
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
                if (apply_sigmoid) v = sigmoidf_ref(v);
            }
            tile[tr * W + x] = v;
        }
    }
    __syncthreads();

    // peak test of one cell (decode.py:9-15); t = offset of the cell in the tile
    auto nms_val = [&](int t, int x) -> float {
        const float *row = tile + t;
        const float v = row[0];
        float m = fmaxf(fmaxf(row[-W], row[W]), v);
        if (x > 0) m = fmaxf(fmaxf(m, row[-1]), fmaxf(row[-W - 1], row[W - 1]));
        if (x < W - 1) m = fmaxf(fmaxf(m, row[1]), fmaxf(row[-W + 1], row[W + 1]));
        if (dbg_nonms) m = v;
        return ((m == v) ? v : 0.0f) + 0.0f;  // heat * keep, -0.0 -> +0.0
    };
    // append the tile offset of a positive peak; one LDS atomic per wave per call
    auto append = [&](bool is, int t) {
        const u64 bal = __ballot(is);
        if (bal) {
            const int leader = __ffsll((long long)bal) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&sh.ncand, (uint32_t)__popcll(bal));
            base = __shfl(base, leader);
            if (is) {
                const uint32_t pos =
                    base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                if (pos < (uint32_t)CAND_CAP) clist[pos] = (uint16_t)t;
            }
        }
    };

    if (vec) {
        const int w4 = W >> 2;
        const int nq = rows * w4;
        const int nqr = (nq + NT - 1) / NT * NT;  // whole waves take part in the ballots
        for (int q = tid; q < nqr; q += NT) {
            bool pk[4] = {false, false, false, false};
            int t0 = 0;
            if (q < nq) {
                const int y = q / w4;
                const int x4 = q - y * w4;
                t0 = (y + 1) * W + x4 * 4;
                float hm[4] = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
                cn_f32x4 ctr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dr = -1; dr <= 1; ++dr) {
                    const float *row = tile + t0 + dr * W;
                    const cn_f32x4 cv = *reinterpret_cast<const cn_f32x4 *>(row);
                    const float l = (x4 > 0) ? row[-1] : NEG_INF;
                    const float r = (x4 < w4 - 1) ? row[4] : NEG_INF;
                    hm[0] = fmaxf(hm[0], fmaxf(fmaxf(l, cv.x), cv.y));
                    hm[1] = fmaxf(hm[1], fmaxf(fmaxf(cv.x, cv.y), cv.z));
                    hm[2] = fmaxf(hm[2], fmaxf(fmaxf(cv.y, cv.z), cv.w));
                    hm[3] = fmaxf(hm[3], fmaxf(fmaxf(cv.z, cv.w), r));
                    if (dr == 0) ctr = cv;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = (dbg_nonms || hm[e] == ctr[e]) && ctr[e] > 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) append(pk[e], t0 + e);
        }
    } else {
        const int nr = (n_band + NT - 1) / NT * NT;
        for (int e = tid; e < nr; e += NT) {
            bool is = false;
            int t = 0;
            if (e < n_band) {
                const int y = e / W, x = e - y * W;
                t = (y + 1) * W + x;
                is = nms_val(t, x) > 0.0f;
            }
            append(is, t);
        }
    }
    __syncthreads();

    const uint32_t base = (uint32_t)(r0 * W);
    const int kb = min(K, n_band);
    const uint32_t npos = sh.ncand;
    const bool fast = !dbg_slow && npos >= (uint32_t)kb && npos <= (uint32_t)CAND_CAP;
    u64 prefix, mask;
    if (dbg_noselect) {
        if (tid < KMAX) sh.sel[tid] = npos;
        __syncthreads();
    } else if (fast) {
        auto for_each = [&](auto &&f) {
            for (uint32_t j = tid; j < npos; j += NT) {
                const uint32_t t = clist[j];
                f(((u64)f2key(tile[t]) << 32) | (u64)(0xFFFFFFFFu - (base + t - (uint32_t)W)), false);
            }
        };
        radix_select<NT>(for_each, (uint32_t)kb, sh, prefix, mask);
        collect_and_sort<NT>(for_each, prefix, mask, sh);
    } else {
        // exact fallback: every cell takes part (zeros from suppressed cells included)
        auto for_each = [&](auto &&f) {
            for (int e = tid; e < n_band; e += NT) {
                const int y = e / W, x = e - y * W;
                const uint32_t kk = f2key(nms_val((y + 1) * W + x, x));
                f(((u64)kk << 32) | (u64)(0xFFFFFFFFu - (base + (uint32_t)e)), kk == KEY_ZERO);
            }
        };
        radix_select<NT>(for_each, (uint32_t)kb, sh, prefix, mask);
        collect_and_sort<NT>(for_each, prefix, mask, sh);
    }

    if (tid < K) {
        const size_t o = ((((size_t)b * C + c) * nbands) + band) * K + tid;
        if (tid < kb) {
            const u64 k = sh.sel[tid];
            cand_score[o] = key2f((uint32_t)(k >> 32));
            cand_idx[o] = (int32_t)(0xFFFFFFFFu - (uint32_t)k);
        } else {
            cand_score[o] = NEG_INF;
            cand_idx[o] = -1;
        }
    }
}

// ---------------------------------------------------------------------------
// Image-level top-K without a per-band select (ctdet / _topk: the K best peaks of ALL classes of
// an image, decode.py:103-119).  Only ~K of the C*H*W cells matter, so the exact select runs on
// a threshold-pruned candidate list instead of in every (class, band) -- in TWO launches:
//   launch 1  group_max_kernel: ONE streaming pass over the raw map (logits when the sigmoid is
//             fused: the logistic is monotone, no transcendental per cell).  A GROUP is 8 rows x 128
//             columns of a plane; per group it records the largest raw value of all cells and the
//             largest raw value among the cells that pass the 3x3 peak test on RAW values (a raw
//             peak is also a peak of the sigmoid values).
//   launch 2  collect_merge_kernel, one workgroup per plane:
//             image_threshold: T_b = K-th largest group peak-maximum of image b (as a score),
//               computed by every plane of the image from the same ~1 k keys (cheaper than a launch
//               boundary, and no workgroup ever waits for another).  At least K distinct peaks reach
//               T_b, so every cell of the exact top-K has a peak value >= T_b -- ties at T_b
//               included -- and nothing below can be in it.
//             plane_collect: only the groups whose all-cell maximum reaches T_b are looked at again
//               (L2 / Infinity-Cache resident); their cells get the EXACT treatment -- sigmoid, 3x3
//               equality test on sigmoid values (decode.py:9-15) -- and are appended to the image's
//               candidate list as 64-bit keys (score, ~flat index).
//             the image's LAST plane to arrive (one atomic counter per image): exact radix select +
//               sort of the few hundred candidates, gather, box assembly.
// A plane hands on at most its own K best keys (exact select inside the plane when it holds more:
// saturated plateaus), so the image's list of C * K keys cannot overflow; images with T_b <= 0 (fewer
// than K groups with a positive peak; constant maps: zeros of suppressed cells take part) run that
// per-plane select over all cells of every plane.  Every input is handled exactly by the same two
// launches; both forms are bit-identical to the per-(class, band) select of round 1.
// ---------------------------------------------------------------------------

// A GROUP = 8 rows x 128 columns of one (image, class) plane.  One half-wave owns a 16-row x
// 128-column unit (two groups): lane l holds the 4-cell quad l of a row and walks down the
// rows with the previous / current / next row in registers, so every cell is loaded from global
// memory exactly once (18 row loads for 16 rows, all issued up front), horizontal neighbours come
// from the adjacent lanes by shuffle, and nothing goes through LDS.
constexpr int GROWS = 8;     // rows per group
constexpr int GUNIT = 16;    // rows per half-wave unit

__global__ __launch_bounds__(NT) void group_max_kernel(const float *__restrict__ heat, int H, int W,
                                                       int nrg, int ncb, int flags,
                                                       uint32_t *__restrict__ gpeak,
                                                       uint32_t *__restrict__ gall, int C,
                                                       int32_t *__restrict__ counts,
                                                       int32_t *__restrict__ done)
{
    const int tid = threadIdx.x;
    // the second launch's per-image candidate count and arrival counter start at zero (stream order)
    if (tid == 0 && blockIdx.x % (unsigned)C == 0) {
        counts[blockIdx.x / (unsigned)C] = 0;
        done[blockIdx.x / (unsigned)C] = 0;
    }
    const int lane = tid & (CN_WAVE - 1);
    const int hl = lane & 31;                 // lane inside the half-wave
    const int hw = tid >> 5;                  // half-wave of the workgroup (0..7)
    const int nunit_r = (nrg + 1) / 2;        // 16-row units per plane
    const int units = nunit_r * ncb;          // units per plane
    const int w4 = W >> 2;
    const float NEG_INF = -__builtin_huge_valf();
    const bool nonms = (flags & CN_DECODE_NO_PEAK_TEST) != 0;
    const size_t plane_id = blockIdx.x;       // b * C + c
    const float *plane = heat + plane_id * (size_t)H * W;
    for (int u = hw; u < units; u += NT / 32) {   // uniform per half-wave
        const int ur = u / ncb, cb = u - ur * ncb;
        const int y0 = ur * GUNIT;
        const int x4 = cb * 32 + hl;              // this lane's quad column
        const bool col_ok = x4 < w4;
        // rows y0-1 .. y0+16: all loads issued before the first use
        cn_f32x4 rowv[GUNIT + 2];
        float lft[GUNIT + 2], rgt[GUNIT + 2];     // cells just outside the 128-column block
#pragma unroll
        for (int r = 0; r < GUNIT + 2; ++r) {
            const int y = y0 - 1 + r;
            const bool ok = col_ok && y >= 0 && y < H;
            rowv[r].x = rowv[r].y = rowv[r].z = rowv[r].w = NEG_INF;
            lft[r] = rgt[r] = NEG_INF;
            if (ok) {
                const float *p = plane + (size_t)y * W + x4 * 4;
                rowv[r] = *reinterpret_cast<const cn_f32x4 *>(p);
                if (hl == 0 && x4 > 0) lft[r] = p[-1];
                if (hl == 31 && x4 + 1 < w4) rgt[r] = p[4];
            }
        }
        // horizontal 3-max of every row, then the vertical combination
        cn_f32x4 hmax[GUNIT + 2];
#pragma unroll
        for (int r = 0; r < GUNIT + 2; ++r) {
            float l = __shfl_up(rowv[r].w, 1, 32);
            float rr = __shfl_down(rowv[r].x, 1, 32);
            if (hl == 0) l = lft[r];
            if (hl == 31) rr = rgt[r];
            if (!col_ok) { l = NEG_INF; rr = NEG_INF; }
            // a lane beyond the map's last quad hands -inf to its left neighbour
            hmax[r].x = fmaxf(fmaxf(l, rowv[r].x), rowv[r].y);
            hmax[r].y = fmaxf(fmaxf(rowv[r].x, rowv[r].y), rowv[r].z);
            hmax[r].z = fmaxf(fmaxf(rowv[r].y, rowv[r].z), rowv[r].w);
            hmax[r].w = fmaxf(fmaxf(rowv[r].z, rowv[r].w), rr);
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint32_t kp = 0u, ka = 0u;
#pragma unroll
            for (int r = 1 + half * GROWS; r < 1 + (half + 1) * GROWS; ++r) {
                const int y = y0 - 1 + r;
                if (!(col_ok && y < H)) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = rowv[r][e];
                    const float m = fmaxf(fmaxf(hmax[r - 1][e], hmax[r][e]), hmax[r + 1][e]);
                    const uint32_t k = f2key(v + 0.0f);
                    ka = max(ka, k);
                    if (nonms || m == v) kp = max(kp, k);
                }
            }
            for (int o = 16; o > 0; o >>= 1) {
                kp = max(kp, (uint32_t)__shfl_xor((int)kp, o, 32));
                ka = max(ka, (uint32_t)__shfl_xor((int)ka, o, 32));
            }
            const int rg = ur * 2 + half;
            if (hl == 0 && rg < nrg) {
                const size_t gi = (plane_id * nrg + rg) * ncb + cb;
                gpeak[gi] = kp;
                gall[gi] = ka;
            }
        }
    }
}

// phase 2 (device function, run by EVERY plane's workgroup of the second launch -- the select over
// an image's ~1 k group maxima is cheaper than a launch boundary and needs no inter-workgroup
// wait): the K-th largest group peak-maximum of image b (exact).  Returns, to every thread, the
// SCORE key of the threshold (the logistic applied when it is fused; <= KEY_ZERO = degenerate
// image: fewer than K groups with a peak, or a non-positive threshold -- zeros of suppressed cells
// would take part) and a conservative lower bound, in raw units, of every cell whose score can
// reach it.
// the `need`-th largest of the 32-bit keys `for_each(f)` enumerates (f(key32)), exactly: three
// digit passes (11, 11, 10 bits, msb first) over a histogram in LDS, no early exit, no sort
// The bin of sh.hist that holds the `need`-th largest element (bins counted from the top): sh.digit =
// that bin, sh.need = the rank still to find inside it, sh.bincount = elements in that bin and above.
// All threads call it behind a barrier that closes the histogram; it ends with a barrier.
template <int TB>
__device__ __forceinline__ void suffix_bin(uint32_t need, SelShared &sh)
{
    constexpr int BPT = HBINS / TB;
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1), wave = tid / CN_WAVE;
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < BPT; ++j) p += sh.hist[tid * BPT + j];
    uint32_t s = p;
#pragma unroll
    for (int o = 1; o < CN_WAVE; o <<= 1) {
        const uint32_t t = __shfl_down(s, o);
        if (lane + o < CN_WAVE) s += t;
    }
    if (lane == 0) sh.wsum[wave] = s;
    __syncthreads();
    for (int w = wave + 1; w < TB / CN_WAVE; ++w) s += sh.wsum[w];
    const uint32_t above = s - p;  // elements in strictly higher bins
    if (above < need && s >= need) {
        uint32_t run = above;
        for (int j = BPT - 1; j >= 0; --j) {
            const uint32_t h = sh.hist[tid * BPT + j];
            if (run + h >= need) {
                sh.digit = tid * BPT + j;
                sh.need = need - run;
                sh.bincount = run + h;
                break;
            }
            run += h;
        }
    }
    __syncthreads();
}

template <int TB, class ForEach>
__device__ __forceinline__ uint32_t kth_largest_key32(ForEach &&for_each, uint32_t need, SelShared &sh)
{
    constexpr int BPT = HBINS / TB;
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1), wave = tid / CN_WAVE;
    uint32_t prefix = 0, mask = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const uint32_t dmask = pass == 2 ? 1023u : 2047u;
        for (int i = tid; i < HBINS; i += TB) sh.hist[i] = 0;
        __syncthreads();
        for_each([&](uint32_t k) {
            if ((k & mask) == prefix) atomicAdd(&sh.hist[(k >> shift) & dmask], 1u);
        });
        __syncthreads();
        uint32_t p = 0;
#pragma unroll
        for (int j = 0; j < BPT; ++j) p += sh.hist[tid * BPT + j];
        uint32_t s = p;
#pragma unroll
        for (int o = 1; o < CN_WAVE; o <<= 1) {
            const uint32_t t = __shfl_down(s, o);
            if (lane + o < CN_WAVE) s += t;
        }
        if (lane == 0) sh.wsum[wave] = s;
        __syncthreads();
        for (int w = wave + 1; w < TB / CN_WAVE; ++w) s += sh.wsum[w];
        const uint32_t above = s - p;  // keys in strictly higher bins
        if (above < need && s >= need) {
            uint32_t run = above;
            for (int j = BPT - 1; j >= 0; --j) {
                const uint32_t h = sh.hist[tid * BPT + j];
                if (run + h >= need) {
                    sh.digit = tid * BPT + j;
                    sh.need = need - run;
                    break;
                }
                run += h;
            }
        }
        __syncthreads();
        prefix |= sh.digit << shift;
        mask |= dmask << shift;
        need = sh.need;
        __syncthreads();       // (sh.digit / sh.need are rewritten by the next pass)
    }
    return prefix;
}

__device__ __forceinline__ uint32_t image_threshold(const uint32_t *__restrict__ g, int ng, int K, int flags,
                                                    SelShared &sh, float &rawthr)
{
    const int tid = threadIdx.x;
    rawthr = 0.f;
    if (ng < K) return 0u;
    // the image's group maxima: fetched ONCE into registers (a select pass over global memory is a
    // load round trip per pass: ~10 us per workgroup, and every plane's workgroup does this)
    constexpr int RK = 8;
    uint32_t kraw;
    if (ng <= RK * NT) {
        uint32_t kr[RK];
#pragma unroll
        for (int u = 0; u < RK; ++u) kr[u] = (tid + u * NT < ng) ? g[tid + u * NT] : 0u;
        auto for_each = [&](auto &&f) {
#pragma unroll
            for (int u = 0; u < RK; ++u)
                if (tid + u * NT < ng) f(kr[u]);
        };
        kraw = kth_largest_key32<NT>(for_each, (uint32_t)K, sh);
    } else {
        auto for_each = [&](auto &&f) {
            for (int j = tid; j < ng; j += NT) f(g[j]);
        };
        kraw = kth_largest_key32<NT>(for_each, (uint32_t)K, sh);
    }
    if (kraw == 0u) return 0u;    // fewer than K groups hold a peak at all
    const float raw = key2f(kraw);
    const bool sig = (flags & 1) != 0;
    const float score = sig ? sigmoidf_ref(raw) : raw;
    // the device logistic is monotone only up to its last bit: admit a margin of raw values
    // below the K-th one; the exact test in phase 3 sorts them out
    rawthr = sig ? raw - (1e-3f + 1e-3f * fabsf(raw)) : raw;
    return f2key(score + 0.0f);
}

// phase 3 (device function): the candidate keys of ONE plane.  The workgroup's eight half-waves share
// the plane's live groups (all-cell maximum >= the raw threshold).  A half-wave re-reads its 8 x 128
// group with the same rolling register window as phase 1 (10 row loads, neighbours by shuffle),
// applies the logistic to the whole window and runs the reference's test on the SCORES -- 3x3
// maximum, exact equality (decode.py:9-15) -- in registers; qualifying cells are counted per lane,
// placed by a half-wave prefix sum into a list in LDS.  The threshold often falls INTO the noise floor
// of a real heat-map (a few confident objects, K = 100): then most groups are live and this pass costs
// about what phase 1 does plus the logistics -- not nine dependent loads per cell over the threshold.
// A plane never has to hand on more than its own K best keys (the image's K best are among them), so
// the image's list -- capacity C * K -- cannot overflow whatever the map holds:
//   n <= K qualifying cells        -> all of them
//   K < n <= PLCAP                 -> exact select of the K best from the LDS list
//   n > PLCAP                      -> (class planes with a high bias hold most of an image's candidates)
//                                     the plane raises ITS threshold to the K-th best of the PLCAP keys
//                                     it did keep -- the plane's own K best all reach it -- and
//                                     collects again; only if that changes nothing (a plateau of more
//                                     than PLCAP equal scores)
//                                  -> exact select over the cells of the plane, keys recomputed per
//                                     pass from global memory (slow: hundreds of microseconds; rare)
// and a DEGENERATE image (threshold <= 0: fewer than K groups with a positive peak, constant maps --
// zeros of suppressed cells take part in the top K) takes the last route for every plane with all
// cells admitted: every input is handled exactly, by the same two launches.
constexpr int PLCAP = 1024;   // candidate keys of a plane kept in LDS

__device__ __forceinline__ void plane_collect(const float *__restrict__ heat, int C, int H, int W, int nrg,
                                              int ncb, int flags, int K, const uint32_t *__restrict__ gall,
                                              uint32_t tkey, float rthr, SelShared &sh, u64 *__restrict__ keys,
                                              int cap, int32_t *__restrict__ counts)
{
    __shared__ u64 pl_keys[PLCAP];
    __shared__ int pl_cnt, pl_base;
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1);
    const int hl = lane & 31, hw = tid >> 5;
    const size_t plane_id = blockIdx.x;
    const int b = (int)(plane_id / C), c = (int)(plane_id - (size_t)b * C);
    const bool sig = (flags & 1) != 0;
    const bool nonms = (flags & CN_DECODE_NO_PEAK_TEST) != 0;
    const bool degenerate = tkey <= KEY_ZERO;
    const uint32_t rkey = f2key(rthr + 0.0f);   // group maxima are RAW keys
    const int HW = H * W;
    const float *plane = heat + plane_id * (size_t)HW;
    const uint32_t base = (uint32_t)c * (uint32_t)HW;
    u64 *kimg = keys + (size_t)b * cap;
    const int w4 = W >> 2;
    const float NEG_INF = -__builtin_huge_valf();
    uint32_t tcur = tkey;          // the plane's current threshold (raised when its list overflows)

    auto collect_group = [&](int g) {
        const int rg = g / ncb, cb = g - rg * ncb;
        const int y0 = rg * GROWS;
        const int x4 = cb * 32 + hl;
        const bool col_ok = x4 < w4;
        cn_f32x4 rowv[GROWS + 2];
        float lft[GROWS + 2], rgt[GROWS + 2];
#pragma unroll
        for (int r = 0; r < GROWS + 2; ++r) {
            const int y = y0 - 1 + r;
            const bool ok = col_ok && y >= 0 && y < H;
            rowv[r].x = rowv[r].y = rowv[r].z = rowv[r].w = NEG_INF;
            lft[r] = rgt[r] = NEG_INF;
            if (ok) {
                const float *p = plane + (size_t)y * W + x4 * 4;
                rowv[r] = *reinterpret_cast<const cn_f32x4 *>(p);
                if (hl == 0 && x4 > 0) lft[r] = p[-1];
                if (hl == 31 && x4 + 1 < w4) rgt[r] = p[4];
            }
        }
        if (sig) {   // scores of the whole window (cells outside the map stay -inf)
#pragma unroll
            for (int r = 0; r < GROWS + 2; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (rowv[r][e] != NEG_INF) rowv[r][e] = sigmoidf_ref(rowv[r][e]);
                if (lft[r] != NEG_INF) lft[r] = sigmoidf_ref(lft[r]);
                if (rgt[r] != NEG_INF) rgt[r] = sigmoidf_ref(rgt[r]);
            }
        }
        cn_f32x4 hmax[GROWS + 2];
#pragma unroll
        for (int r = 0; r < GROWS + 2; ++r) {
            float l = __shfl_up(rowv[r].w, 1, 32);
            float rr = __shfl_down(rowv[r].x, 1, 32);
            if (hl == 0) l = lft[r];
            if (hl == 31) rr = rgt[r];
            if (!col_ok) { l = NEG_INF; rr = NEG_INF; }
            hmax[r].x = fmaxf(fmaxf(l, rowv[r].x), rowv[r].y);
            hmax[r].y = fmaxf(fmaxf(rowv[r].x, rowv[r].y), rowv[r].z);
            hmax[r].z = fmaxf(fmaxf(rowv[r].y, rowv[r].z), rowv[r].w);
            hmax[r].w = fmaxf(fmaxf(rowv[r].z, rowv[r].w), rr);
        }
        // this lane's 32 cells: bit (r-1)*4+e set when the cell's key reaches the threshold
        auto cell_key = [&](int r, int e) -> uint32_t {
            const float v = rowv[r][e];
            const float m = fmaxf(fmaxf(hmax[r - 1][e], hmax[r][e]), hmax[r + 1][e]);
            return f2key(((nonms || m == v) ? v : 0.0f) + 0.0f);
        };
        uint32_t tmask = 0u;
#pragma unroll
        for (int r = 1; r <= GROWS; ++r) {
            const int y = y0 - 1 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool take = col_ok && y < H && cell_key(r, e) >= tcur;
                tmask |= take ? (1u << ((r - 1) * 4 + e)) : 0u;
            }
        }
        // half-wave inclusive prefix sum of the per-lane counts, one LDS atomic for the group
        const int mine = __popc(tmask);
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int t = __shfl_up(incl, o, 32);
            if (hl >= o) incl += t;
        }
        const int total = __shfl(incl, 31, 32);
        if (total == 0) return;
        int pos0 = 0;
        if (hl == 31) pos0 = atomicAdd(&pl_cnt, total);
        int pos = __shfl(pos0, 31, 32) + incl - mine;
#pragma unroll
        for (int r = 1; r <= GROWS; ++r) {
            const int y = y0 - 1 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (tmask & (1u << ((r - 1) * 4 + e))) {
                    const uint32_t cell = (uint32_t)(y * W + x4 * 4 + e);
                    if (pos < PLCAP)
                        pl_keys[pos] = ((u64)cell_key(r, e) << 32) | (u64)(0xFFFFFFFFu - (base + cell));
                    ++pos;
                }
            }
        }
    };
    bool plateau = false;
    if (!degenerate)
    for (int round = 0;; ++round) {
        if (tid == 0) pl_cnt = 0;
        __syncthreads();
        const int ng = nrg * ncb;
        // which groups can hold a qualifying cell: all group maxima are fetched at once (a chain of
        // dependent loads here cost more than the whole streaming pass)
        // and the live ones compacted into a list, so that the two halves of a wave always work on
        // two groups at the same time
        __shared__ u64 live[NT / 64];
        __shared__ int glist[NT];
        for (int g0 = 0; g0 < ng; g0 += NT) {
            const int g = g0 + tid;
            const bool q = g < ng && gall[plane_id * ng + g] >= rkey;
            const u64 bal = __ballot(q);
            if (lane == 0) live[tid >> 6] = bal;
            __syncthreads();
            int before = 0, nlive = 0;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) {
                const int n = __popcll(live[w]);
                if (w < (tid >> 6)) before += n;
                nlive += n;
            }
            if (q) glist[before + __popcll(bal & ((1ull << lane) - 1ull))] = g;
            __syncthreads();
            for (int i = hw; i < nlive; i += NT / 32) collect_group(glist[i]);
            __syncthreads();
        }
        if (pl_cnt <= PLCAP) break;            // (uniform: read behind the barrier)
        // more qualifying cells than the list holds: raise the plane's threshold to the K-th best of the
        // PLCAP keys that were kept (its own K best all reach that) and collect again
        auto kept = [&](auto &&f) {
            for (int j = tid; j < PLCAP; j += NT) f((uint32_t)(pl_keys[j] >> 32));
        };
        const uint32_t tnew = kth_largest_key32<NT>(kept, (uint32_t)K, sh);
        if (tnew == tcur || round == 3) {      // a plateau of equal scores (or no progress): exact select below
            plateau = true;
            break;
        }
        tcur = tnew;
    }
    // ---- hand the plane's keys on: at most its K best
    const int n = (degenerate || plateau) ? PLCAP + 1 : pl_cnt;      // (uniform; the last loop round ended with a barrier)
    int m;                                              // keys this plane emits
    const u64 *src;
    if (n <= K) {
        m = n;
        src = pl_keys;
    } else {
        m = min(K, HW);
        u64 prefix, mask;
        if (n <= PLCAP) {
            auto for_each = [&](auto &&f) {
                for (int j = tid; j < n; j += NT) f(pl_keys[j], false);
            };
            radix_select<NT>(for_each, (uint32_t)m, sh, prefix, mask);
            collect_and_sort<NT>(for_each, prefix, mask, sh);
        } else {
            // every cell of the plane (degenerate image), or every cell that reaches the threshold (more
            // of them than the LDS list holds): keys recomputed from global memory in every pass
            auto for_each = [&](auto &&f) {
                for (int e = tid; e < HW; e += NT) {
                    const int y = e / W, x = e - y * W;
                    auto sc = [&](int yy, int xx) {
                        const float v = plane[yy * W + xx];
                        return sig ? sigmoidf_ref(v) : v;
                    };
                    const float v = sc(y, x);
                    float mx = v;
                    if (!nonms) {
                        for (int dy = -1; dy <= 1; ++dy) {
                            const int yy = y + dy;
                            if (yy < 0 || yy >= H) continue;
                            for (int dx = -1; dx <= 1; ++dx) {
                                const int xx = x + dx;
                                if (xx < 0 || xx >= W || (dy == 0 && dx == 0)) continue;
                                mx = fmaxf(mx, sc(yy, xx));
                            }
                        }
                    }
                    const uint32_t kk = f2key(((mx == v) ? v : 0.0f) + 0.0f);   // heat * keep, -0.0 -> +0.0
                    if (degenerate || kk >= tcur)
                        f(((u64)kk << 32) | (u64)(0xFFFFFFFFu - (base + (uint32_t)e)), kk == KEY_ZERO);
                }
            };
            radix_select<NT>(for_each, (uint32_t)m, sh, prefix, mask);
            collect_and_sort<NT>(for_each, prefix, mask, sh);
        }
        src = sh.sel;
    }
    if (m > 0) {
        // one returning atomic per plane reserves its slice of the image's list; the keys go out as
        // device-scope stores (read by the image's last workgroup, possibly on another XCD, without any
        // cache maintenance in between -- see collect_merge_kernel)
        if (tid == 0) pl_base = atomicAdd(&counts[b], m);
        __syncthreads();
        const int o = pl_base;
        for (int j = tid; j < m; j += NT)
            if (o + j < cap) __hip_atomic_store(kimg + o + j, src[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------
// The rows of the K winners, and the merge of the per-band form.
//   CTDET : group = image; N = C*per_class candidates, class = j / per_class;
//           output = gathered boxes (decode.py:472-493)
//   !CTDET: group = (image, channel); output = (scores, inds)  (_topk_channel)
// ---------------------------------------------------------------------------

// rows 0 .. K-1 of the sorted selection sh.sel -> outputs of group g (see merge_topk_kernel)
template <int MODE>
__device__ __forceinline__ void emit_rows(const SelShared &sh, int g, int H, int W, int K, int C, const EmitArgs &ea)
{
    const float *__restrict__ wh = ea.wh, *__restrict__ reg = ea.reg, *__restrict__ kps_map = ea.kps_map;
    float *__restrict__ dets = ea.dets, *__restrict__ out_scores = ea.out_scores;
    int32_t *__restrict__ inds_out = ea.inds_out, *__restrict__ cls_out = ea.cls_out;
    const int cat_spec_wh = ea.cat_spec_wh, J = ea.J;
    const int det_dim = 6 + 2 * J;   // a row: box, score, 2J keypoint coordinates (MODE_POSE), class
    constexpr bool CTDET = (MODE != MODE_CHANNEL);
    const int tid = threadIdx.x;
    const int HW = H * W;
    if (tid < K) {
        const u64 k = sh.sel[tid];
        const float score = key2f((uint32_t)(k >> 32));
        const uint32_t fid = 0xFFFFFFFFu - (uint32_t)k;
        if (CTDET) {
            const int cls = (int)(fid / (uint32_t)HW);
            const int ind = (int)(fid - (uint32_t)cls * (uint32_t)HW);
            const int yi = ind / W, xi = ind - yi * W;
            float xs = (float)xi, ys = (float)yi;
            const int b = g;
            if (MODE == MODE_TOPK) {  // _topk (decode.py:103-119): scores, inds, clses only
                out_scores[(size_t)b * K + tid] = score;
                inds_out[(size_t)b * K + tid] = ind;
                cls_out[(size_t)b * K + tid] = cls;
                return;
            }
            if (reg) {  // decode.py:472-476
                xs = xs + reg[((size_t)b * 2 + 0) * HW + ind];
                ys = ys + reg[((size_t)b * 2 + 1) * HW + ind];
            } else {  // decode.py:477-479
                xs = xs + 0.5f;
                ys = ys + 0.5f;
            }
            const int whC = cat_spec_wh ? 2 * C : 2;
            const int wc = cat_spec_wh ? 2 * cls : 0;  // decode.py:481-486
            const float w = wh[((size_t)b * whC + wc + 0) * HW + ind];
            const float h = wh[((size_t)b * whC + wc + 1) * HW + ind];
            float *d = dets + ((size_t)b * K + tid) * det_dim;
            d[0] = xs - w / 2;  // decode.py:489-492
            d[1] = ys - h / 2;
            d[2] = xs + w / 2;
            d[3] = ys + h / 2;
            d[4] = score;
            d[det_dim - 1] = (float)cls;
            if (MODE == MODE_POSE) {
                // decode.py:506-509: kps = hps[ind] + (xs, ys) with the un-offset centre
                const float x0 = (float)xi, y0 = (float)yi;
                for (int j = 0; j < J; ++j) {
                    d[5 + 2 * j] = kps_map[((size_t)b * 2 * J + 2 * j) * HW + ind] + x0;
                    d[5 + 2 * j + 1] = kps_map[((size_t)b * 2 * J + 2 * j + 1) * HW + ind] + y0;
                }
            }
            if (inds_out) inds_out[(size_t)b * K + tid] = ind;
        } else {
            out_scores[(size_t)g * K + tid] = score;
            inds_out[(size_t)g * K + tid] = (int32_t)fid;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(NTM) void merge_topk_kernel(
    const float *__restrict__ cand_score, const int32_t *__restrict__ cand_idx, int N,
    int per_class, int H, int W, int K, int C, const EmitArgs ea)
{
    constexpr bool CTDET = (MODE != MODE_CHANNEL);  // group = image, class from position
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    const int HW = H * W;
    const float *cs = cand_score + (size_t)g * N;
    const int32_t *ci = cand_idx + (size_t)g * N;

    u64 prefix, mask;
    auto for_each = [&](auto &&f) {
        for (int j = tid; j < N; j += NTM) {
            const int32_t idx = ci[j];
            if (idx < 0) continue;
            const uint32_t kk = f2key(cs[j] + 0.0f);
            const uint32_t fid = CTDET ? (uint32_t)((j / per_class) * HW + idx) : (uint32_t)idx;
            f(((u64)kk << 32) | (u64)(0xFFFFFFFFu - fid), kk == KEY_ZERO);
        }
    };
    radix_select<NTM>(for_each, (uint32_t)K, sh, prefix, mask);
    collect_and_sort<NTM>(for_each, prefix, mask, sh);
    emit_rows<MODE>(sh, g, H, W, K, C, ea);
}

// ---------------------------------------------------------------------------
// Second (and last) launch of the image-level decode: one workgroup per (image, class) plane
//   1. image_threshold  -- every plane of an image derives the same threshold from the group maxima
//                          of launch 1 (no wait between workgroups);
//   2. plane_collect    -- the plane's candidate keys;
//   3. the LAST plane of an image to arrive (one atomic counter per image; nobody waits for anybody)
//      selects and sorts the image's K best candidates and writes its detections.
// Degenerate images and saturated plateaus are dealt with plane by plane in plane_collect (every
// plane hands on at most its K best keys): the last arriver always finds between K and C * K keys.
// ---------------------------------------------------------------------------

template <int MODE>
__global__ __launch_bounds__(NT) void collect_merge_kernel(const float *__restrict__ heat, int C, int H,
                                                           int W, int nrg, int ncb, int flags, int K,
                                                           const uint32_t *__restrict__ gpeak,
                                                           const uint32_t *__restrict__ gall,
                                                           u64 *__restrict__ keys, int cap,
                                                           int32_t *__restrict__ counts,
                                                           int32_t *__restrict__ done, const EmitArgs ea)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)C);
    const int ng = C * nrg * ncb;
    float rthr;
    const uint32_t tkey = image_threshold(gpeak + (size_t)b * ng, ng, K, flags, sh, rthr);
    plane_collect(heat, C, H, W, nrg, ncb, flags, K, gall, tkey, rthr, sh, keys, cap, counts);
    // ---- arrival.  What the image's last workgroup reads from the others -- candidate keys and their
    // count -- is written with device-scope atomics (write-through to the coherence point) and read
    // with device-scope loads: no __threadfence() on either side (on this part a device-scope release /
    // acquire is a write-back / invalidate of the whole L2 of the XCD; 2560 workgroups doing that cost
    // 0.18 ms).  Order: every wave waits for the acknowledgement of its stores, the workgroup
    // meets, then ONE thread bumps the image's counter.
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
        s_last = (__hip_atomic_fetch_add(&done[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == C - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    // every plane handed on its K best (or all it had): between K and C * K keys, the image's K best
    // among them (fewer than K only when the whole image has fewer cells: excluded by the caller)
    const int cnt = min(__hip_atomic_load(&counts[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), cap);
    const u64 *kg = keys + (size_t)b * cap;
    u64 prefix, mask;
    constexpr int RK = 16;
    if (cnt <= RK * NT) {
        // fetched once into registers (16 per thread), device-scope loads
        u64 kr[RK];
#pragma unroll
        for (int u = 0; u < RK; ++u)
            kr[u] = (tid + u * NT < cnt) ? __hip_atomic_load(kg + tid + u * NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                         : 0ull;
        auto for_each = [&](auto &&f) {
#pragma unroll
            for (int u = 0; u < RK; ++u)
                if (tid + u * NT < cnt) f(kr[u], (uint32_t)(kr[u] >> 32) == KEY_ZERO);
        };
        radix_select<NT>(for_each, (uint32_t)K, sh, prefix, mask);
        collect_and_sort<NT>(for_each, prefix, mask, sh);
    } else {
        auto for_each = [&](auto &&f) {
            for (int j = tid; j < cnt; j += NT) {
                const u64 k = __hip_atomic_load(kg + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                f(k, (uint32_t)(k >> 32) == KEY_ZERO);
            }
        };
        radix_select<NT>(for_each, (uint32_t)K, sh, prefix, mask);
        collect_and_sort<NT>(for_each, prefix, mask, sh);
    }
    emit_rows<MODE>(sh, b, H, W, K, C, ea);
}

// ---------------------------------------------------------------------------
// ONE-launch form of the image-level decode (round 4): planes of at most 128 x 128 cells -- the
// ctdet map of a 512 x 512 input and everything smaller.  The heat-map is read exactly ONCE: a
// workgroup of eight waves owns one (image, class) plane and holds it in REGISTERS -- half-wave u
// keeps rows 8u .. 8u+7 (+ one halo row above and below, from L2), lane l the 4-cell quad l of every
// row -- so the logistic, the 3x3 peak test on the scores (decode.py:9-15) and every later look at a
// cell are register work; horizontal neighbours come from the adjacent lanes by shuffle.  Then
//   1. every lane takes the largest key of its 32 cells; T0 = the K-th largest of the 512 lane maxima
//      to OP_TBITS bits (ONE wave, the maxima in its registers, a binary search on wave ballots: no
//      histogram, no barrier inside).  At least K cells of the plane reach T0, so nothing below it
//      can be among the plane's -- or the image's -- K best.  T0 is folded into the image's FLOOR (a
//      device-scope atomic maximum): planes that start later skip every cell below the best T0
//      published so far.  Workgroups run class-major (all images' plane 0, then plane 1, ...): an
//      image's planes are spread over the launch and most of them find a floor;
//   2. the cells that reach max(T0, floor) go into a list in LDS; up to OP_PE keys go as they are
//      into the plane's OWN slot of the image's key buffer (no position to fetch from a counter: one
//      device-scope round trip less), a longer list goes through the exact select of the plane's K
//      best, and a list that overflows LDS (plateaus, tiny or constant maps: T0 useless) through the
//      same select over the register cells, zeros of suppressed cells included;
//   3. arrival as in collect_merge_kernel; the last arriver reads the planes' key counts, keeps the
//      keys that reach the image's FINAL floor (a few hundred: in LDS), selects and sorts the K best
//      and writes the detections.  It leaves the image's state words (arrival counter, floor) at zero.
// Every input is handled exactly inside this launch; results are bit-identical to the two-launch
// and the per-band forms (tests/test_gpu_decode.py).
// ---------------------------------------------------------------------------
constexpr int OP_NT = 512;        // threads (8 waves)
constexpr int OP_ROWS = 8;        // rows a half-wave owns
constexpr int OP_CELLS = OP_ROWS * 4;
constexpr int OP_PE = 256;        // key slots of a plane in the image's buffer (>= KMAX)
constexpr int OP_RK = 40;         // key slots per thread the last arriver keeps in registers (80 planes)
constexpr int OP_CMAX = 1024;     // classes (the planes' key counts sit in LDS)
constexpr int OP_TBITS = 16;      // leading key bits T0 is resolved to
static_assert(OP_PE >= KMAX && OP_PE <= PLCAP, "plane emit cap");
static_assert((OP_PE & (OP_PE - 1)) == 0 && OP_NT * 4 % OP_PE == 0, "slot arithmetic");

#ifdef CN_ABLATE_DECODE       // variant builds only (tools/build_variant.sh): leave after stage (flags >> 16) & 15
#define PSM_STAGE_EXIT(n, keep)                                                         \
    if (((flags >> 16) & 15) == (n)) {                                                  \
        if ((keep) == 0xdeadbeefu) floorv[b] = 1u;                                      \
        return;                                                                         \
    }
#else
#define PSM_STAGE_EXIT(n, keep)
#endif

// The image's last arriver of plane_select_merge_kernel (its own function, not inlined: 80 registers of
// keys must not weigh on the allocation of the plane part every workgroup runs).
template <int MODE>
__device__ __attribute__((noinline)) void psm_last_arriver(SelShared &sh, int32_t *s_pc, uint32_t *s_kmax_p, int b,
                                                           int C, int H, int W, int K,
                                                           const u64 *__restrict__ keys,
                                                           const int32_t *__restrict__ pcount,
                                                           const uint32_t *__restrict__ floorv, const EmitArgs ea)
{
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1);
    uint32_t &s_kmax = *s_kmax_p;
    // every plane's floor update precedes its arrival: this is the image's final floor, and the
    // image's K best all reach it (the plane that set it has K cells there and handed them on)
    const uint32_t F = max(__hip_atomic_load(&floorv[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 1u);
    for (int p = tid; p < C; p += OP_NT)
        s_pc[p] = __hip_atomic_load(&pcount[(size_t)b * C + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) s_kmax = 0u;
    for (int i = tid; i < HBINS; i += OP_NT) sh.hist[i] = 0;
    __syncthreads();
    const u64 *kimg = keys + (size_t)b * C * OP_PE;
    const int slots = C * OP_PE;
    u64 prefix, mask;
    if (slots <= OP_NT * OP_RK) {
        // Every key of the image in registers, ONE round trip to the coherence point.  Then a LINEAR
        // histogram of the score keys over [F, largest key] (2048 bins: order-preserving integers, so
        // the bin that holds the K-th largest is exact) leaves the keys of that bin and above -- K plus
        // a few -- which are sorted as they are; a plateau that fills the bin goes through the digit
        // select.
        u64 kr[OP_RK];
#pragma unroll
        for (int u = 0; u < OP_RK; ++u) {
            const int i = tid + u * OP_NT;
            const bool ok = i < slots && (i & (OP_PE - 1)) < s_pc[min(i, slots - 1) / OP_PE];
            kr[u] = ok ? __hip_atomic_load(kimg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
        uint32_t mx = 0u;
#pragma unroll
        for (int u = 0; u < OP_RK; ++u) {
            const uint32_t sk = (uint32_t)(kr[u] >> 32);
            if (sk < F) kr[u] = 0ull;                            // (and the empty slots: key 0)
            else mx = max(mx, sk);
        }
#pragma unroll
        for (int o = CN_WAVE / 2; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        if (lane == 0 && mx) atomicMax(&s_kmax, mx);
        __syncthreads();
        const uint32_t range = max(s_kmax, F) - F;
        const int shift = max(0, 21 - __clz((int)(range | 1u)));      // (range >> shift) < 2048
#pragma unroll
        for (int u = 0; u < OP_RK; ++u)
            if (kr[u]) atomicAdd(&sh.hist[((uint32_t)(kr[u] >> 32) - F) >> shift], 1u);
        __syncthreads();
        suffix_bin<OP_NT>((uint32_t)K, sh);                      // sh.digit: the bin, sh.bincount: keys in it and above
        const uint32_t F1 = F + (sh.digit << shift);
        const uint32_t kept = sh.bincount;
        auto for_each = [&](auto &&f) {
#pragma unroll
            for (int u = 0; u < OP_RK; ++u) {
                const uint32_t sk = (uint32_t)(kr[u] >> 32);
                if (sk >= F1) f(kr[u], sk == KEY_ZERO);
            }
        };
        if (kept <= (uint32_t)KMAX) {
            collect_and_sort<OP_NT>(for_each, 0ull, 0ull, sh);   // all of them
        } else {
            radix_select<OP_NT>(for_each, (uint32_t)K, sh, prefix, mask);
            collect_and_sort<OP_NT>(for_each, prefix, mask, sh);
        }
    } else {                                 // (more planes than the registers take: straight from the slots)
        auto for_each = [&](auto &&f) {
            for (int i = tid; i < slots; i += OP_NT) {
                if ((i & (OP_PE - 1)) < s_pc[i / OP_PE]) {
                    const u64 k = __hip_atomic_load(kimg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((uint32_t)(k >> 32) >= F) f(k, (uint32_t)(k >> 32) == KEY_ZERO);
                }
            }
        };
        radix_select<OP_NT>(for_each, (uint32_t)K, sh, prefix, mask);
        collect_and_sort<OP_NT>(for_each, prefix, mask, sh);
    }
    emit_rows<MODE>(sh, b, H, W, K, C, ea);
}

#ifndef CN_PSM_WAVES
#define CN_PSM_WAVES 4        // waves per SIMD the register budget is cut for (two workgroups per CU)
#endif
template <int MODE>
__global__ __launch_bounds__(OP_NT, CN_PSM_WAVES) void plane_select_merge_kernel(const float *__restrict__ heat, int B, int C,
                                                                      int H, int W, int flags, int K,
                                                                      u64 *__restrict__ keys,
                                                                      int32_t *__restrict__ pcount,
                                                                      int32_t *__restrict__ done,
                                                                      uint32_t *__restrict__ floorv, const EmitArgs ea)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    __shared__ u64 kbuf[PLCAP];             // the plane's list
    __shared__ uint32_t s_lmax[OP_NT / 2];
    __shared__ int32_t s_pc[OP_CMAX];
    __shared__ int pl_cnt, s_last;
    __shared__ uint32_t s_thr, s_kmax;
    const int tid = threadIdx.x;
    const int lane = tid & (CN_WAVE - 1);
    const int hl = lane & 31, hw = tid >> 5;
    int b, c;
    // planes class by class (all images' plane 0, then plane 1, ...): an image's planes are spread over the
    // launch and most of them find a floor.  (Round 4 A/B, removed in round 5: image by image +40 % time;
    // class-major in blocks of eight classes +9 % warm, -19 % cold -- DESIGN.md 3.4.)
    c = (int)(blockIdx.x / (unsigned)B);
    b = (int)blockIdx.x - c * B;
    const size_t plane_id = (size_t)b * C + c;
    const bool sig = (flags & 1) != 0;
    const bool nonms = (flags & CN_DECODE_NO_PEAK_TEST) != 0;
    const int HW = H * W;
    const float *plane = heat + plane_id * (size_t)HW;
    const uint32_t base = (uint32_t)c * (uint32_t)HW;
    const int w4 = W >> 2;
    // the image's floor so far: requested first, lands under the map loads
    uint32_t fl = 0u;
    if (tid == 0) fl = __hip_atomic_load(&floorv[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // ---- the plane into registers: rows y0-1 .. y0+8 of this half-wave, all loads issued up front
    const int y0 = hw * OP_ROWS;
    const bool col_ok = hl < w4;
    const int nv = col_ok ? min(max(H - y0, 0), OP_ROWS) : 0;    // valid rows of this lane's 8
    // (branch-free: rows / quads outside the map read a clamped address and are replaced below)
    cn_f32x4 rowv[OP_ROWS + 2];
    {
        const uint32_t xoff = col_ok ? (uint32_t)hl * 4u : 0u;
#pragma unroll
        for (int r = 0; r < OP_ROWS + 2; ++r) {
            const int yc = min(max(y0 - 1 + r, 0), H - 1);
            rowv[r] = *reinterpret_cast<const cn_f32x4 *>(plane + ((uint32_t)yc * (uint32_t)W + xoff));
        }
    }
#ifdef CN_ABLATE_DECODE
    if (((flags >> 16) & 15) == 1) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < OP_ROWS + 2; ++r) acc += rowv[r].x + rowv[r].y + rowv[r].z + rowv[r].w;
        if (acc == 123.456f) floorv[b] = 1u;
        return;
    }
#endif
    // (selections below are written as bit masks: left as ?: the compiler wraps every transcendental
    // and every shuffle fix-up in its own branch)
    const uint32_t NINF = 0xff800000u;
    auto sel = [](uint32_t msk, float a, float bfl) -> float {   // msk ? a : b, bitwise
        return __uint_as_float((__float_as_uint(a) & msk) | (__float_as_uint(bfl) & ~msk));
    };
    // scores of a window row; cells outside the map stay -inf (the peak test's padding, decode.py:12)
    auto score_row = [&](int r) {
        const int y = y0 - 1 + r;
        const uint32_t in_map = (col_ok && y >= 0 && y < H) ? 0xffffffffu : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = rowv[r][e];
            rowv[r][e] = sel(in_map, sig ? sigmoidf_ref(x) : x, __uint_as_float(NINF));
        }
    };
    // horizontal 3-max of a row (neighbour quads by shuffle inside the half-wave)
    const uint32_t has_l = (hl != 0 && col_ok) ? 0xffffffffu : 0u;
    const uint32_t has_r = (hl != 31 && col_ok) ? 0xffffffffu : 0u;
    auto hrow = [&](int r) -> cn_f32x4 {
        const float l = sel(has_l, __shfl_up(rowv[r].w, 1, 32), __uint_as_float(NINF));
        const float rr = sel(has_r, __shfl_down(rowv[r].x, 1, 32), __uint_as_float(NINF));
        cn_f32x4 h;
        h.x = fmaxf(fmaxf(l, rowv[r].x), rowv[r].y);
        h.y = fmaxf(fmaxf(rowv[r].x, rowv[r].y), rowv[r].z);
        h.z = fmaxf(fmaxf(rowv[r].y, rowv[r].z), rowv[r].w);
        h.w = fmaxf(fmaxf(rowv[r].z, rowv[r].w), rr);
        return h;
    };
    // the 32 cells of this lane as keys of heat * keep (decode.py:14; -0.0 -> +0.0); cell i = row
    // y0 + (i >> 2), column 4 hl + (i & 3).  Cells outside the map get key 0, which no threshold
    // admits (thresholds are >= 1; a cell of the map has key 0 only for one NaN pattern).  A row's
    // registers die as soon as the row below it has been combined.
    uint32_t kreg[OP_CELLS];
    {
        score_row(0);
        score_row(1);
        cn_f32x4 h0 = hrow(0), h1 = hrow(1);
#pragma unroll
        for (int r = 1; r <= OP_ROWS; ++r) {
            score_row(r + 1);
            const cn_f32x4 h2 = hrow(r + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = rowv[r][e];
                const float m = fmaxf(fmaxf(h0[e], h1[e]), h2[e]);
                const uint32_t k = f2key(((nonms || m == v) ? v : 0.0f) + 0.0f);
                kreg[(r - 1) * 4 + e] = (r - 1 < nv) ? k : 0u;
            }
            h0 = h1;
            h1 = h2;
        }
    }
    auto key64 = [&](int i) -> u64 {
        const uint32_t cell = (uint32_t)((y0 + (i >> 2)) * W + hl * 4 + (i & 3));
        return ((u64)kreg[i] << 32) | (u64)(0xFFFFFFFFu - (base + cell));
    };

    // ---- 1. T0 = K-th largest lane maximum, to OP_TBITS bits (0: fewer than K lanes hold a cell --
    // small maps: every cell of the map is admitted)
    uint32_t lmax = 0u;
#pragma unroll
    for (int i = 0; i < OP_CELLS; ++i) lmax = max(lmax, kreg[i]);
    PSM_STAGE_EXIT(2, lmax)
    // (a lane and its partner in the other half-wave count as one: 256 values, each the key of one cell)
    const uint32_t pmax = max(lmax, (uint32_t)__shfl_xor((int)lmax, 32));
    if (lane < 32) s_lmax[(tid >> 6) * 32 + lane] = pmax;
    if (tid == 0) pl_cnt = 0;
    __syncthreads();
    if (tid < CN_WAVE) {
        // ONE wave searches while seven wait: it goes first on its SIMD
        __builtin_amdgcn_s_setprio(3);
        constexpr int NV = OP_NT / 2 / CN_WAVE;
        uint32_t v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = s_lmax[lane + j * CN_WAVE];
        uint32_t T0 = 0u;
#pragma unroll
        for (int bit = 31; bit >= 32 - OP_TBITS; --bit) {
            const uint32_t cand = T0 | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j) cnt += __popcll(__ballot(v[j] >= cand));
            if (cnt >= K) T0 = cand;
        }
        if (tid == 0) {
            s_thr = max(max(T0, fl), 1u);
            if (T0 > fl) __hip_atomic_fetch_max(&floorv[b], T0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    const uint32_t thr = s_thr;
    PSM_STAGE_EXIT(3, thr)

    // ---- 2. cells that reach thr -> LDS list (half-wave prefix sums, one LDS atomic per half-wave)
    uint32_t m0 = 0u;
#pragma unroll
    for (int i = 0; i < OP_CELLS; ++i) m0 |= (kreg[i] >= thr) ? (1u << i) : 0u;
    {
        const int mine = __popc(m0);
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int t = __shfl_up(incl, o, 32);
            if (hl >= o) incl += t;
        }
        const int total = __shfl(incl, 31, 32);
        int pos0 = 0;
        if (hl == 31 && total) pos0 = atomicAdd(&pl_cnt, total);
        int pos = __shfl(pos0, 31, 32) + incl - mine;
        if (mine) {
#pragma unroll
            for (int i = 0; i < OP_CELLS; ++i) {
                if ((m0 >> i) & 1u) {
                    if (pos < PLCAP) kbuf[pos] = key64(i);
                    ++pos;
                }
            }
        }
    }
    __syncthreads();
    const int n = pl_cnt;                    // (uniform)
    PSM_STAGE_EXIT(4, (uint32_t)n)
    int m;
    const u64 *src;
    if (n <= OP_PE) {
        m = n;
        src = kbuf;
    } else {
        m = K;                               // n > OP_PE >= K cells reach thr: the plane's K best are among them
        u64 prefix, mask;
        if (n <= PLCAP) {
            auto for_each = [&](auto &&f) {
                for (int j = tid; j < n; j += OP_NT) f(kbuf[j], false);
            };
            radix_select<OP_NT>(for_each, (uint32_t)m, sh, prefix, mask);
            collect_and_sort<OP_NT>(for_each, prefix, mask, sh);
        } else {
            auto for_each = [&](auto &&f) {
#pragma unroll
                for (int i = 0; i < OP_CELLS; ++i)
                    if (kreg[i] >= thr) f(key64(i), kreg[i] == KEY_ZERO);
            };
            radix_select<OP_NT>(for_each, (uint32_t)m, sh, prefix, mask);
            collect_and_sort<OP_NT>(for_each, prefix, mask, sh);
        }
        src = sh.sel;
    }
    // the plane's own slot: nothing to fetch before the stores can go
    u64 *kslot = keys + plane_id * OP_PE;
    for (int j = tid; j < m; j += OP_NT) __hip_atomic_store(kslot + j, src[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) __hip_atomic_store(&pcount[plane_id], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    PSM_STAGE_EXIT(5, (uint32_t)m)

    // ---- 3. arrival (see collect_merge_kernel for the memory-ordering argument)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
        s_last = (__hip_atomic_fetch_add(&done[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == C - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    PSM_STAGE_EXIT(6, (uint32_t)m)
    psm_last_arriver<MODE>(sh, s_pc, &s_kmax, b, C, H, W, K, keys, pcount, floorv, ea);
    // the image's state words go back to zero: the next call on this workspace needs no fill
    // (device-scope stores: the words of other images share these cache lines and are being updated
    // by atomics from other XCDs)
    if (tid == 0) {
        __hip_atomic_store(&done[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&floorv[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the launches of a routed call; the image-level kernels exist for the modes that rank all classes of an image
template <int MODE>
int topk_launch(const TopkCall &c, const TopkPlan &p)
{
    char *ws = (char *)c.workspace;
    const int B = c.B, C = c.C, H = c.H, W = c.W, K = c.K;
    if constexpr (MODE == MODE_CTDET || MODE == MODE_TOPK) {
        if (p.form == TOPK_ONE_LAUNCH || p.form == TOPK_TWO_LAUNCHES) {
            uint32_t *gpeak = (uint32_t *)(ws + p.gpeak);
            uint32_t *gall = (uint32_t *)(ws + p.gall);
            int32_t *counts = (int32_t *)(ws + p.counts);
            int32_t *done = (int32_t *)(ws + p.done);
            u64 *keys = (u64 *)(ws + p.keys);
            dim3 grid((unsigned)(B * C)), block(NT);
            if (p.form == TOPK_ONE_LAUNCH) {
                // The image state words (arrival counter, floor) must be zero on entry and are left at zero
                // by the kernel: a caller that keeps the workspace to itself says so (CN_DECODE_STATE_CLEAN)
                // after zeroing it once; anyone else pays a small fill.
                if (p.fill_state) {
                    if (hipMemsetAsync(ws + p.state_offset, 0, p.state_bytes, c.st) != hipSuccess) return CN_ERR_LAUNCH;
                }
                hipLaunchKernelGGL(plane_select_merge_kernel<MODE>, grid, dim3(OP_NT), sizeof(SelShared), c.st,
                                   c.heat, B, C, H, W, c.flags, K, keys, (int32_t *)(ws + p.pcount), done,
                                   (uint32_t *)(ws + p.floorv), c.ea);
                CN_CHECK_LAUNCH();
                return CN_OK;
            }
            hipLaunchKernelGGL(group_max_kernel, grid, block, 0, c.st, c.heat, H, W, p.nrg, p.ncb, c.flags, gpeak,
                               gall, C, counts, done);
            CN_CHECK_LAUNCH();
            hipLaunchKernelGGL(collect_merge_kernel<MODE>, grid, block, sizeof(SelShared), c.st, c.heat, C, H, W,
                               p.nrg, p.ncb, c.flags, K, gpeak, gall, keys, p.cap, counts, done, c.ea);
            CN_CHECK_LAUNCH();
            return CN_OK;
        }
    }
    // per band; with one band per plane the channel lists are final as the select writes them
    const bool direct = p.form == TOPK_BAND_DIRECT;
    float *cand_score = direct ? c.ea.out_scores : (float *)(ws + p.cand_score);
    int32_t *cand_idx = direct ? c.ea.inds_out : (int32_t *)(ws + p.cand_idx);
    CN_SET_MAX_LDS_ONCE(nms_topk_kernel, 160 * 1024);
    hipLaunchKernelGGL(nms_topk_kernel, dim3(p.nbands, C, B), dim3(NT), p.lds, c.st, c.heat, C, H, W, K, p.R,
                       c.flags, cand_score, cand_idx);
    CN_CHECK_LAUNCH();
    if (direct) return CN_OK;
    const int per_class = p.nbands * K;
    constexpr bool per_channel = MODE == MODE_CHANNEL;   // one group per (image, channel), else per image
    hipLaunchKernelGGL(merge_topk_kernel<MODE>, dim3(per_channel ? B * C : B), dim3(NTM), sizeof(SelShared), c.st,
                       cand_score, cand_idx, per_channel ? per_class : C * per_class, per_class, H, W, K, C, c.ea);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace

// Which form a top-K call takes and where its scratch lives: a deterministic function of the shapes, the mode
// and the flags (workspace query == launch).
TopkPlan topk_route(const TopkCall &c)
{
    TopkPlan p = {};
    const int B = c.B, C = c.C, H = c.H, W = c.W, K = c.K;
    p.rc = CN_ERR_SHAPE;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return p;
    p.rc = CN_ERR_UNSUPPORTED;
    // ---- band geometry of the per-band select.  Bands of <= 8192 cells: tile + list + select state stay
    // under ~52 KB, so three workgroups share a CU and their load / peak-test / select phases overlap.
    if (W > 4096) return p;
    int R = 8192 / W;
    if (R < 1) R = 1;
    if (R > H) R = H;
    while (R < H && R * W < K) ++R;  // a band should be able to supply K candidates
    if ((long)R * W > 16384) return p;
    p.R = R;
    p.nbands = cn_cdiv(H, R);
    p.lds = sizeof(SelShared) + (size_t)(R + 2) * W * sizeof(float) + CAND_CAP * sizeof(uint16_t);
    if (p.lds > 160 * 1024) return p;
    p.rc = CN_OK;
    // ---- workspace: the per-band candidate arrays, the image-level scratch behind them.  One layout for
    // every mode and flag: what a query answers holds for whatever form the call then takes.
    const size_t n = (size_t)B * C * p.nbands * K;
    size_t o = 0;
    p.cand_score = o; o += cn_align_up(n * sizeof(float), 256);
    p.cand_idx = o;   o += cn_align_up(n * sizeof(int32_t), 256);
    p.cand_bytes = o;
    p.nrg = cn_cdiv(H, GROWS);
    p.ncb = cn_cdiv(W, 128);
    // enough groups per image for a meaningful threshold; rows of whole quads
    const bool use = (W & 3) == 0 && (long)C * p.nrg * p.ncb >= 4L * K;
    // planes of <= 128 x 128 cells: plane_select_merge_kernel (ONE launch)
    const bool one_pass = use && H <= (OP_NT / 32) * OP_ROWS && W <= 128 && C <= OP_CMAX;
    const size_t ng = (size_t)B * C * p.nrg * p.ncb;
    p.gpeak = o;  o += cn_align_up(ng * 4, 256);
    p.gall = o;   o += cn_align_up(ng * 4, 256);
    p.counts = o; o += cn_align_up((size_t)B * 4, 256);
    p.done = o;   o += cn_align_up((size_t)B * 4, 256);
    p.floorv = o; o += cn_align_up((size_t)B * 4, 256);
    const size_t state_bytes = o - p.counts;   // counts | done | floorv: contiguous
    p.pcount = o; o += cn_align_up((size_t)B * C * 4, 256);   // keys in every plane's slot (one-launch form)
    p.cap = C * (one_pass ? OP_PE : K);        // every plane hands on at most its K best (its slot: OP_PE)
    p.keys = o;   o += cn_align_up((size_t)B * p.cap * 8, 256);
    p.total = o;
    // ---- the form
    // the image-level forms rank all classes of an image: single-class maps (the pose centre map) and the
    // per-channel lists keep the per-band select
    const bool image_mode = c.mode == MODE_CTDET || c.mode == MODE_TOPK;
    if (image_mode && use && !(c.flags & CN_DECODE_PER_BAND))   // (the flag: tests / A-B)
        p.form = (one_pass && !(c.flags & CN_DECODE_TWO_LAUNCHES)) ? TOPK_ONE_LAUNCH : TOPK_TWO_LAUNCHES;
    else   // one band per plane: the select already leaves the final sorted (B, C, K) channel lists
        p.form = (c.mode == MODE_CHANNEL && p.nbands == 1) ? TOPK_BAND_DIRECT : TOPK_BAND_MERGE;
    if (p.form == TOPK_ONE_LAUNCH) {
        p.state_offset = p.counts;
        p.state_bytes = state_bytes;
        p.fill_state = !(c.flags & CN_DECODE_STATE_CLEAN);
    }
    return p;
}

int topk_checks(const TopkCall &c)
{
    if (!c.heat) return CN_ERR_NULL;
    if (c.B <= 0 || c.C <= 0 || c.H <= 0 || c.W <= 0 || c.K <= 0) return CN_ERR_SHAPE;
    if ((long)c.K > (long)c.H * c.W) return CN_ERR_SHAPE;  // torch.topk: k out of range
    if (c.K > KMAX) return CN_ERR_UNSUPPORTED;
    if ((long)c.C * c.H * c.W >= (1L << 31)) return CN_ERR_UNSUPPORTED;
    const int rc = topk_route(c).rc;
    if (rc != CN_OK) return rc;
    if (((c.W & 3) == 0) && !cn_aligned16(c.heat)) return CN_ERR_ALIGN;
    return CN_OK;
}

int topk_run(const TopkCall &c)
{
    const int rc = topk_checks(c);
    if (rc != CN_OK) return rc;
    const TopkPlan p = topk_route(c);
    const EmitArgs &ea = c.ea;
    bool missing = false;   // an output the mode writes
    switch (c.mode) {
    case MODE_CTDET: missing = !ea.wh || !ea.dets; break;
    case MODE_POSE: missing = !ea.wh || !ea.kps_map || !ea.dets; break;
    case MODE_TOPK: missing = !ea.out_scores || !ea.inds_out || !ea.cls_out; break;
    case MODE_CHANNEL: missing = !ea.out_scores || !ea.inds_out; break;
    default: return CN_ERR_UNSUPPORTED;
    }
    if (missing) return CN_ERR_NULL;
    if (p.form != TOPK_BAND_DIRECT) {   // (the direct form touches no workspace)
        if (!c.workspace) return CN_ERR_NULL;
        if (c.workspace_bytes < (c.cand_only ? p.cand_bytes : p.total)) return CN_ERR_WORKSPACE;
    }
    switch (c.mode) {   // the one place a run-time mode becomes a template argument
    case MODE_CTDET: return topk_launch<MODE_CTDET>(c, p);
    case MODE_POSE: return topk_launch<MODE_POSE>(c, p);
    case MODE_TOPK: return topk_launch<MODE_TOPK>(c, p);
    default: return topk_launch<MODE_CHANNEL>(c, p);
    }
}

// the call of an entry: shapes, flags, mode and where it works; the entry adds its outputs
static TopkCall topk_call(const float *heat, int B, int C, int H, int W, int K, int flags, int mode,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    TopkCall c = {};
    c.heat = heat;
    c.B = B; c.C = C; c.H = H; c.W = W; c.K = K;
    c.flags = flags;
    c.mode = mode;
    c.workspace = workspace;
    c.workspace_bytes = workspace_bytes;
    c.st = (hipStream_t)stream;
    return c;
}

extern "C" size_t cn_ctdet_decode_workspace_bytes(int B, int C, int H, int W, int K)
{
    const TopkPlan p = topk_route(topk_call(nullptr, B, C, H, W, K, 0, MODE_CTDET, nullptr, 0, nullptr));
    return p.rc == CN_OK ? p.total : 0;
}

// Where the one-launch image-level decode keeps its per-image state words inside the workspace of
// cn_ctdet_decode_f32 / cn_topk_f32 (byte offset and size; 0 bytes when the shape takes another form).
// They are zero between calls: a caller that owns its workspace (CN_DECODE_STATE_CLEAN) can check or
// re-zero exactly this region after a failed call instead of trusting it.
extern "C" int cn_decode_state_region(int B, int C, int H, int W, int K, size_t *offset, size_t *bytes)
{
    if (!offset || !bytes) return CN_ERR_NULL;
    const TopkPlan p = topk_route(topk_call(nullptr, B, C, H, W, K, 0, MODE_CTDET, nullptr, 0, nullptr));
    *offset = p.state_offset;   // (0, 0 without a plan)
    *bytes = p.state_bytes;
    return p.rc;
}

extern "C" int cn_ctdet_decode_f32(const float *heat, const float *wh, const float *reg, int B,
                                   int C, int H, int W, int K, int cat_spec_wh, int apply_sigmoid,
                                   float *dets, int32_t *inds, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    TopkCall c = topk_call(heat, B, C, H, W, K, apply_sigmoid, MODE_CTDET, workspace, workspace_bytes, stream);
    c.ea.wh = wh;
    c.ea.reg = reg;
    c.ea.cat_spec_wh = cat_spec_wh;
    c.ea.dets = dets;
    c.ea.inds_out = inds;
    return topk_run(c);
}

extern "C" int cn_topk_f32(const float *heat, int B, int C, int H, int W, int K, int apply_sigmoid,
                           float *scores, int32_t *inds, int32_t *clses, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    TopkCall c = topk_call(heat, B, C, H, W, K, apply_sigmoid, MODE_TOPK, workspace, workspace_bytes, stream);
    c.ea.out_scores = scores;
    c.ea.inds_out = inds;
    c.ea.cls_out = clses;
    return topk_run(c);
}

extern "C" int cn_nms_topk_channel_f32(const float *heat, int B, int C, int H, int W, int K,
                                       int apply_sigmoid, float *scores, int32_t *inds,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    TopkCall c = topk_call(heat, B, C, H, W, K, apply_sigmoid, MODE_CHANNEL, workspace, workspace_bytes, stream);
    c.ea.out_scores = scores;
    c.ea.inds_out = inds;
    return topk_run(c);
}

// ---------------------------------------------------------------------------
// _transpose_and_gather_feat (models/utils.py:12-26)
// ---------------------------------------------------------------------------
namespace {

// out[b,k,c] = feat[b,c,ind[b,k]]  (NCHW map -> (B,K,C); replaces permute+contiguous+gather)
__global__ void gather_feat_kernel(const float *__restrict__ feat, const int32_t *__restrict__ inds,
                                   float *__restrict__ out, int C, int HW, int K, size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t bk = i / C;
    const size_t b = bk / K;
    // an index outside the map never reads out of bounds (the Python wrapper raises for it, as
    // torch.gather does; a raw C-ABI caller gets NaN in that row)
    const int32_t ind = inds[bk];
    out[i] = ((uint32_t)ind < (uint32_t)HW) ? feat[(b * C + c) * HW + ind]
                                             : __builtin_nanf("");
}

}  // namespace

extern "C" int cn_gather_feat_f32(const float *feat, const int32_t *inds, float *out, int B, int C,
                                  int H, int W, int K, void *stream)
{
    if (!feat || !inds || !out) return CN_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return CN_ERR_SHAPE;
    const size_t total = (size_t)B * K * C;
    hipLaunchKernelGGL(gather_feat_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, feat, inds, out, C, H * W, K, total);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

