// cn_tiles_pose.hip -- the tile merge of multi_pose run_tiles (cn_multi_pose_tiles_merge_f32;
// post_process.multi_pose_tiles_results is its host specification, bit for bit).  The task has one class, so a
// frame's survivors are ONE soft-NMS segment, and a 4K frame has thousands of them: more than the one-wave
// soft_nms_segment of cn_tail.hip holds (2048) and far more than one wave walks quickly.  Here one workgroup of
// sixteen waves owns a frame, in ONE launch:
//   A. filter + stable compaction: a row of tile t survives when its box centre lies in the tile's core (and,
//      with a min_score, score >= min_score).  Every wave owns a contiguous run of the frame's T * K rows in
//      whole steps of 64; ballot counts, the sum over the waves in front, ballot ranks -- the survivors' box,
//      score and source row index land in LDS in input order.  The 34 joint columns never enter LDS.
//   B. soft-NMS (Gaussian, sigma 0.5, threshold 0.001) with the arithmetic and the row moves of
//      soft_nms_segment<true>, the argmax and the decay shared by ALL waves.  Step i, rows [i, N) live:
//        argmax  every thread takes the rows i + t, i + t + 1024, ...; wave reduction, one (score, position) per
//                wave through LDS, every thread reduces the sixteen.  The first maximum wins.
//        decay   on the rows as they are BEFORE the argmax swap, which would otherwise need a barrier of its own:
//                the top row is read at bpos, and position bpos stands for row i (what the swap will put there).
//                Every wave takes aligned 64-row chunks, so the discard flags of a chunk are one ballot word.
//        walk    wave 0 alone, after the barrier: the swap, then from discard to discard through the ballot
//                words (a step without a discard, the common one, walks nothing).  N shrinks; broadcast.
//        The decayed scores go to the places their rows now occupy at the start of the next step's argmax, by
//        the thread that reads them there.  Three __syncthreads per step.  A segment of up to
//        CN_POSE_TILES_ONE_WAVE_ROWS rows runs the same steps on wave 0 alone, without the barriers: measured
//        faster there (profiles/run_tiles_pose.txt).
//   C. cut + gather: when more than max_per_frame rows are left, thresh = the max_per_frame-th largest score by
//      radix_select over distinct (score key, ~position) keys, as tiles_cut_kernel; then the ordered
//      compaction, the joints gathered once from the input through the source row index.
// LDS per survivor: 4 x 4 (box) + 4 (score) + 4 (decayed score) + 2 (source row) + 2 (start-of-step position)
// bytes and one ballot bit = 28.125 bytes, dynamic, sized for min(T * K, CN_POSE_TILES_MAX_ROWS) rows.
#include "cn_select.h"

// the float32 chains below are the host's operations one by one only without FMA contraction (see cn_tail.hip)
#pragma clang fp contract(off)

namespace {
constexpr int PT_THREADS = 1024;
constexpr int PT_WAVES = PT_THREADS / CN_WAVE;
constexpr int PT_ROW = 39;
constexpr int PT_CAP = CN_POSE_TILES_MAX_ROWS;
constexpr float PT_SIGMA = 0.5f, PT_THRESHOLD = 0.001f;
constexpr int PT_NONE = 0x7fffffff;
constexpr int PT_ONE_WAVE = CN_POSE_TILES_ONE_WAVE_ROWS;   // segments up to this long: soft-NMS by wave 0 alone
static_assert(PT_CAP % CN_WAVE == 0 && PT_CAP <= 65536, "positions are uint16_t, chunks are whole waves");
static_assert(CN_TILES_MAX_ROWS <= 65536, "source row indices are uint16_t");

struct PoseTilesLds {
    SelShared sel;
    float best[PT_WAVES];
    int bpos[PT_WAVES];
    int wsum[PT_WAVES];
    uint32_t low[PT_WAVES];
    int nlive;               // N after the step's walk
    int any;                 // the step's decay discarded a row
};

// rows of LDS for a frame of R rows, and the dynamic bytes they take
inline int pose_tiles_lds_rows(int R)
{
    const int up = (R + CN_WAVE - 1) / CN_WAVE * CN_WAVE;
    return up < PT_CAP ? up : PT_CAP;
}
inline size_t pose_tiles_lds_bytes(int cap) { return (size_t)cap * 28 + (size_t)cap / 8; }

// LDS written by one lane is read by the others of the same wave next: order the wave's own accesses
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// float division through double: the IEEE quotient whatever the device division flags are (cn_tail.hip)
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// Soft-NMS of the segment [0, n) in place (see the head of the file).  ALL: every wave of the workgroup calls it and
// shares the argmax and the decay, three __syncthreads per step; !ALL: wave 0 alone calls it (w == 0), the same
// step with the wave's own ordering in the barriers' place -- the faster form for a short segment, where the
// barriers and the trip through LDS cost more than fifteen more waves save (PT_ONE_WAVE).
template <bool ALL>
__device__ __forceinline__ void pose_soft_nms(float *x1, float *y1, float *x2, float *y2, float *sc, float *ns,
                                              uint16_t *jsrc, uint16_t *orig, u64 *dmask, PoseTilesLds &S, int n,
                                              int lane, int w)
{
    constexpr int STRIDE = ALL ? PT_THREADS : CN_WAVE;
    const int tid = w * CN_WAVE + lane;
    auto sync = [] {
        if (ALL) __syncthreads(); else wave_sync();
    };
    int N = n;
    bool pending = false;            // the decayed scores of the previous step are still in ns[]
    for (int i = 0; i < n && i < N; ++i) {
        // argmax over [i, N): the first maximum wins
        float best = 0.f;
        int bpos = PT_NONE;
        for (int p = i + tid; p < N; p += STRIDE) {
            float s;
            if (pending) {
                s = ns[orig[p]];
                sc[p] = s;
            } else {
                s = sc[p];
            }
            if (bpos == PT_NONE || s > best) { best = s; bpos = p; }
        }
        for (int off = CN_WAVE / 2; off > 0; off >>= 1) {
            const float s2 = __shfl_xor(best, off);
            const int p2 = __shfl_xor(bpos, off);
            if (p2 != PT_NONE && (bpos == PT_NONE || s2 > best || (s2 == best && p2 < bpos))) {
                best = s2;
                bpos = p2;
            }
        }
        if (ALL) {
            if (lane == 0) {
                S.best[w] = best;
                S.bpos[w] = bpos;
            }
            __syncthreads();
            best = S.best[0];
            bpos = S.bpos[0];
#pragma unroll
            for (int k = 1; k < PT_WAVES; ++k) {
                const float s2 = S.best[k];
                const int p2 = S.bpos[k];
                if (p2 != PT_NONE && (bpos == PT_NONE || s2 > best || (s2 == best && p2 < bpos))) {
                    best = s2;
                    bpos = p2;
                }
            }
        } else {
            wave_sync();                 // the scores written above are read by other lanes below
        }
        // the top row, where it lies before the swap
        const float tx1 = x1[bpos], ty1 = y1[bpos], tx2 = x2[bpos], ty2 = y2[bpos];
        // decay: every live row, as cn_soft_nms_f32 computes it; position bpos holds row i after the swap
        for (int base = ((i + 1) & ~(CN_WAVE - 1)) + w * CN_WAVE; base < N; base += STRIDE) {
            const int p = base + lane;
            const bool live = p > i && p < N;
            bool d = false;
            if (live) {
                const int q = p == bpos ? i : p;
                const float bx1 = x1[q], by1 = y1[q], bx2 = x2[q], by2 = y2[q];
                float s = sc[q];
                const float area = (float)(((double)(bx2 - bx1) + 1.0) * ((double)(by2 - by1) + 1.0));
                const float iw = (float)((double)(fminf(tx2, bx2) - fmaxf(tx1, bx1)) + 1.0);
                if (iw > 0) {
                    const float ih = (float)((double)(fminf(ty2, by2) - fmaxf(ty1, by1)) + 1.0);
                    if (ih > 0) {
                        const float ua = (float)((((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0) +
                                                  (double)area) - (double)(iw * ih));
                        const float ov = div_rn(iw * ih, ua);
                        const float weight = (float)exp((double)div_rn(-(ov * ov), PT_SIGMA));
                        s = weight * s;
                        d = s < PT_THRESHOLD;
                    }
                }
                ns[p] = s;
                orig[p] = (uint16_t)p;
            }
            const u64 m = __ballot(live && d);
            if (lane == 0) {
                dmask[base / CN_WAVE] = m;
                if (m) S.any = 1;            // (every writer writes 1)
            }
        }
        sync();
        if (w == 0) {
            if (lane == 0 && bpos != i) {
                float f;
                f = x1[i]; x1[i] = x1[bpos]; x1[bpos] = f;
                f = y1[i]; y1[i] = y1[bpos]; y1[bpos] = f;
                f = x2[i]; x2[i] = x2[bpos]; x2[bpos] = f;
                f = y2[i]; y2[i] = y2[bpos]; y2[bpos] = f;
                f = sc[i]; sc[i] = sc[bpos]; sc[bpos] = f;
                const uint16_t j = jsrc[i]; jsrc[i] = jsrc[bpos]; jsrc[bpos] = j;
            }
            if (S.any) {                     // (the same word for the whole wave)
                wave_sync();
                // walk: from discard to discard
                int pos = i + 1;
                while (pos < N) {
                    int p = -1;
                    for (int c0 = pos / CN_WAVE; c0 * CN_WAVE < N; c0 += CN_WAVE) {
                        const int c = c0 + lane, left = N - c * CN_WAVE;     // live rows from the chunk's first on
                        u64 word = left > 0 ? dmask[c] : 0ull;
                        if (c == pos / CN_WAVE) word &= ~0ull << (pos & (CN_WAVE - 1));
                        if (left > 0 && left < CN_WAVE) word &= (1ull << left) - 1ull;
                        const u64 has = __ballot(word != 0ull);
                        if (has) {
                            const int l = __builtin_ctzll(has);
                            const uint32_t lo = __shfl((uint32_t)word, l), hi = __shfl((uint32_t)(word >> 32), l);
                            p = (c0 + l) * CN_WAVE + __builtin_ctzll(((u64)hi << 32) | lo);
                            break;
                        }
                    }
                    if (p < 0) break;
                    // the row at p (a row that has not moved) is discarded; so is every row moved onto p
                    // after it that is itself discarded
                    for (;;) {
                        if (p == N - 1) {    // the last live row: it takes its own columns, N shrinks past it
                            if (lane == 0) sc[p] = ns[orig[p]];
                            N = p;
                            break;
                        }
                        const int last = N - 1;      // has not moved: orig[last] == last, old score
                        if (lane == 0) {
                            x1[p] = x1[last]; y1[p] = y1[last]; x2[p] = x2[last]; y2[p] = y2[last];
                            sc[p] = sc[last];
                            orig[p] = (uint16_t)last;
                            const uint16_t j = jsrc[p]; jsrc[p] = jsrc[last]; jsrc[last] = j;
                        }
                        N = last;
                        if (!((dmask[last / CN_WAVE] >> (last & (CN_WAVE - 1))) & 1ull)) break;
                    }
                    wave_sync();
                    pos = p + 1;
                }
                if (lane == 0) S.any = 0;
            }
            if (lane == 0) S.nlive = N;
        }
        sync();
        N = S.nlive;
        pending = true;              // rows [i + 1, N): read, and written to sc[], by the next step's argmax
    }
    // (the loop ends with i >= N: no live row is left whose decayed score is still to be written)
}

__global__ __launch_bounds__(PT_THREADS) void pose_tiles_merge_kernel(const float *__restrict__ rows, int T, int K,
                                                                      const float *__restrict__ cores, int do_nms,
                                                                      int max_per_frame, float min_score, int cap,
                                                                      float *__restrict__ out_rows,
                                                                      int32_t *__restrict__ out_counts,
                                                                      int32_t *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ PoseTilesLds S;
    float *x1 = reinterpret_cast<float *>(smem), *y1 = x1 + cap, *x2 = y1 + cap, *y2 = x2 + cap;
    float *sc = y2 + cap, *ns = sc + cap;
    uint16_t *jsrc = reinterpret_cast<uint16_t *>(ns + cap), *orig = jsrc + cap;
    u64 *dmask = reinterpret_cast<u64 *>(orig + cap);
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    const int R = T * K;
    const float *fr = rows + (size_t)b * R * PT_ROW;
    const bool use_min = min_score == min_score;         // NaN: no score test

    // ---- A. filter and stable compaction
    // cx = (x1 + x2) * 0.5f, lo <= cx < hi in float32: the host's comparison; a NaN centre or score fails it
    auto passes = [&](int e) -> bool {
        const float *s = fr + (size_t)e * PT_ROW;
        const float *co = cores + (size_t)(e / K) * 4;
        const float cx = (s[0] + s[2]) * 0.5f, cy = (s[1] + s[3]) * 0.5f;
        bool ok = cx >= co[0] && cx < co[2] && cy >= co[1] && cy < co[3];
        if (use_min) ok = ok && s[4] >= min_score;
        return ok;
    };
    const int per = (R + PT_THREADS - 1) / PT_THREADS * CN_WAVE;
    const int w0 = min(w * per, R), w1 = min(w0 + per, R);
    int cnt = 0;
    for (int base = w0; base < w1; base += CN_WAVE) {
        const int e = base + lane;
        cnt += __popcll(__ballot(e < w1 && passes(e)));
    }
    if (lane == 0) S.wsum[w] = cnt;
    if (t == 0) S.any = 0;
    __syncthreads();
    int run = 0, n = 0;
#pragma unroll
    for (int k = 0; k < PT_WAVES; ++k) {
        const int v = S.wsum[k];
        if (k < w) run += v;
        n += v;
    }
    if (n > cap) {                       // the same word for every thread: the whole workgroup leaves
        if (t == 0) {
            status[b] = 1;
            out_counts[b] = 0;
        }
        return;
    }
    if (t == 0) status[b] = 0;
    for (int base = w0; base < w1; base += CN_WAVE) {
        const int e = base + lane;
        const bool ok = e < w1 && passes(e);
        const u64 m = __ballot(ok);
        if (ok) {
            const int pos = run + __popcll(m & ((1ull << lane) - 1ull));
            const float *s = fr + (size_t)e * PT_ROW;
            x1[pos] = s[0];
            y1[pos] = s[1];
            x2[pos] = s[2];
            y2[pos] = s[3];
            sc[pos] = s[4];
            jsrc[pos] = (uint16_t)e;
        }
        run += __popcll(m);
    }
    __syncthreads();

    // ---- B. soft-NMS of the segment [0, n)
    if (do_nms && n > 1) {
        if (n > PT_ONE_WAVE)
            pose_soft_nms<true>(x1, y1, x2, y2, sc, ns, jsrc, orig, dmask, S, n, lane, w);
        else if (w == 0)
            pose_soft_nms<false>(x1, y1, x2, y2, sc, ns, jsrc, orig, dmask, S, n, lane, 0);
        __syncthreads();
    }

    // ---- C. cut and gather
    const bool cut = n > max_per_frame;
    float thresh = 0.f;
    if (cut) {                           // (the same for every thread)
        auto for_each = [&](auto &&f) {
            for (int r = t; r < n; r += PT_THREADS) {
                const uint32_t k = f2key(sc[r]);
                f(((u64)k << 32) | (uint32_t)~(uint32_t)r, k == KEY_ZERO);
            }
        };
        u64 prefix, mask;
        radix_select<PT_THREADS>(for_each, (uint32_t)max_per_frame, S.sel, prefix, mask);
        uint32_t low = 0xffffffffu;
        for_each([&](u64 k, bool) {
            if ((k & mask) >= prefix) low = min(low, (uint32_t)(k >> 32));
        });
        for (int o = CN_WAVE / 2; o > 0; o >>= 1) low = min(low, (uint32_t)__shfl_xor((int)low, o));
        if (lane == 0) S.low[w] = low;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PT_WAVES; ++k) low = min(low, S.low[k]);
        thresh = key2f(low);
    }
    // order-preserving compaction: a contiguous chunk of rows per thread, the scan of the chunks' counts
    const int chunk = (n + PT_THREADS - 1) / PT_THREADS, r0 = min(t * chunk, n), r1 = min(r0 + chunk, n);
    int keep = 0;
    for (int r = r0; r < r1; ++r) keep += (!cut || sc[r] >= thresh) ? 1 : 0;
    int incl = keep;
    for (int o = 1; o < CN_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    __syncthreads();                     // wsum[] of phase A has been read
    if (lane == CN_WAVE - 1) S.wsum[w] = incl;
    __syncthreads();
    int at = incl - keep, kept = 0;
#pragma unroll
    for (int k = 0; k < PT_WAVES; ++k) {
        const int v = S.wsum[k];
        if (k < w) at += v;
        kept += v;
    }
    int *dst = reinterpret_cast<int *>(ns);
    for (int r = r0; r < r1; ++r) dst[r] = (!cut || sc[r] >= thresh) ? at++ : -1;
    __syncthreads();
    if (t == 0) out_counts[b] = kept;
    float *ob = out_rows + (size_t)b * R * PT_ROW;
    for (int e = t; e < n * PT_ROW; e += PT_THREADS) {
        const int r = e / PT_ROW, c = e - r * PT_ROW, d = dst[r];
        if (d < 0) continue;
        float v;
        if (c == 0) v = x1[r];
        else if (c == 1) v = y1[r];
        else if (c == 2) v = x2[r];
        else if (c == 3) v = y2[r];
        else if (c == 4) v = sc[r];
        else v = fr[(size_t)jsrc[r] * PT_ROW + c];
        ob[(size_t)d * PT_ROW + c] = v;
    }
}
}  // namespace

// Nothing lies in global memory between the stages: the workspace is the interface's, for a form of the merge
// that splits into launches; one 16-byte unit is asked for so that the argument checks are the ctdet entry's.
extern "C" size_t cn_multi_pose_tiles_merge_workspace_bytes(int B, int T, int K)
{
    if (B <= 0 || T <= 0 || K <= 0) return 0;
    return 16;
}

extern "C" int cn_multi_pose_tiles_merge_f32(const float *rows, int B, int T, int K, const float *cores_dev,
                                             int apply_nms, int max_per_frame, float min_score, float *out_rows,
                                             int32_t *out_counts, int32_t *status, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    if (!rows || !cores_dev || !out_rows || !out_counts || !status || !workspace) return CN_ERR_NULL;
    if (B <= 0 || T < 1 || K <= 0 || max_per_frame <= 0) return CN_ERR_SHAPE;
    if (K > 128 || (long long)T * K > CN_TILES_MAX_ROWS) return CN_ERR_SHAPE;
    if (workspace_bytes < cn_multi_pose_tiles_merge_workspace_bytes(B, T, K)) return CN_ERR_WORKSPACE;
    if (!cn_aligned16(workspace)) return CN_ERR_ALIGN;
    const int cap = pose_tiles_lds_rows(T * K);
    CN_SET_MAX_LDS_ONCE(pose_tiles_merge_kernel, pose_tiles_lds_bytes(PT_CAP));
    hipLaunchKernelGGL(pose_tiles_merge_kernel, dim3(B), dim3(PT_THREADS), pose_tiles_lds_bytes(cap),
                       (hipStream_t)stream, rows, T, K, cores_dev, (T > 1 || apply_nms) ? 1 : 0, max_per_frame,
                       min_score, cap, out_rows, out_counts, status);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
