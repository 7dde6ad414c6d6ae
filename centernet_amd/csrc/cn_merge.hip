// cn_merge.hip -- the ctdet scale merge on the device (CtdetDetector.merge_outputs, detectors/ctdet.py:54-74;
// reference ctdet.py:58-73), bit for bit.  Input: the device tail's output of every test scale
// (cn_ctdet_post_process_f32 into slice s of rows (S, B, K, 5) / bounds (S, B, nc + 1)).  Output in the
// tail's own format, so the host slices it as it slices a single scale.  Behind it the multi_pose scale
// merge (multi_pose_merge_kernel): the same soft-NMS routine on 39-column rows, one segment per image.  And the
// exdet tail: exdet_post_kernel (post_process + the positive-score filter + a stable class grouping of up to
// MG_ROWS rows) in front of the same merge kernel with the row cap checked per image (class_merge_kernel<true>).
//
// One workgroup of four waves per image; the image's rows (<= CN_MERGE_MAX_ROWS) live in LDS.
//   1. per class, the rows of all scales in scale order (the np.concatenate of merge_outputs);
//   2. when S > 1 or apply_nms: Gaussian soft-NMS (sigma 0.5, threshold 0.001) of every class segment,
//      one wave per segment, with the arithmetic of cn_soft_nms_f32 (cn_misc.hip) term by term.  The whole
//      in-place array is kept: the reference ignores the kept count, rows past N stay with stale scores;
//   3. when the image has more rows than max_per_image: thresh = the max_per_image-th largest score
//      (duplicates counted: np.partition(scores, len - max_per_image)), keep score >= thresh in array order.
//
// The greedy step of soft-NMS, for one segment and step i (rows [i, N) still live):
//   argmax  -- a wave reduction; equal scores go to the lowest position (the reference's strict `<`);
//   decay   -- every live row p > i is examined exactly once per step, at its own position or, after a
//              discard moved it there, at the discarded row's position; its box does not change on the
//              way, so its new score ns[p] = weight(p) * score(p) and whether it is discarded are computed
//              for all rows at once, lane-parallel;
//   walk    -- what stays order dependent is WHERE rows end up: a discarded row takes columns 0..4 of row
//              N - 1 (which has not been examined yet and so still holds its old score), N shrinks and the
//              moved row is examined at the same position next.  The wave jumps from discard to discard
//              with ballots; orig[] records which row now sits where, and the decayed scores are written
//              afterwards, at the positions their rows occupy.  tests/test_tta_host.py holds this form
//              equal to cn_soft_nms_f32 on seeded arrays before any GPU run.
#include "cn_common.h"

namespace {
constexpr int MG_THREADS = 256;
constexpr int MG_WAVES = MG_THREADS / CN_WAVE;
constexpr int MG_ROWS = CN_MERGE_MAX_ROWS;
constexpr int MG_CLASSES = CN_MERGE_MAX_CLASSES;
constexpr float MG_SIGMA = 0.5f, MG_THRESHOLD = 0.001f;

struct NmsLds {
    float box[4][MG_ROWS];   // x1, y1, x2, y2 of the merged rows (class segments back to back)
    float sc[MG_ROWS];       // score
    float ns[MG_ROWS];       // soft-NMS: decayed score of the row that started the step at p; select: prefix
    int16_t orig[MG_ROWS];   // soft-NMS: start-of-step position of the row now at p
    uint8_t disc[MG_ROWS];   // soft-NMS: the row that started the step at p is discarded
};
struct MergeLds : NmsLds {
    int seg[MG_CLASSES + 1]; // class c = [seg[c], seg[c + 1])
    int red[MG_WAVES];
};
// multi_pose rows carry 34 joint columns behind the score.  They never enter LDS (2048 x 34 floats would
// not fit): jsrc[p] names the input row whose joints sit at position p, and the joints are gathered from
// the global input once, at the end.
struct PoseLds : NmsLds {
    int16_t jsrc[MG_ROWS];
};

// LDS written by one lane is read by the others of the same wave next: order the wave's own accesses
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int block_sum(int v, int *red)
{
    for (int o = CN_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x / CN_WAVE;
    __syncthreads();                      // red[] of the previous call has been read
    if ((threadIdx.x & (CN_WAVE - 1)) == 0) red[w] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int k = 0; k < MG_WAVES; ++k) s += red[k];
    return s;
}

// float -> unsigned key of the same order
__device__ __forceinline__ uint32_t order_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// float division through double: a / b for float a, b rounds to the same float either way (53 >= 2 * 24 + 2
// bits), so the result is the IEEE quotient the host computes whatever the device division flags are
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// Soft-NMS of one class segment [o, o + n) by one wave (see the head of the file).  JOINTS: the rows have
// columns behind the score (nms.pyx:260-268, cn_soft_nms_f32): the argmax swap exchanges whole rows, a
// discarded row takes columns 0..4 of row N - 1 and EXCHANGES columns 5.. with it -- both are exchanges of
// jsrc[], `jsrc` being the segment's slice of PoseLds::jsrc (unused without JOINTS).
template <bool JOINTS>
__device__ void soft_nms_segment(NmsLds &L, int o, int n, int lane, int16_t *jsrc)
{
#pragma clang fp contract(off)
    float *x1 = L.box[0] + o, *y1 = L.box[1] + o, *x2 = L.box[2] + o, *y2 = L.box[3] + o;
    float *sc = L.sc + o, *ns = L.ns + o;
    int16_t *orig = L.orig + o;
    uint8_t *disc = L.disc + o;
    int N = n;
    for (int i = 0; i < n && i < N; ++i) {
        // argmax over [i, N): the first maximum wins
        float best = 0.f;
        int bpos = 0x7fffffff;
        for (int p = i + lane; p < N; p += CN_WAVE) {
            const float s = sc[p];
            if (bpos == 0x7fffffff || s > best) { best = s; bpos = p; }
        }
        for (int off = CN_WAVE / 2; off > 0; off >>= 1) {
            const float s2 = __shfl_xor(best, off);
            const int p2 = __shfl_xor(bpos, off);
            if (p2 != 0x7fffffff && (bpos == 0x7fffffff || s2 > best || (s2 == best && p2 < bpos))) {
                best = s2;
                bpos = p2;
            }
        }
        if (lane == 0 && bpos != i) {
            float t;
            t = x1[i]; x1[i] = x1[bpos]; x1[bpos] = t;
            t = y1[i]; y1[i] = y1[bpos]; y1[bpos] = t;
            t = x2[i]; x2[i] = x2[bpos]; x2[bpos] = t;
            t = y2[i]; y2[i] = y2[bpos]; y2[bpos] = t;
            t = sc[i]; sc[i] = sc[bpos]; sc[bpos] = t;
            if (JOINTS) {
                const int16_t j = jsrc[i]; jsrc[i] = jsrc[bpos]; jsrc[bpos] = j;
            }
        }
        wave_sync();
        const float tx1 = x1[i], ty1 = y1[i], tx2 = x2[i], ty2 = y2[i];
        // decay: every live row, as cn_soft_nms_f32 computes it
        for (int p = i + 1 + lane; p < N; p += CN_WAVE) {
            const float bx1 = x1[p], by1 = y1[p], bx2 = x2[p], by2 = y2[p];
            float s = sc[p];
            bool d = false;
            const float area = (float)(((double)(bx2 - bx1) + 1.0) * ((double)(by2 - by1) + 1.0));
            const float iw = (float)((double)(fminf(tx2, bx2) - fmaxf(tx1, bx1)) + 1.0);
            if (iw > 0) {
                const float ih = (float)((double)(fminf(ty2, by2) - fmaxf(ty1, by1)) + 1.0);
                if (ih > 0) {
                    const float ua = (float)((((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0) +
                                              (double)area) - (double)(iw * ih));
                    const float ov = div_rn(iw * ih, ua);
                    const float weight = (float)exp((double)div_rn(-(ov * ov), MG_SIGMA));
                    s = weight * s;
                    d = s < MG_THRESHOLD;
                }
            }
            ns[p] = s;
            disc[p] = d ? 1 : 0;
            orig[p] = (int16_t)p;
        }
        wave_sync();
        // walk: from discard to discard
        int pos = i + 1;
        while (pos < N) {
            int p = -1;
            for (int base = pos; base < N; base += CN_WAVE) {
                const int q = base + lane;
                const unsigned long long m = __ballot(q < N && disc[q]);
                if (m) {
                    p = base + __builtin_ctzll(m);
                    break;
                }
            }
            if (p < 0) break;
            // the row at p (a row that has not moved) is discarded; so is every row moved onto p after it
            // that is itself discarded
            for (;;) {
                if (p == N - 1) {        // the last live row: it takes its own columns, N shrinks past it
                    if (lane == 0) sc[p] = ns[orig[p]];
                    N = p;
                    break;
                }
                const int last = N - 1;  // has not moved: orig[last] == last, old score
                if (lane == 0) {
                    x1[p] = x1[last]; y1[p] = y1[last]; x2[p] = x2[last]; y2[p] = y2[last]; sc[p] = sc[last];
                    orig[p] = (int16_t)last;
                    if (JOINTS) {
                        const int16_t j = jsrc[p]; jsrc[p] = jsrc[last]; jsrc[last] = j;
                    }
                }
                N = last;
                if (!disc[last]) break;
            }
            wave_sync();
            pos = p + 1;
        }
        // the decayed scores, where their rows now are
        for (int q = i + 1 + lane; q < N; q += CN_WAVE) sc[q] = ns[orig[q]];
        wave_sync();
    }
}

// CHECKED (exdet): the row cap holds for the rows that are present, not for S * K -- an image with more than
// MG_ROWS rows over all scales is not merged, status[b] says so and its bounds are zero (status is unused
// without CHECKED: the ctdet entry refuses S * K > MG_ROWS before the launch).
template <bool CHECKED>
__global__ __launch_bounds__(MG_THREADS) void class_merge_kernel(const float *__restrict__ rows,
                                                                 const int32_t *__restrict__ bounds, int S, int B,
                                                                 int K, int nc, int do_nms, int max_per_image,
                                                                 float *__restrict__ out_rows,
                                                                 int32_t *__restrict__ out_bounds,
                                                                 int32_t *__restrict__ status)
{
    __shared__ MergeLds L;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    const size_t bstride = (size_t)nc + 1;
    const int cap = min(S * K, MG_ROWS);          // rows of one image in out_rows
    // 1. merged class segments: class c starts behind every row of classes < c of every scale
    for (int c = t; c <= nc; c += MG_THREADS) {
        int n = 0;
        for (int s = 0; s < S; ++s) n += bounds[((size_t)s * B + b) * bstride + c];
        L.seg[c] = n;
    }
    __syncthreads();
    if (CHECKED) {
        const bool over = L.seg[nc] > cap;        // the same word for every thread: the whole workgroup leaves
        if (t == 0) status[b] = over ? 1 : 0;
        if (over) {
            for (int c = t; c <= nc; c += MG_THREADS) out_bounds[(size_t)b * bstride + c] = 0;
            return;
        }
    }
    const int total = min(L.seg[nc], cap);
    for (int e = t; e < S * K; e += MG_THREADS) {
        const int s = e / K, r = e - s * K;
        const int32_t *bd = bounds + ((size_t)s * B + b) * bstride;
        if (r >= bd[nc]) continue;
        int lo = 0, hi = nc;             // class of row r: the last c with bd[c] <= r
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (bd[mid] <= r) lo = mid; else hi = mid;
        }
        int dst = L.seg[lo] + (r - bd[lo]);
        for (int s2 = 0; s2 < s; ++s2) {
            const int32_t *b2 = bounds + ((size_t)s2 * B + b) * bstride;
            dst += b2[lo + 1] - b2[lo];
        }
        if (dst < 0 || dst >= total) continue;
        const float *src = rows + (((size_t)s * B + b) * K + r) * 5;
        L.box[0][dst] = src[0];
        L.box[1][dst] = src[1];
        L.box[2][dst] = src[2];
        L.box[3][dst] = src[3];
        L.sc[dst] = src[4];
    }
    __syncthreads();
    // 2. soft-NMS, one class segment per wave at a time
    if (do_nms) {
        for (int c = w; c < nc; c += MG_WAVES) {
            const int o = L.seg[c], e = min(L.seg[c + 1], total);
            if (e - o > 1) soft_nms_segment<false>(L, o, e - o, lane, nullptr);
        }
        __syncthreads();
    }
    // 3. top max_per_image by threshold: the largest key T with #{key >= T} >= max_per_image, bit by bit
    const int per = (total + MG_THREADS - 1) / MG_THREADS, r0 = min(t * per, total), r1 = min(r0 + per, total);
    bool cut = total > max_per_image;
    float thresh = 0.f;
    if (cut) {
        uint32_t T = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            int n = 0;
            for (int r = r0; r < r1; ++r) n += order_key(L.sc[r]) >= cand ? 1 : 0;
            if (block_sum(n, L.red) >= max_per_image) T = cand;
        }
        thresh = key_value(T);
    }
    // order-preserving compaction: exclusive prefix of the kept flags (chunk per thread, then a scan)
    int n = 0;
    for (int r = r0; r < r1; ++r) n += (!cut || L.sc[r] >= thresh) ? 1 : 0;
    int incl = n;
    for (int o = 1; o < CN_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    __syncthreads();
    if (lane == CN_WAVE - 1) L.red[w] = incl;
    __syncthreads();
    int run = incl - n;
    for (int k = 0; k < w; ++k) run += L.red[k];
    int kept = 0;
    for (int k = 0; k < MG_WAVES; ++k) kept += L.red[k];
    int *prefix = reinterpret_cast<int *>(L.ns);
    float *ob = out_rows + (size_t)b * cap * 5;
    for (int r = r0; r < r1; ++r) {
        prefix[r] = run;
        if (!cut || L.sc[r] >= thresh) {
            float *d = ob + (size_t)run * 5;
            d[0] = L.box[0][r];
            d[1] = L.box[1][r];
            d[2] = L.box[2][r];
            d[3] = L.box[3][r];
            d[4] = L.sc[r];
            ++run;
        }
    }
    __syncthreads();
    for (int c = t; c <= nc; c += MG_THREADS) {
        const int sg = min(L.seg[c], total);
        out_bounds[(size_t)b * bstride + c] = sg < total ? prefix[sg] : kept;
    }
}

// MultiPoseDetector.merge_outputs (detectors/multi_pose.py:135-142; reference multi_pose.py:74-81) on the
// device: one workgroup per image, the image's S * K rows in scale order (row s * K + k: the np.concatenate),
// one segment (the person class is the only one), soft-NMS by the first wave, no cut.  The whole in-place
// array is written: rows past the kept count hold the box and score they last held and the joints that the
// exchanges left there.
constexpr int MG_POSE_ROW = 39;
__global__ __launch_bounds__(MG_THREADS) void multi_pose_merge_kernel(const float *__restrict__ rows, int S, int B,
                                                                      int K, int do_nms,
                                                                      float *__restrict__ out_rows)
{
    __shared__ PoseLds L;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    const int total = S * K;
    for (int e = t; e < total; e += MG_THREADS) {
        const int s = e / K, r = e - s * K;
        const float *src = rows + (((size_t)s * B + b) * K + r) * MG_POSE_ROW;
        L.box[0][e] = src[0];
        L.box[1][e] = src[1];
        L.box[2][e] = src[2];
        L.box[3][e] = src[3];
        L.sc[e] = src[4];
        L.jsrc[e] = (int16_t)e;
    }
    __syncthreads();
    if (do_nms && w == 0 && total > 1) soft_nms_segment<true>(L, 0, total, lane, L.jsrc);
    __syncthreads();
    float *ob = out_rows + (size_t)b * total * MG_POSE_ROW;
    for (int e = t; e < total * MG_POSE_ROW; e += MG_THREADS) {
        const int r = e / MG_POSE_ROW, c = e - r * MG_POSE_ROW;
        float v;
        if (c < 4) {
            v = L.box[c][r];
        } else if (c == 4) {
            v = L.sc[r];
        } else {
            const int j = L.jsrc[r], s = j / K;
            v = rows[(((size_t)s * B + b) * K + (j - s * K)) * MG_POSE_ROW + c];
        }
        ob[e] = v;
    }
}

// ExdetDetector.post_process + the `score > 0` filter and the per-class selection of merge_outputs
// (detectors/exdet.py:51-74; reference exdet.py:86-110) for one test scale: one workgroup per frame, the
// frame's R <= MG_ROWS raw rows [x1, y1, x2, y2, score, 8 extreme-point coordinates, class] -> rows
// [x1, y1, x2, y2, score] in source pixels / scale, grouped by class and inside a class in input order.
// The grouping is a stable counting sort.  Every wave owns a contiguous quarter of the rows:
//   1. class of every row (PX_NONE: not kept), a class histogram per wave (LDS atomics: counts only);
//   2. exclusive scan of the class totals = the bounds; hist[w][c] becomes the position of wave w's first
//      row of class c, i.e. bounds[c] + the counts of the waves in front of it;
//   3. every wave walks its rows 64 at a time in input order; the rows of a step that share a class are
//      found by ballot, take positions hist[w][c] + (rank among them by lane) and move hist[w][c] on.
//      hist[w][.] is touched by wave w alone from here on: wave_sync() orders it, no workgroup barrier.
constexpr int PX_ROW = 14;
constexpr int16_t PX_NONE = -1;
struct ExdetPostLds {
    int hist[MG_WAVES][MG_CLASSES + 1];
    int16_t cls[MG_ROWS];
    int red[MG_WAVES];
};
__global__ __launch_bounds__(MG_THREADS) void exdet_post_kernel(const float *__restrict__ dets, int R, int nc,
                                                                float out_w, const double *__restrict__ to_source,
                                                                int per_image, float scale,
                                                                float *__restrict__ rows,
                                                                int32_t *__restrict__ bounds)
{
#pragma clang fp contract(off)
    __shared__ ExdetPostLds L;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    const float *in = dets + (size_t)b * R * PX_ROW;
    float *out = rows + (size_t)b * R * 5;
    const double *tr = to_source + (per_image ? (size_t)b * 6 : 0);
    const double t0 = tr[0], t1 = tr[1], t2 = tr[2], t3 = tr[3], t4 = tr[4], t5 = tr[5];
    // rows of wave w: [w0, w1), whole steps of 64
    const int per = (R + MG_THREADS - 1) / MG_THREADS * CN_WAVE;
    const int w0 = min(w * per, R), w1 = min(w0 + per, R);
    for (int c = t; c < MG_WAVES * (MG_CLASSES + 1); c += MG_THREADS) (&L.hist[0][0])[c] = 0;
    __syncthreads();
    // 1. classes and the histograms
    for (int r = w0 + lane; r < w1; r += CN_WAVE) {
        const float score = in[(size_t)r * PX_ROW + 4], cf = in[(size_t)r * PX_ROW + 13];
        int16_t c = PX_NONE;
        if (score > 0.f && cf >= 0.f && cf < (float)nc) {      // (a NaN fails every comparison)
            const int ci = (int)cf;
            if ((float)ci == cf) c = (int16_t)ci;              // `classes == j`: an integer value only
        }
        L.cls[r] = c;
        if (c != PX_NONE) atomicAdd(&L.hist[w][c], 1);
    }
    __syncthreads();
    // 2. bounds: exclusive scan of the class totals, a chunk of classes per thread
    const int cper = (nc + MG_THREADS) / MG_THREADS, c0 = min(t * cper, nc), c1 = min(c0 + cper, nc);
    int n = 0;
    for (int c = c0; c < c1; ++c)
        for (int k = 0; k < MG_WAVES; ++k) n += L.hist[k][c];
    int incl = n;
    for (int o = 1; o < CN_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == CN_WAVE - 1) L.red[w] = incl;
    __syncthreads();
    int run = incl - n, total = 0;
    for (int k = 0; k < MG_WAVES; ++k) {
        if (k < w) run += L.red[k];
        total += L.red[k];
    }
    for (int c = c0; c < c1; ++c) {
        bounds[(size_t)b * (nc + 1) + c] = run;
        for (int k = 0; k < MG_WAVES; ++k) {
            const int h = L.hist[k][c];
            L.hist[k][c] = run;
            run += h;
        }
    }
    if (t == 0) bounds[(size_t)b * (nc + 1) + nc] = total;
    __syncthreads();
    // 3. positions, the arithmetic of post_process, the rows
    int *cur = L.hist[w];
    for (int base = w0; base < w1; base += CN_WAVE) {
        const int r = base + lane;
        const int c = r < w1 ? (int)L.cls[r] : (int)PX_NONE;
        int pos = -1;
        unsigned long long todo = __ballot(c != PX_NONE);
        while (todo) {                                          // wave-uniform: one class of the step per turn
            const int leader = __builtin_ctzll(todo);
            const int cl = __shfl(c, leader);
            const unsigned long long m = __ballot(c == cl);
            if (c == cl) pos = cur[cl] + __popcll(m & ((1ull << lane) - 1ull));
            wave_sync();
            if (lane == leader) cur[cl] += __popcll(m);
            wave_sync();
            todo &= ~m;
        }
        if (pos < 0 || pos >= R) continue;
        const float *d = in + (size_t)r * PX_ROW;
        float x1 = d[0], x2 = d[2];
        const float y1 = d[1], y2 = d[3];
        if (r >= R / 2) {                                       // the mirror image's half (exdet.py:87-91)
            const float l = x1;
            x1 = out_w - x2;
            x2 = out_w - l;
        }
        float *o = out + (size_t)pos * 5;
        o[0] = (float)(((double)x1 * t0 + (double)y1 * t1) + t2) / scale;
        o[1] = (float)(((double)x1 * t3 + (double)y1 * t4) + t5) / scale;
        o[2] = (float)(((double)x2 * t0 + (double)y2 * t1) + t2) / scale;
        o[3] = (float)(((double)x2 * t3 + (double)y2 * t4) + t5) / scale;
        o[4] = d[4];
    }
    // rows behind the last bound: zeros, so that the array is a function of the input
    for (int e = total * 5 + t; e < R * 5; e += MG_THREADS) out[e] = 0.f;
}
}  // namespace

extern "C" int cn_multi_pose_merge_f32(const float *rows, int S, int B, int K, int apply_nms, float *out_rows,
                                       void *stream)
{
    if (!rows || !out_rows) return CN_ERR_NULL;
    if (S <= 0 || B <= 0 || K <= 0) return CN_ERR_SHAPE;
    if ((long long)S * K > CN_MERGE_MAX_ROWS) return CN_ERR_SHAPE;
    hipLaunchKernelGGL(multi_pose_merge_kernel, dim3(B), dim3(MG_THREADS), 0, (hipStream_t)stream, rows, S, B, K,
                       (S > 1 || apply_nms) ? 1 : 0, out_rows);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_ctdet_merge_f32(const float *rows, const int32_t *bounds, int S, int B, int K, int num_classes,
                                  int apply_nms, int max_per_image, float *out_rows, int32_t *out_bounds,
                                  void *stream)
{
    if (!rows || !bounds || !out_rows || !out_bounds) return CN_ERR_NULL;
    if (S <= 0 || B <= 0 || K <= 0 || num_classes <= 0 || max_per_image <= 0) return CN_ERR_SHAPE;
    if ((long long)S * K > CN_MERGE_MAX_ROWS || num_classes > CN_MERGE_MAX_CLASSES) return CN_ERR_SHAPE;
    hipLaunchKernelGGL(class_merge_kernel<false>, dim3(B), dim3(MG_THREADS), 0, (hipStream_t)stream, rows, bounds,
                       S, B, K, num_classes, (S > 1 || apply_nms) ? 1 : 0, max_per_image, out_rows, out_bounds,
                       (int32_t *)nullptr);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_exdet_post_process_f32(const float *dets, int B, int R, int num_classes, int out_width,
                                         const double *to_source_2x3, int per_image, float scale, float *rows,
                                         int32_t *bounds, void *stream)
{
    if (!dets || !to_source_2x3 || !rows || !bounds) return CN_ERR_NULL;
    if (B <= 0 || R <= 0 || (R & 1) || num_classes <= 0 || out_width <= 0 || !(scale > 0.f)) return CN_ERR_SHAPE;
    if (R > CN_MERGE_MAX_ROWS || num_classes > CN_MERGE_MAX_CLASSES) return CN_ERR_SHAPE;
    hipLaunchKernelGGL(exdet_post_kernel, dim3(B), dim3(MG_THREADS), 0, (hipStream_t)stream, dets, R, num_classes,
                       (float)out_width, to_source_2x3, per_image ? 1 : 0, scale, rows, bounds);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_exdet_merge_f32(const float *rows, const int32_t *bounds, int S, int B, int R, int num_classes,
                                  int max_per_image, float *out_rows, int32_t *out_bounds, int32_t *status,
                                  void *stream)
{
    if (!rows || !bounds || !out_rows || !out_bounds || !status) return CN_ERR_NULL;
    if (S <= 0 || B <= 0 || R <= 0 || (R & 1) || num_classes <= 0 || max_per_image <= 0) return CN_ERR_SHAPE;
    if (R > CN_MERGE_MAX_ROWS || num_classes > CN_MERGE_MAX_CLASSES) return CN_ERR_SHAPE;
    if ((long long)S * R > (1 << 24)) return CN_ERR_SHAPE;        // (S * R is an int inside the kernel)
    hipLaunchKernelGGL(class_merge_kernel<true>, dim3(B), dim3(MG_THREADS), 0, (hipStream_t)stream, rows, bounds, S,
                       B, R, num_classes, 1, max_per_image, out_rows, out_bounds, status);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
