// cn_tail.hip -- the tasks' tails of the frame pipe on the device (frame_pipe.py: DeviceTail), bit for bit what
// the host tails compute.  Per test scale a post-process kernel: ctdet_post_kernel, multi_pose_post_kernel,
// ddd_post_kernel (raw detections of the decode -> rows in source pixels; ctdet and ddd grouped by class, with
// the class bounds) and exdet_post_kernel (post_process + the positive-score filter + a stable class grouping of
// up to MG_ROWS rows).  Behind the last scale the merge kernels.
//
// class_merge_kernel<false> is the ctdet scale merge (CtdetDetector.merge_outputs, detectors/ctdet.py:54-74;
// reference ctdet.py:58-73).  Input: cn_ctdet_post_process_f32's output of every test scale, slice s of rows
// (S, B, K, 5) / bounds (S, B, nc + 1).  Output in the same format, so the host slices it as it slices a single
// scale.  class_merge_kernel<true> is the same merge behind exdet_post_kernel with the row cap checked per image;
// multi_pose_merge_kernel runs the same soft-NMS routine on 39-column rows, one segment per image.
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
//
// The tile merge of run_tiles (cn_ctdet_tiles_merge_f32; post_process.ctdet_tiles_results is its host
// restatement) is the same merge with tiles in the place of scales, for frames whose rows no longer fit one
// workgroup's LDS: three launches, the class-grouped rows of a frame in global memory between them.
//   tiles_group_kernel  one workgroup per frame: the core filter (a row survives when its centre lies in its
//                       tile's core), a class histogram per wave, the scan to the class bounds and a stable
//                       scatter -- exdet_post_kernel's counting sort with (tile, row) in the place of rows;
//   tiles_nms_kernel    one wave per (frame, class): the segment into NmsLds at o = 0, soft_nms_segment, back;
//   tiles_cut_kernel    one workgroup per frame: the max_per_frame-th largest score by cn_select.h's
//                       radix_select over distinct (score, position) keys, then the ordered compaction.
// What bounds a frame is the longest class segment (CN_MERGE_MAX_ROWS, the LDS of one soft-NMS), not its rows.
// cn_ctdet_tiles_merge_gated_f32 (a tile pyramid; post_process.ctdet_pyramid_results) is the same
// three launches with a size gate per tile next to the core in the filter; the old entry passes a null gate table.
#include "cn_select.h"

// hipcc defaults to -ffp-contract=fast-honor-pragmas: the float64 point map and the float32 chains below are
// the host's operations one by one only without FMA contraction, anywhere in this file (cn_select.h sets the
// same pragma for the files that include it; it is repeated here because this file depends on it by itself).
#pragma clang fp contract(off)

namespace {
constexpr int PP_KMAX = 128;     // rows per image of the ctdet / multi_pose / ddd post-process kernels
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

// Workgroup exclusive scan of one int per thread (MG_THREADS threads, all of them call it): the sum over the
// threads in front of this one; `total`: over all of them.
__device__ __forceinline__ int block_exclusive_scan(int n, int *red, int &total)
{
    const int lane = threadIdx.x & (CN_WAVE - 1), w = threadIdx.x / CN_WAVE;
    int incl = n;
    for (int o = 1; o < CN_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    __syncthreads();                      // red[] of an earlier use has been read
    if (lane == CN_WAVE - 1) red[w] = incl;
    __syncthreads();
    int run = incl - n;
    total = 0;
    for (int k = 0; k < MG_WAVES; ++k) {
        if (k < w) run += red[k];
        total += red[k];
    }
    return run;
}

// Output grid -> source pixels, the arithmetic of utils/image.py:63-66: float32 point -> float64
// (x * t0 + y * t1) + t2 -> ONE rounding to float32.  The map of image b, or the one map of the batch.
struct PointMap {
    double t0, t1, t2, t3, t4, t5;
    __device__ __forceinline__ PointMap(const double *to_source, int per_image, int b)
    {
        const double *t = to_source + (per_image ? (size_t)b * 6 : 0);
        t0 = t[0]; t1 = t[1]; t2 = t[2]; t3 = t[3]; t4 = t[4]; t5 = t[5];
    }
    __device__ __forceinline__ void operator()(float x, float y, float &sx, float &sy) const
    {
        sx = (float)(((double)x * t0 + (double)y * t1) + t2);
        sy = (float)(((double)x * t3 + (double)y * t4) + t5);
    }
};

// Stable grouping by class of the K <= PP_KMAX rows of one image, thread k = row k, cls_s[k] = its class
// (num_classes: no class, behind every class).  The position of row k: behind the rows of lower classes and the
// earlier rows of its own.
__device__ __forceinline__ int class_rank(const int *cls_s, int K, int cls, int k)
{
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += (cls_s[j] < cls || (cls_s[j] == cls && j < k)) ? 1 : 0;
    return rank;
}
// bounds[c] = rows of classes < c, c in [0, num_classes].  With pass_s (ddd): kept[c] = the length of class c's
// leading run of rows with pass_s set.
__device__ __forceinline__ void class_bounds(const int *cls_s, const int *pass_s, int K, int num_classes, int k,
                                             int32_t *bounds, int32_t *kept)
{
    for (int c = k; c <= num_classes; c += PP_KMAX) {
        int n = 0, lead = 0, open = 1;
        for (int j = 0; j < K; ++j) {
            n += cls_s[j] < c ? 1 : 0;
            if (pass_s && cls_s[j] == c) {
                open &= pass_s[j];
                lead += open;
            }
        }
        bounds[c] = n;
        if (pass_s && c < num_classes) kept[c] = lead;
    }
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
    int n = 0, kept;
    for (int r = r0; r < r1; ++r) n += (!cut || L.sc[r] >= thresh) ? 1 : 0;
    int run = block_exclusive_scan(n, L.red, kept);
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

// ctdet_post_process + the per-class split (utils/post_process.py:83-100, utils/image.py:19-24,63-66,
// detectors/ctdet.py:47-56), so that the host tail of a batch is one small copy and 80 slices per image: for
// every image the K raw detections [x1, y1, x2, y2, score, class] in output-grid units become rows [x1, y1, x2,
// y2, score] in source-frame pixels (PointMap, then / scale in float32), grouped by class (ascending; inside a
// class in their original, score-descending order), plus the class bounds.  The class is the float truncated
// (astype(np.int64)); rows whose class lies outside [0, num_classes) are dropped (they match no `classes == j`).
__global__ __launch_bounds__(PP_KMAX) void ctdet_post_kernel(const float *__restrict__ dets, int K, int num_classes,
                                                             const double *__restrict__ to_source, int per_image,
                                                             float scale, float *__restrict__ rows,
                                                             int32_t *__restrict__ bounds)
{
    __shared__ int cls_s[PP_KMAX];
    const int b = blockIdx.x, k = threadIdx.x;
    const PointMap to_src(to_source, per_image, b);
    float r[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int cls = num_classes;             // sorts behind every class
    if (k < K) {
        const float *d = dets + ((size_t)b * K + k) * 6;
        const int c = (int)(long long)d[5];        // astype(np.int64): truncation
        if (c >= 0 && c < num_classes) cls = c;
        to_src(d[0], d[1], r[0], r[1]);
        to_src(d[2], d[3], r[2], r[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = r[e] / scale;
        r[4] = d[4];
    }
    cls_s[k] = cls;
    __syncthreads();
    if (k < K) {
        float *o = rows + ((size_t)b * K + class_rank(cls_s, K, cls, k)) * 5;
#pragma unroll
        for (int e = 0; e < 5; ++e) o[e] = r[e];
    }
    class_bounds(cls_s, nullptr, K, num_classes, k, bounds + (size_t)b * (num_classes + 1), nullptr);
}

// multi_pose_post_process (utils/post_process.py:103-114, detectors/multi_pose.py:62-72): the K raw rows [x1,
// y1, x2, y2, score, 17 x (x, y), class] of every image in output-grid units become rows [x1, y1, x2, y2,
// score, 17 x (x, y)] in source-frame pixels / scale.  The two box corners and the 17 joints are 19 points
// under one inverse map, with the arithmetic of ctdet_post_kernel; the score is copied, the class dropped, the
// row order kept (one class: nothing to group).  One item per point or score, so the 39 columns of a row are
// written by neighbouring lanes.
constexpr int MP_IN = 40, MP_OUT = 39, MP_ITEMS = 20;   // 19 points + the score per row
__global__ __launch_bounds__(MG_THREADS) void multi_pose_post_kernel(const float *__restrict__ dets, int K,
                                                                     const double *__restrict__ to_source,
                                                                     int per_image, float scale,
                                                                     float *__restrict__ rows)
{
    const int b = blockIdx.x;
    const PointMap to_src(to_source, per_image, b);
    for (int e = threadIdx.x; e < K * MP_ITEMS; e += MG_THREADS) {
        const int k = e / MP_ITEMS, j = e - k * MP_ITEMS;
        const float *d = dets + ((size_t)b * K + k) * MP_IN;
        float *o = rows + ((size_t)b * K + k) * MP_OUT;
        if (j == MP_ITEMS - 1) {
            o[4] = d[4];
            continue;
        }
        const int c = j < 2 ? 2 * j : 2 * j + 1;     // corners in columns 0..3, joints from column 5
        float sx, sy;
        to_src(d[c], d[c + 1], sx, sy);
        o[c] = sx / scale;
        o[c + 1] = sy / scale;
    }
}

// ddd_post_process_2d + ddd_post_process_3d + DddDetector.merge_outputs (utils/post_process.py:24-79,
// utils/ddd_utils.py:68-114, detectors/ddd.py:82-88) for a batch, image b lifted with ITS matrix: the K raw
// rows [x, y, score, rot 8, depth, dim 3, w, h, class] of ddd_decode become [alpha, x1, y1, x2, y2, h, w, l,
// x, y, z, rotation_y, score], grouped by class as ctdet_post_kernel groups them, plus per class the length
// of the leading run of rows with score > peak_thresh (the rows of a class are in descending score order,
// so merge_outputs' mask is that prefix).  Types as the reference's: centre and (w, h) through the float64
// point map (translation included for both) and rounded to float32; unproject, "+ h / 2", the box and the
// angle sums in float32.  The two arctan2 are float64 atan2 rounded once to float32 (NumPy's float32
// arctan2 differs from that by at most one ulp of the angle; no device form equals it bit for bit).
// A class is taken when the float equals an integer in [0, num_classes) (`classes == j`).
constexpr int DDD_IN = 18, DDD_OUT = 13;
__global__ __launch_bounds__(PP_KMAX) void ddd_post_kernel(const float *__restrict__ dets, int K, int num_classes,
                                                           const double *__restrict__ to_source, int per_image,
                                                           const float *__restrict__ calibs, float peak_thresh,
                                                           float *__restrict__ rows, int32_t *__restrict__ bounds,
                                                           int32_t *__restrict__ kept)
{
    __shared__ int cls_s[PP_KMAX];
    __shared__ int pass_s[PP_KMAX];
    const float HALF_PI = 1.57079637f, PI = 3.14159274f, TWO_PI = 6.28318548f;   // float32(np.pi) and kin
    const int b = blockIdx.x, k = threadIdx.x;
    const PointMap to_src(to_source, per_image, b);
    const float *P = calibs + (size_t)b * 12;
    float r[DDD_OUT];
#pragma unroll
    for (int e = 0; e < DDD_OUT; ++e) r[e] = 0.f;
    int cls = num_classes;             // sorts behind every class
    if (k < K) {
        const float *d = dets + ((size_t)b * K + k) * DDD_IN;
        const float cf = d[DDD_IN - 1];
        if (cf >= 0.f && cf < (float)num_classes) {
            const int c = (int)cf;
            if ((float)c == cf) cls = c;
        }
        float cx, cy, w2, h2;          // centre, then the (w, h) pair: the same map for both
        to_src(d[0], d[1], cx, cy);
        to_src(d[15], d[16], w2, h2);
        w2 = w2 / 2.f;
        h2 = h2 / 2.f;
        // get_alpha: bin 1 (centred on -pi / 2) when its second logit is the larger one
        const bool first = d[4] > d[8];
        const float bin = (float)atan2((double)(first ? d[5] : d[9]), (double)(first ? d[6] : d[10]));
        const float alpha = bin + (first ? -HALF_PI : HALF_PI);
        const float depth = d[11], dim_h = d[12];
        // unproject_2d_to_3d, then location[1] += h / 2
        const float z = depth - P[11];
        const float lx = ((cx * depth - P[3]) - P[2] * z) / P[0];
        const float ly = ((cy * depth - P[7]) - P[6] * z) / P[5] + dim_h / 2.f;
        // alpha2rot_y
        float ry = alpha + (float)atan2((double)(cx - P[2]), (double)P[0]);
        if (ry > PI) ry = ry - TWO_PI;
        if (ry < -PI) ry = ry + TWO_PI;
        r[0] = alpha;
        r[1] = cx - w2; r[2] = cy - h2; r[3] = cx + w2; r[4] = cy + h2;
        r[5] = dim_h; r[6] = d[13]; r[7] = d[14];
        r[8] = lx; r[9] = ly; r[10] = z;
        r[11] = ry; r[12] = d[2];
    }
    cls_s[k] = cls;
    pass_s[k] = (k < K && r[12] > peak_thresh) ? 1 : 0;
    __syncthreads();
    if (k < K) {
        float *o = rows + ((size_t)b * K + class_rank(cls_s, K, cls, k)) * DDD_OUT;
#pragma unroll
        for (int e = 0; e < DDD_OUT; ++e) o[e] = r[e];
    }
    class_bounds(cls_s, pass_s, K, num_classes, k, bounds + (size_t)b * (num_classes + 1),
                 kept + (size_t)b * num_classes);
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
    __shared__ ExdetPostLds L;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    const float *in = dets + (size_t)b * R * PX_ROW;
    float *out = rows + (size_t)b * R * 5;
    const PointMap to_src(to_source, per_image, b);
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
    int total, run = block_exclusive_scan(n, L.red, total);
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
        float p[4];
        to_src(x1, y1, p[0], p[1]);
        to_src(x2, y2, p[2], p[3]);
        float *o = out + (size_t)pos * 5;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = p[e] / scale;
        o[4] = d[4];
    }
    // rows behind the last bound: zeros, so that the array is a function of the input
    for (int e = total * 5 + t; e < R * 5; e += MG_THREADS) out[e] = 0.f;
}
// ------------------------------------------------------------------------------------------------
// run_tiles: the tile merge (see the head of the file)
// ------------------------------------------------------------------------------------------------
// Row e = t * K + r of frame b (row r of tile t as cn_ctdet_post_process_f32 left it) -> its class when it is a
// row of a class (r in front of the tile's last bound) and its centre lies in the tile's core, else -1.
// cx = (x1 + x2) * 0.5f, lo <= cx < hi in float32: the host's comparison; a NaN centre fails it.
// gates (T, 2) [lo, hi) or null (cn_ctdet_tiles_merge_gated_f32; uniform over the launch): with w = x2 - x1 and
// h = y2 - y1 a NaN in either drops the row, otherwise s = max(w, h) must have lo <= s < hi as well.
__device__ __forceinline__ int tile_row_class(const float *__restrict__ rows, const int32_t *__restrict__ bounds,
                                              const float *__restrict__ cores, const float *__restrict__ gates,
                                              int b, int T, int K, int nc, int e)
{
    const int t = e / K, r = e - t * K;
    const int32_t *bd = bounds + ((size_t)b * T + t) * ((size_t)nc + 1);
    if (r >= bd[nc]) return -1;
    const float *s = rows + (((size_t)b * T + t) * K + r) * 5;
    const float cx = (s[0] + s[2]) * 0.5f, cy = (s[1] + s[3]) * 0.5f;
    const float *co = cores + (size_t)t * 4;
    if (!(cx >= co[0] && cx < co[2] && cy >= co[1] && cy < co[3])) return -1;
    if (gates) {
        const float w = s[2] - s[0], h = s[3] - s[1];
        if (w != w || h != h) return -1;
        const float sz = w > h ? w : h;      // (no NaN left: a plain maximum)
        if (!(sz >= gates[2 * t] && sz < gates[2 * t + 1])) return -1;
    }
    int lo = 0, hi = nc;                 // the last c with bd[c] <= r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bd[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// Launch 1.  grouped (B, T * K, 5): per class the survivors of all tiles in tile order, each tile's rows in
// their order (the np.concatenate of the host); segs (B, nc + 1): the class bounds in it.  Every wave owns a
// contiguous quarter of the frame's T * K rows in whole steps of 64, as in exdet_post_kernel; the class of a
// row is computed again in step 3 instead of being kept (T * K int16 would not fit next to the histograms).
// A frame with a class segment above MG_ROWS is not merged: status[b] = 1, its out_bounds zero.
struct TilesGroupLds {
    int hist[MG_WAVES][MG_CLASSES + 1];
    int red[MG_WAVES];
    int over;
};
__global__ __launch_bounds__(MG_THREADS) void tiles_group_kernel(const float *__restrict__ rows,
                                                                 const int32_t *__restrict__ bounds, int T, int K,
                                                                 int nc, const float *__restrict__ cores,
                                                                 const float *__restrict__ gates,
                                                                 float *__restrict__ grouped,
                                                                 int32_t *__restrict__ segs,
                                                                 int32_t *__restrict__ out_bounds,
                                                                 int32_t *__restrict__ status)
{
    __shared__ TilesGroupLds L;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    const int R = T * K;
    const int per = (R + MG_THREADS - 1) / MG_THREADS * CN_WAVE;
    const int w0 = min(w * per, R), w1 = min(w0 + per, R);
    for (int c = t; c < MG_WAVES * (MG_CLASSES + 1); c += MG_THREADS) (&L.hist[0][0])[c] = 0;
    if (t == 0) L.over = 0;
    __syncthreads();
    // 1. the survivors' class histograms (LDS atomics: counts only)
    for (int e = w0 + lane; e < w1; e += CN_WAVE) {
        const int c = tile_row_class(rows, bounds, cores, gates, b, T, K, nc, e);
        if (c >= 0) atomicAdd(&L.hist[w][c], 1);
    }
    __syncthreads();
    // 2. class bounds: exclusive scan of the class totals, a chunk of classes per thread; hist[w][c] becomes
    //    the position of wave w's first row of class c
    const int cper = (nc + MG_THREADS) / MG_THREADS, c0 = min(t * cper, nc), c1 = min(c0 + cper, nc);
    int n = 0;
    for (int c = c0; c < c1; ++c)
        for (int k = 0; k < MG_WAVES; ++k) n += L.hist[k][c];
    int total, run = block_exclusive_scan(n, L.red, total);
    int32_t *sg = segs + (size_t)b * (nc + 1);
    bool over = false;
    for (int c = c0; c < c1; ++c) {
        const int first = run;
        sg[c] = run;
        for (int k = 0; k < MG_WAVES; ++k) {
            const int h = L.hist[k][c];
            L.hist[k][c] = run;
            run += h;
        }
        over |= run - first > MG_ROWS;
    }
    if (t == 0) sg[nc] = total;
    if (over) L.over = 1;                // (every writer writes 1)
    __syncthreads();
    if (L.over) {                        // the same word for every thread: the whole workgroup leaves
        if (t == 0) status[b] = 1;
        for (int c = t; c <= nc; c += MG_THREADS) out_bounds[(size_t)b * (nc + 1) + c] = 0;
        return;
    }
    if (t == 0) status[b] = 0;
    // 3. positions by ballot, wave by wave in input order (hist[w][.] is wave w's alone from here on)
    int *cur = L.hist[w];
    float *out = grouped + (size_t)b * R * 5;
    for (int base = w0; base < w1; base += CN_WAVE) {
        const int e = base + lane;
        const int c = e < w1 ? tile_row_class(rows, bounds, cores, gates, b, T, K, nc, e) : -1;
        int pos = -1;
        unsigned long long todo = __ballot(c >= 0);
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
        const int tl = e / K;
        const float *s = rows + (((size_t)b * T + tl) * K + (e - tl * K)) * 5;
        float *o = out + (size_t)pos * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) o[k] = s[k];
    }
}

// Launch 2.  One wave per (frame, class): a segment of two rows or more goes through soft_nms_segment in LDS
// and back, in place.  Segments of different workgroups do not overlap.
__global__ __launch_bounds__(CN_WAVE) void tiles_nms_kernel(float *__restrict__ grouped,
                                                            const int32_t *__restrict__ segs,
                                                            const int32_t *__restrict__ status, int R, int nc)
{
    __shared__ NmsLds L;
    const int b = blockIdx.x / nc, c = blockIdx.x - b * nc, lane = threadIdx.x;
    if (status[b]) return;
    const int32_t *sg = segs + (size_t)b * (nc + 1);
    const int o = sg[c], n = sg[c + 1] - o;
    if (n <= 1 || n > MG_ROWS || o < 0 || o + n > R) return;
    float *g = grouped + ((size_t)b * R + o) * 5;
    for (int p = lane; p < n; p += CN_WAVE) {
        const float *s = g + (size_t)p * 5;
        L.box[0][p] = s[0];
        L.box[1][p] = s[1];
        L.box[2][p] = s[2];
        L.box[3][p] = s[3];
        L.sc[p] = s[4];
    }
    wave_sync();
    soft_nms_segment<false>(L, 0, n, lane, nullptr);
    wave_sync();
    for (int p = lane; p < n; p += CN_WAVE) {
        float *d = g + (size_t)p * 5;
        d[0] = L.box[0][p];
        d[1] = L.box[1][p];
        d[2] = L.box[2][p];
        d[3] = L.box[3][p];
        d[4] = L.sc[p];
    }
}

// Launch 3.  thresh = the max_per_frame-th largest score, duplicates counted: radix_select takes the
// max_per_frame largest of the DISTINCT keys (score key, ~position), and the smallest score among them is that
// score.  Then score >= thresh in array order, a contiguous chunk of rows per thread; the thread that passes a
// class bound on its way writes the bound's new value.
struct TilesCutLds {
    SelShared sel;
    int seg[MG_CLASSES + 1];
    int red[MG_WAVES];
    uint32_t low[MG_WAVES];
};
__global__ __launch_bounds__(MG_THREADS) void tiles_cut_kernel(const float *__restrict__ grouped,
                                                               const int32_t *__restrict__ segs,
                                                               const int32_t *__restrict__ status, int R, int nc,
                                                               int max_per_frame, float *__restrict__ out_rows,
                                                               int32_t *__restrict__ out_bounds)
{
    __shared__ TilesCutLds L;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (CN_WAVE - 1), w = t / CN_WAVE;
    if (status[b]) return;
    for (int c = t; c <= nc; c += MG_THREADS) L.seg[c] = segs[(size_t)b * (nc + 1) + c];
    __syncthreads();
    const int total = min(max(L.seg[nc], 0), R);
    const float *g = grouped + (size_t)b * R * 5;
    const bool cut = total > max_per_frame;
    float thresh = 0.f;
    if (cut) {                           // (the same for every thread)
        auto for_each = [&](auto &&f) {
            for (int r = t; r < total; r += MG_THREADS) {
                const uint32_t k = f2key(g[(size_t)r * 5 + 4]);
                f(((u64)k << 32) | (uint32_t)~(uint32_t)r, k == KEY_ZERO);
            }
        };
        u64 prefix, mask;
        radix_select<MG_THREADS>(for_each, (uint32_t)max_per_frame, L.sel, prefix, mask);
        uint32_t low = 0xffffffffu;
        for_each([&](u64 k, bool) {
            if ((k & mask) >= prefix) low = min(low, (uint32_t)(k >> 32));
        });
        for (int o = CN_WAVE / 2; o > 0; o >>= 1) low = min(low, (uint32_t)__shfl_xor((int)low, o));
        if (lane == 0) L.low[w] = low;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MG_WAVES; ++k) low = min(low, L.low[k]);
        thresh = key2f(low);
    }
    const int per = (total + MG_THREADS - 1) / MG_THREADS, r0 = min(t * per, total), r1 = min(r0 + per, total);
    int n = 0, kept;
    for (int r = r0; r < r1; ++r) n += (!cut || g[(size_t)r * 5 + 4] >= thresh) ? 1 : 0;
    int run = block_exclusive_scan(n, L.red, kept);
    int cnext = 0;                       // the first class bound at or behind r0
    {
        int lo = -1, hi = nc + 1;        // seg[] ascends: the first c with seg[c] >= r0
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (L.seg[mid] >= r0) hi = mid; else lo = mid;
        }
        cnext = hi;
    }
    float *ob = out_rows + (size_t)b * R * 5;
    int32_t *obd = out_bounds + (size_t)b * (nc + 1);
    for (int r = r0; r < r1; ++r) {
        while (cnext <= nc && L.seg[cnext] == r) obd[cnext++] = run;
        const float *s = g + (size_t)r * 5;
        if (!cut || s[4] >= thresh) {
            float *d = ob + (size_t)run * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) d[k] = s[k];
            ++run;
        }
    }
    for (int c = t; c <= nc; c += MG_THREADS)
        if (L.seg[c] >= total) obd[c] = kept;
}
}  // namespace

extern "C" int cn_ctdet_post_process_f32(const float *dets, int B, int K, int num_classes,
                                         const double *to_source_2x3, int per_image, float scale,
                                         float *rows, int32_t *bounds, void *stream)
{
    if (!dets || !to_source_2x3 || !rows || !bounds) return CN_ERR_NULL;
    if (B <= 0 || K <= 0 || num_classes <= 0 || !(scale > 0.f)) return CN_ERR_SHAPE;
    if (K > PP_KMAX) return CN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ctdet_post_kernel, dim3(B), dim3(PP_KMAX), 0, (hipStream_t)stream, dets, K, num_classes,
                       to_source_2x3, per_image ? 1 : 0, scale, rows, bounds);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_multi_pose_post_process_f32(const float *dets, int B, int K, const double *to_source_2x3,
                                              int per_image, float scale, float *rows, void *stream)
{
    if (!dets || !to_source_2x3 || !rows) return CN_ERR_NULL;
    if (B <= 0 || K <= 0 || !(scale > 0.f)) return CN_ERR_SHAPE;
    if (K > PP_KMAX) return CN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(multi_pose_post_kernel, dim3(B), dim3(MG_THREADS), 0, (hipStream_t)stream, dets, K,
                       to_source_2x3, per_image ? 1 : 0, scale, rows);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_ddd_post_process_f32(const float *dets, int B, int K, int row_floats, int num_classes,
                                       const double *to_source_2x3, int per_image, const float *calibs,
                                       float peak_thresh, float *rows, int32_t *bounds, int32_t *kept, void *stream)
{
    if (!dets || !to_source_2x3 || !calibs || !rows || !bounds || !kept) return CN_ERR_NULL;
    if (B <= 0 || K <= 0 || num_classes <= 0 || (row_floats != 16 && row_floats != DDD_IN)) return CN_ERR_SHAPE;
    if (row_floats != DDD_IN) return CN_ERR_UNSUPPORTED;    // no (w, h): the reference's 3-D stage has no box either
    if (K > PP_KMAX) return CN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ddd_post_kernel, dim3(B), dim3(PP_KMAX), 0, (hipStream_t)stream, dets, K, num_classes,
                       to_source_2x3, per_image ? 1 : 0, calibs, peak_thresh, rows, bounds, kept);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

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

static size_t tiles_grouped_bytes(int B, int T, int K) { return cn_align_up((size_t)B * T * K * 5 * sizeof(float), 16); }

extern "C" size_t cn_ctdet_tiles_merge_workspace_bytes(int B, int T, int K, int num_classes)
{
    if (B <= 0 || T <= 0 || K <= 0 || num_classes <= 0) return 0;
    return tiles_grouped_bytes(B, T, K) + cn_align_up((size_t)B * (num_classes + 1) * sizeof(int32_t), 16);
}

// the old entry (gates_dev null) and the gated one: the same three launches
static int tiles_merge(const float *rows, const int32_t *bounds, int B, int T, int K, int num_classes,
                       const float *cores_dev, const float *gates_dev, int apply_nms, int max_per_frame,
                       float *out_rows, int32_t *out_bounds, int32_t *status, void *workspace,
                       size_t workspace_bytes, void *stream)
{
    if (B <= 0 || T <= 0 || K <= 0 || num_classes <= 0 || max_per_frame <= 0) return CN_ERR_SHAPE;
    if (K > PP_KMAX || (long long)T * K > CN_TILES_MAX_ROWS || num_classes > CN_MERGE_MAX_CLASSES) return CN_ERR_SHAPE;
    if ((long long)B * num_classes > 0x7fffffffLL) return CN_ERR_SHAPE;      // (the grid of the soft-NMS launch)
    if (workspace_bytes < cn_ctdet_tiles_merge_workspace_bytes(B, T, K, num_classes)) return CN_ERR_WORKSPACE;
    if (!cn_aligned16(workspace)) return CN_ERR_ALIGN;
    float *grouped = reinterpret_cast<float *>(workspace);
    int32_t *segs = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(workspace) + tiles_grouped_bytes(B, T, K));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tiles_group_kernel, dim3(B), dim3(MG_THREADS), 0, st, rows, bounds, T, K, num_classes,
                       cores_dev, gates_dev, grouped, segs, out_bounds, status);
    CN_CHECK_LAUNCH();
    if (T > 1 || apply_nms) {
        hipLaunchKernelGGL(tiles_nms_kernel, dim3((unsigned)B * num_classes), dim3(CN_WAVE), 0, st, grouped, segs,
                           status, T * K, num_classes);
        CN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tiles_cut_kernel, dim3(B), dim3(MG_THREADS), 0, st, grouped, segs, status, T * K,
                       num_classes, max_per_frame, out_rows, out_bounds);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_ctdet_tiles_merge_f32(const float *rows, const int32_t *bounds, int B, int T, int K,
                                        int num_classes, const float *cores_dev, int apply_nms, int max_per_frame,
                                        float *out_rows, int32_t *out_bounds, int32_t *status, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    if (!rows || !bounds || !cores_dev || !out_rows || !out_bounds || !status || !workspace) return CN_ERR_NULL;
    return tiles_merge(rows, bounds, B, T, K, num_classes, cores_dev, nullptr, apply_nms, max_per_frame, out_rows,
                       out_bounds, status, workspace, workspace_bytes, stream);
}

extern "C" size_t cn_ctdet_tiles_merge_gated_workspace_bytes(int B, int T, int K, int num_classes)
{
    return cn_ctdet_tiles_merge_workspace_bytes(B, T, K, num_classes);
}

extern "C" int cn_ctdet_tiles_merge_gated_f32(const float *rows, const int32_t *bounds, int B, int T, int K,
                                              int num_classes, const float *cores_dev, const float *gates_dev,
                                              int apply_nms, int max_per_frame, float *out_rows, int32_t *out_bounds,
                                              int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rows || !bounds || !cores_dev || !gates_dev || !out_rows || !out_bounds || !status || !workspace)
        return CN_ERR_NULL;
    return tiles_merge(rows, bounds, B, T, K, num_classes, cores_dev, gates_dev, apply_nms, max_per_frame, out_rows,
                       out_bounds, status, workspace, workspace_bytes, stream);
}
