// cn_heads_at.hip -- the gather-only heads evaluated at the K decoded centres: wh, reg of ctdet
// (cn_ctdet_heads_at_cells_f32), wh, hps, reg of multi_pose (cn_multi_pose_heads_at_cells_f32) and dep, rot,
// dim, wh, reg of ddd (cn_ddd_heads_at_cells_f32).
//
// ctdet_decode (decode.py:472-486) reads `wh` and `reg` at the K winning cells of every image and
// nowhere else, so a detector that does not need the dense maps runs the fused heads launch for `hm`
// alone, the image-level top-K on it (cn_topk_f32), and then this kernel: for each of the B x K cells
// and each deferred head
//     hidden = ReLU(conv3x3(feature, w1) + b1)   at that one cell (padding = 1: taps outside read 0)
//     out    = w2 . hidden + b2                  (two outputs per head)
// followed by the box arithmetic of emit_rows (cn_decode.hip), written the same way.
//
// multi_pose_decode (decode.py:506-519) gathers `hps`, `reg` and `wh` at the K centres in the same way; the
// pose entry runs the same kernel body with the heads (wh, hps[, reg]) -- 2 + 2J [+ 2] outputs per cell --
// and the row writer of emit_rows<MODE_POSE> (stage A of cn_multi_pose_decode_f32).  Staging and weight
// stream are shared; the task only selects the row writer (template parameter TASK).
//
// Arithmetic: plain fp32 FMA on the decoded feature values ((hi + lo) * 2^e is exact in fp32) and the
// original, unsplit fp32 weights: no range words, nothing can clamp.
//
// Shape of the launch: one workgroup of 256 threads per (image, 16 consecutive cells).  The 3x3 x 64
// channel patches of its cells sit in LDS (16 x 576 floats per 64-channel chunk of Cin); a thread owns
// one to three hidden channels of the concatenated heads and CT of the 16 cells, streams its weights as
// float4 (four consecutive k of one channel: cn_pack_cell_heads_w1 order) with the next group of loads
// in flight, and reads the patch values as LDS broadcasts (all lanes of a wave share the cell).  The
// hidden values then replace the patches in LDS, four lanes share one 1x1 output (a loop over the
// 16 x outputs-per-cell values, 64 per pass), and the rows are assembled from them.  Weight traffic:
// the whole first-layer weight once per workgroup from L2 (295 KB for two 64-wide heads, 1.77 MB for
// three 256-wide ones; B * ceil(K / 16) workgroups).
//
// ddd_decode (decode.py:426-462) gathers `dep`, `rot`, `dim`, `wh` and `reg` at the K centres.  Five 256-wide
// heads are 1280 hidden channels, more than one workgroup holds, and every column of a ddd row depends on one
// head only: the ddd task walks *head groups* in a third grid dimension.  A workgroup evaluates the one to three
// heads of its group (its own packed first layer, N <= 768) for its 16 cells and writes those heads' columns
// straight into the rows (ddd_assemble_kernel's arithmetic); group 0 adds score and class, the group that owns
// `reg` (group 0 without `reg`) the centre.  No second pass, nothing shared between workgroups, no atomics.
//
// LDS: the patches take 16 x 576 floats (36 KB).  The hidden rows overwrite them, which holds N <= 576
// hidden channels.  Three 256-wide heads (N = 768) run on a three-slot instantiation whose rows are
// 768 floats wide (16 x 768 floats = 48 KB, still static LDS): the patches are staged once and every
// weight is read once, where walking the heads in groups would stage the patches per group and keep a
// second pass over the chunk loop alive for one shape.  The narrower instantiations keep 36 KB, so the
// ctdet launches are what they were.
#include "cn_common.h"
#include "cn_internal.h"

namespace {

constexpr int HA_NT = 256;      // threads per workgroup
constexpr int HA_CELLS = 16;    // cells per workgroup
constexpr int HA_CC = 64;       // channels of Cin per staged chunk
constexpr int HA_ROW = 9 * HA_CC;   // floats of one cell's patch (one chunk)
constexpr int HA_MAXN = 768;    // hidden channels of all deferred heads together
constexpr int HA_MAXJ = 17;     // joints of the pose task's hps head
constexpr int HA_MAXOUT = 2 + 2 * HA_MAXJ + 2;   // 1x1 outputs per cell: wh, hps, reg
enum { HA_CTDET = 0, HA_POSE = 1, HA_DDD = 2 };
constexpr int HA_PF = 4;        // float4 weight groups in flight per channel slot
constexpr int HA_MAXGROUPS = 5; // ddd: head groups of one launch (one head each at the most)
constexpr int HA_GROUP_HEADS = 3;   // heads of one group (the channel slots of the widest form)
constexpr int HA_DDD_OUT = 16;  // ddd: 1x1 outputs per cell of one group (rot + dim + wh = 13 at the most)

// ddd: one group of consecutive heads -- its weights and, per head, the outputs and where they go
struct HeadsAtGroup {
    const cn_f32x4 *w1;         // (9 * Cin / 4, n_heads * hidden) float4
    const float *b1, *w2, *b2;  // (n_heads * hidden), (out, hidden), (out) or null
    int n_heads;
    int cout[HA_GROUP_HEADS];   // outputs per head
    int col[HA_GROUP_HEADS];    // first column of the head in a row of dets
    int voff[HA_GROUP_HEADS];   // first column of the head in a row of head_vals
};

struct HeadsAtArgs {
    const char *feat;           // NHWC, row pitch `pitch` channels; f32s or plain fp32
    const float *scores;        // (B, K)
    const int32_t *inds, *clses;  // (B, K)
    const cn_f32x4 *w1;         // (9 * Cin / 4, N) float4: cn_pack_cell_heads_w1
    const float *b1;            // (N)
    const float *w2;            // (out, hidden): the 1x1 rows of the heads, concatenated in head order
    const float *b2;            // (out) or null
    float *dets;                // (B, K, 6), pose: (B, K, 5 + 2J + 1)
    float *vals;                // (B, K, out) or null: the raw head values
    float mul;                  // 2^e of an f32s feature map (1 for plain)
    int H, W, Cin, pitch, K, hidden, n_heads, N;
    int c0, c1;                 // outputs of head 0 and head 1 (head 2 has the rest)
    int out;                    // 1x1 outputs per cell, all heads
    int J;                      // pose: joints
    // ddd only (behind everything the other tasks read: their argument offsets are what they were)
    HeadsAtGroup grp[HA_MAXGROUPS];   // indexed by blockIdx.z
    int D;                      // columns of a row of dets: 18 with wh, else 16
    int vals_out;               // columns of a row of head_vals: all heads of all groups
    int raw_depth;              // CN_DECODE_DDD_RAW_DEPTH: column 11 = 1 / (sigmoid(dep) + 1e-6) - 1
    int half_group;             // the group that writes the centre as cell + 0.5 (no reg head), or -1
};

// rows of ctdet_decode (emit_rows<MODE_CTDET>): [x1, y1, x2, y2, score, cls]; o = this cell's head values
__device__ __forceinline__ void ha_ctdet_row(const HeadsAtArgs &a, size_t row, int ind, const float *o)
{
    float *d = a.dets + row * 6;
    const float score = a.scores[row];
    const float cls = (float)a.clses[row];
    if (ind < 0) {
        const float nan = __builtin_nanf("");
        d[0] = nan; d[1] = nan; d[2] = nan; d[3] = nan; d[4] = score; d[5] = cls;
        if (a.vals)
            for (int v = 0; v < a.out; ++v) a.vals[row * a.out + v] = nan;
        return;
    }
    const int yi = ind / a.W, xi = ind - yi * a.W;
    float xs = (float)xi, ys = (float)yi;
    if (a.n_heads > 1) {  // decode.py:472-476
        xs = xs + o[2];
        ys = ys + o[3];
    } else {  // decode.py:477-479
        xs = xs + 0.5f;
        ys = ys + 0.5f;
    }
    const float w = o[0];
    const float h = o[1];
    d[0] = xs - w / 2;  // decode.py:489-492
    d[1] = ys - h / 2;
    d[2] = xs + w / 2;
    d[3] = ys + h / 2;
    d[4] = score;
    d[5] = cls;
    if (a.vals)
        for (int v = 0; v < a.out; ++v) a.vals[row * a.out + v] = o[v];
}

// column `col` of a multi_pose_decode stage-A row (emit_rows<MODE_POSE>): [x1, y1, x2, y2, score, 2J kps,
// cls]; o = this cell's head values [w, h, 2J hps, (reg_x, reg_y)].  One rounding per line, as there.
__device__ __forceinline__ float ha_pose_col(const HeadsAtArgs &a, size_t row, int ind, const float *o, int col)
{
    const int D = 5 + 2 * a.J + 1;
    if (col == 4) return a.scores[row];
    if (col == D - 1) return (float)a.clses[row];
    if (ind < 0) return __builtin_nanf("");
    const int yi = ind / a.W, xi = ind - yi * a.W;
    if (col >= 5) {  // decode.py:506-509: kps = hps[ind] + (xs, ys) with the un-offset centre
        const int v = col - 5;
        return o[2 + v] + (float)((v & 1) ? yi : xi);
    }
    const bool isy = col & 1;
    float c = (float)(isy ? yi : xi);
    if (a.n_heads > 2) c = c + o[2 + 2 * a.J + (isy ? 1 : 0)];   // decode.py:510-514
    else c = c + 0.5f;                                          // decode.py:515-517
    const float half = o[isy ? 1 : 0] / 2;                       // decode.py:523-526
    return col < 2 ? c - half : c + half;
}

// CT cells per thread (16 / CT cell groups of 16 * CT threads), NS channel slots per thread
template <bool F32S, int CT, int NS, int TASK = HA_CTDET>
__global__ __launch_bounds__(HA_NT) void decode_heads_at_cells_kernel(const HeadsAtArgs a)
{
    constexpr int CG = HA_CELLS / CT;     // cell groups
    constexpr int TPC = HA_NT / CG;       // threads across the channels (a multiple of 64: a wave shares its cells)
    static_assert(TPC % 64 == 0, "the lanes of a wave read one cell's patch");
    // a cell's hidden row: as wide as its patch row, or the channels this form holds when those are more
    constexpr int HROW = NS * TPC > HA_ROW ? NS * TPC : HA_ROW;
    static_assert(NS * TPC <= HA_MAXN && HA_CELLS * HROW * 4 <= 48 * 1024, "static LDS");
    __shared__ __attribute__((aligned(16))) float lds[HA_CELLS * HROW];   // patches, then the hidden values
    __shared__ int s_ind[HA_CELLS];
    __shared__ float s_out[HA_CELLS * (TASK == HA_POSE ? HA_MAXOUT : TASK == HA_DDD ? HA_DDD_OUT : 4)];

    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int k0 = blockIdx.x * HA_CELLS;
    const int ncell = min(HA_CELLS, a.K - k0);
    const int HW = a.H * a.W;
    // the heads this workgroup evaluates: the launch's (ctdet, pose) or those of its group (ddd)
    int N = a.N, out = a.out, hc0 = a.c0, hc1 = a.c1;
    const cn_f32x4 *w1 = a.w1;
    const float *b1 = a.b1, *w2 = a.w2, *b2 = a.b2;
    if constexpr (TASK == HA_DDD) {
        const HeadsAtGroup &g = a.grp[blockIdx.z];
        N = g.n_heads * a.hidden;
        hc0 = g.cout[0];
        hc1 = g.cout[1];
        out = hc0 + hc1 + g.cout[2];
        w1 = g.w1; b1 = g.b1; w2 = g.w2; b2 = g.b2;
    }

    if (tid < HA_CELLS) {
        int ind = -1;
        if (tid < ncell) {
            ind = a.inds[(size_t)b * a.K + k0 + tid];
            if ((uint32_t)ind >= (uint32_t)HW) ind = -1;   // never read outside the map (the row becomes NaN)
        }
        s_ind[tid] = ind;
    }

    const int nl = tid % TPC, cg = tid / TPC;
    float acc[NS][CT];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int i = 0; i < CT; ++i) acc[s][i] = 0.f;

    size_t kq_base = 0;   // float4 rows of w1 in front of this chunk
    for (int c0 = 0; c0 < a.Cin; c0 += HA_CC) {
        const int cc = min(HA_CC, a.Cin - c0);     // 64, or 32 in the last chunk
        const int cq = cc >> 2;
        __syncthreads();   // s_ind is written / the previous chunk's patches are consumed
        // stage: patch[cell][tap * cc + ci], zeros outside the map and for absent cells
        for (int i = tid; i < HA_CELLS * 9 * cq; i += HA_NT) {
            const int q = i % cq, r = i / cq;
            const int tap = r % 9, cell = r / 9;
            const int ind = s_ind[cell];
            cn_f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ind >= 0) {
                const int y = ind / a.W + tap / 3 - 1, x = ind % a.W + tap % 3 - 1;
                if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
                    const size_t pix = ((size_t)b * a.H + y) * a.W + x;
                    if (F32S) {
                        v = cn_load4_f32s(a.feat, pix, a.pitch, c0 + 4 * q);
                        v *= a.mul;
                    } else {
                        v = *reinterpret_cast<const cn_f32x4 *>(a.feat + (pix * (size_t)a.pitch + c0 + 4 * q) * 4);
                    }
                }
            }
            *reinterpret_cast<cn_f32x4 *>(&lds[cell * HA_ROW + tap * cc + 4 * q]) = v;
        }
        __syncthreads();

        const int nkq = 9 * cq;    // float4 groups of this chunk (a multiple of HA_PF: 72 or 144)
        const cn_f32x4 *wq = w1 + kq_base * N;
        cn_f32x4 wn[HA_PF][NS];
#pragma unroll
        for (int p = 0; p < HA_PF; ++p)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int n = nl + s * TPC;
                wn[p][s] = n < N ? wq[(size_t)p * N + n] : cn_f32x4{0.f, 0.f, 0.f, 0.f};
            }
        for (int kq = 0; kq < nkq; kq += HA_PF) {
            cn_f32x4 wv[HA_PF][NS];
#pragma unroll
            for (int p = 0; p < HA_PF; ++p)
#pragma unroll
                for (int s = 0; s < NS; ++s) wv[p][s] = wn[p][s];
            if (kq + HA_PF < nkq) {
#pragma unroll
                for (int p = 0; p < HA_PF; ++p)
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int n = nl + s * TPC;
                        if (n < N) wn[p][s] = wq[(size_t)(kq + HA_PF + p) * N + n];
                    }
            }
#pragma unroll
            for (int p = 0; p < HA_PF; ++p)
#pragma unroll
                for (int i = 0; i < CT; ++i) {
                    const cn_f32x4 pv = *reinterpret_cast<const cn_f32x4 *>(&lds[(i * CG + cg) * HA_ROW + 4 * (kq + p)]);
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        float t = acc[s][i];
                        t = __builtin_fmaf(wv[p][s][0], pv[0], t);
                        t = __builtin_fmaf(wv[p][s][1], pv[1], t);
                        t = __builtin_fmaf(wv[p][s][2], pv[2], t);
                        t = __builtin_fmaf(wv[p][s][3], pv[3], t);
                        acc[s][i] = t;
                    }
                }
        }
        kq_base += (size_t)nkq;
    }

    // hidden[cell][n] = ReLU(acc + b1[n]) replaces the patches (N <= NS * TPC <= HROW)
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int n = nl + s * TPC;
        if (n < N) {
            const float bias = b1[n];
#pragma unroll
            for (int i = 0; i < CT; ++i)
                lds[(i * CG + cg) * HROW + n] = __builtin_fmaxf(acc[s][i] + bias, 0.f);
        }
    }
    __syncthreads();

    // 1x1: output o = (cell, r) of 16 x out, four lanes each, 64 outputs per pass (all 256 threads take
    // part in the shuffles; a pass's absent outputs contribute nothing)
    const int nout = HA_CELLS * out;
    for (int o0 = 0; o0 < nout; o0 += HA_NT / 4) {
        const int o = o0 + (tid >> 2), sub = tid & 3;
        const bool live = o < nout;
        const int cell = o / out, r = o - cell * out;
        const int head = (r >= hc0) + (r >= hc0 + hc1);
        float sum = 0.f;
        if (live) {
            const float *w = w2 + (size_t)r * a.hidden;
            const float *h = &lds[cell * HROW + head * a.hidden];
            for (int c = sub; c < a.hidden; c += 4) sum = __builtin_fmaf(w[c], h[c], sum);
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        if (live && sub == 0) {
            if (b2) sum += b2[r];
            s_out[o] = sum;
        }
    }
    __syncthreads();

    if constexpr (TASK == HA_DDD) {
        // ddd_assemble_kernel's row [xs, ys, score, rot(8), depth, dim(3), (wh(2),) cls]: this group's columns
        const HeadsAtGroup &g = a.grp[blockIdx.z];
        const int D = a.D;
        for (int i = tid; i < ncell * out; i += HA_NT) {
            const int cell = i / out, r = i - cell * out;
            const int head = (r >= hc0) + (r >= hc0 + hc1);
            const int j = r - (head > 0 ? hc0 : 0) - (head > 1 ? hc1 : 0);
            const int col = (head == 0 ? g.col[0] : head == 1 ? g.col[1] : g.col[2]) + j;
            const int vcol = (head == 0 ? g.voff[0] : head == 1 ? g.voff[1] : g.voff[2]) + j;
            const size_t row = (size_t)b * a.K + k0 + cell;
            const int ind = s_ind[cell];
            const float raw = ind < 0 ? __builtin_nanf("") : s_out[i];
            float v = raw;
            if (ind >= 0) {
                if (col < 2) {   // reg: decode.py:433-436
                    const int yi = ind / a.W, xi = ind - yi * a.W;
                    v = (float)(col ? yi : xi) + raw;
                } else if (col == 11 && a.raw_depth) {   // detectors/ddd.py:60, as CN_DECODE_DDD_RAW_DEPTH
                    v = 1.0f / (sigmoidf_ref(raw) + 1e-6f) - 1.0f;
                }
            }
            a.dets[row * D + col] = v;
            if (a.vals) a.vals[row * a.vals_out + vcol] = raw;
        }
        // the columns no head of this group owns
        if (tid < ncell) {
            const size_t row = (size_t)b * a.K + k0 + tid;
            float *d = a.dets + row * D;
            if (blockIdx.z == 0) {
                d[2] = a.scores[row];
                d[D - 1] = (float)a.clses[row];
            }
            if ((int)blockIdx.z == a.half_group) {   // decode.py:437-439
                const int ind = s_ind[tid];
                const int yi = ind / a.W, xi = ind - yi * a.W;
                d[0] = ind < 0 ? __builtin_nanf("") : (float)xi + 0.5f;
                d[1] = ind < 0 ? __builtin_nanf("") : (float)yi + 0.5f;
            }
        }
    } else if (TASK == HA_CTDET) {
        if (tid < ncell) ha_ctdet_row(a, (size_t)b * a.K + k0 + tid, s_ind[tid], &s_out[tid * a.out]);
    } else {
        const int D = 5 + 2 * a.J + 1;
        for (int i = tid; i < ncell * D; i += HA_NT) {
            const int cell = i / D, col = i - cell * D;
            const size_t row = (size_t)b * a.K + k0 + cell;
            a.dets[row * D + col] = ha_pose_col(a, row, s_ind[cell], &s_out[cell * a.out], col);
        }
        if (a.vals)
            for (int i = tid; i < ncell * a.out; i += HA_NT) {
                const int cell = i / a.out;
                a.vals[((size_t)b * a.K + k0) * a.out + i] = s_ind[cell] < 0 ? __builtin_nanf("") : s_out[i];
            }
    }
}

// w (N, Cin, 3, 3) -> out (9 * Cin / 4, N, 4): k = (64-channel chunk of Cin, tap, channel in the chunk),
// four consecutive k of one output channel per float4
__global__ void decode_pack_cell_w1_kernel(const float *__restrict__ w, float *__restrict__ out, int N, int Cin,
                                           size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int e = (int)(i & 3);
    const int n = (int)((i >> 2) % N);
    const int k = (int)((i >> 2) / N) * 4 + e;
    const int chunk = k / (9 * HA_CC);          // only the last chunk can be shorter, so this is exact
    const int c0 = chunk * HA_CC;
    const int cc = min(HA_CC, Cin - c0);
    const int r = k - chunk * 9 * HA_CC;
    const int tap = r / cc, ci = c0 + r % cc;
    out[i] = w[((size_t)n * Cin + ci) * 9 + tap];
}

}  // namespace

extern "C" int cn_pack_cell_heads_w1(const float *w, float *out, int N, int Cin, void *stream)
{
    if (!w || !out) return CN_ERR_NULL;
    if (N <= 0 || Cin <= 0) return CN_ERR_SHAPE;
    if (N > HA_MAXN || (N & 63) || (Cin & 31)) return CN_ERR_UNSUPPORTED;
    if (!cn_aligned16(out)) return CN_ERR_ALIGN;
    const size_t total = (size_t)N * Cin * 9;
    hipLaunchKernelGGL(decode_pack_cell_w1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, w, out, N, Cin, total);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

namespace {

// the instantiation that holds N hidden channels (N = 64 is one head of 64: ctdet and ddd; N > 512 is three
// 256-wide heads: pose and ddd -- each form exists for the tasks that reach it)
template <int TASK>
void ha_launch(const HeadsAtArgs &a, int N, dim3 grid, bool s, hipStream_t st)
{
    const dim3 block(HA_NT);
#define HA_LAUNCH(CT, NS)                                                                                     \
    do {                                                                                                      \
        if (s) hipLaunchKernelGGL((decode_heads_at_cells_kernel<true, CT, NS, TASK>), grid, block, 0, st, a); \
        else hipLaunchKernelGGL((decode_heads_at_cells_kernel<false, CT, NS, TASK>), grid, block, 0, st, a);  \
    } while (0)
    if (N <= 64) {
        if constexpr (TASK != HA_POSE) HA_LAUNCH(4, 1);
    } else if (N <= 128) HA_LAUNCH(8, 1);
    else if (N <= 256) HA_LAUNCH(16, 1);
    else if (N <= 512) HA_LAUNCH(16, 2);
    else if constexpr (TASK != HA_CTDET) HA_LAUNCH(16, 3);
#undef HA_LAUNCH
}

// What the single-buffer entries (ctdet, pose) and the grouped one (ddd) share: the argument checks, in the order
// the error classes are reported -- null, shape, dtype, hidden width and the task's head / group limits, Cin and
// pitch, H * W and B, alignment -- and the HeadsAtArgs fields every task reads.  The task's own part of a class
// comes in as a flag (`ptrs`: its pointers are there, `counts`: its counts are positive) or, where it may only be
// looked at once the classes in front of it have passed, as a callable: `limits()` returns CN_OK or the task's
// error, `w1_aligned()` whether its packed first layers are 16-byte aligned.
template <class Limits, class Aligned>
int ha_prepare(HeadsAtArgs &a, const void *feat, int B, int H, int W, int Cin, int pitch, int dtype, float feat_mul,
               const float *scores, const int32_t *inds, const int32_t *clses, int K, int hidden, int n_heads,
               float *dets, float *head_vals, bool ptrs, bool counts, Limits limits, Aligned w1_aligned)
{
    if (!feat || !scores || !inds || !clses || !dets || !ptrs) return CN_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || K <= 0 || pitch < Cin || !counts) return CN_ERR_SHAPE;
    if (dtype != CN_DTYPE_F32S && dtype != CN_DTYPE_F32) return CN_ERR_UNSUPPORTED;
    if (hidden < 64 || hidden > 256 || (hidden & 63)) return CN_ERR_UNSUPPORTED;
    if (const int rc = limits()) return rc;
    if ((Cin & 31) || (pitch & 3) || (dtype == CN_DTYPE_F32S && (pitch & 31))) return CN_ERR_UNSUPPORTED;
    if ((long)H * W >= (1L << 31) || B > 65535) return CN_ERR_UNSUPPORTED;
    if (!cn_aligned16(feat) || !w1_aligned()) return CN_ERR_ALIGN;
    a.feat = (const char *)feat; a.scores = scores; a.inds = inds; a.clses = clses;
    a.dets = dets; a.vals = head_vals; a.mul = dtype == CN_DTYPE_F32S ? feat_mul : 1.f;
    a.H = H; a.W = W; a.Cin = Cin; a.pitch = pitch; a.K = K; a.hidden = hidden; a.n_heads = n_heads;
    return CN_OK;
}

// the checks and the launch of the ctdet and pose entries
template <int TASK>
int heads_at_cells(const void *feat, int B, int H, int W, int Cin, int pitch, int dtype, float feat_mul,
                   const float *scores, const int32_t *inds, const int32_t *clses, int K,
                   const float *w1_packed, const float *bias1, int hidden, int n_heads, int J, const float *w2,
                   const float *bias2, float *dets, float *head_vals, void *stream)
{
    constexpr int H0 = TASK == HA_POSE ? 2 : 1;     // ctdet: wh[, reg]; pose: wh, hps[, reg]
    HeadsAtArgs a;
    const int rc = ha_prepare(
        a, feat, B, H, W, Cin, pitch, dtype, feat_mul, scores, inds, clses, K, hidden, n_heads, dets, head_vals,
        w1_packed && bias1 && w2, true,
        [&] {
            if (n_heads < H0 || n_heads > H0 + 1) return CN_ERR_UNSUPPORTED;
            return TASK == HA_POSE && (J < 1 || J > HA_MAXJ) ? CN_ERR_UNSUPPORTED : CN_OK;
        },
        [&] { return cn_aligned16(w1_packed); });
    if (rc) return rc;
    a.w1 = (const cn_f32x4 *)w1_packed; a.b1 = bias1; a.w2 = w2; a.b2 = bias2;
    a.N = hidden * n_heads;
    a.J = J;
    a.c0 = 2;
    a.c1 = TASK == HA_POSE ? 2 * J : 2;
    a.out = TASK == HA_POSE ? 2 + 2 * J + (n_heads > 2 ? 2 : 0) : 2 * n_heads;
    ha_launch<TASK>(a, a.N, dim3((unsigned)cn_cdiv(K, HA_CELLS), (unsigned)B), dtype == CN_DTYPE_F32S,
                    (hipStream_t)stream);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace

extern "C" int cn_ctdet_heads_at_cells_f32(const void *feat, int B, int H, int W, int Cin, int pitch, int dtype,
                                           float feat_mul, const float *scores, const int32_t *inds,
                                           const int32_t *clses, int K, const float *w1_packed,
                                           const float *bias1, int hidden, int n_heads, const float *w2,
                                           const float *bias2, float *dets, float *head_vals, void *stream)
{
    return heads_at_cells<HA_CTDET>(feat, B, H, W, Cin, pitch, dtype, feat_mul, scores, inds, clses, K, w1_packed,
                                    bias1, hidden, n_heads, 0, w2, bias2, dets, head_vals, stream);
}

extern "C" int cn_multi_pose_heads_at_cells_f32(const void *feat, int B, int H, int W, int Cin, int pitch,
                                                int dtype, float feat_mul, const float *scores,
                                                const int32_t *inds, const int32_t *clses, int K,
                                                const float *w1_packed, const float *bias1, int hidden,
                                                int n_heads, int J, const float *w2, const float *bias2,
                                                float *dets, float *head_vals, void *stream)
{
    return heads_at_cells<HA_POSE>(feat, B, H, W, Cin, pitch, dtype, feat_mul, scores, inds, clses, K, w1_packed,
                                   bias1, hidden, n_heads, J, w2, bias2, dets, head_vals, stream);
}

extern "C" int cn_ddd_heads_at_cells_f32(const void *feat, int B, int H, int W, int Cin, int pitch, int dtype,
                                         float feat_mul, const float *scores, const int32_t *inds,
                                         const int32_t *clses, int K, int hidden, int n_groups,
                                         const cn_cell_head_group *groups, int has_wh, int has_reg, int flags,
                                         float *dets, float *head_vals, void *stream)
{
    const int n_heads = 3 + (has_wh ? 1 : 0) + (has_reg ? 1 : 0);
    int widest = 0;
    HeadsAtArgs a = {};
    const int rc = ha_prepare(
        a, feat, B, H, W, Cin, pitch, dtype, feat_mul, scores, inds, clses, K, hidden, n_heads, dets, head_vals,
        groups != nullptr, n_groups > 0,
        [&] {
            if (n_groups > HA_MAXGROUPS) return CN_ERR_UNSUPPORTED;
            int total = 0;
            for (int g = 0; g < n_groups; ++g) {
                const int n = groups[g].n_heads;
                if (n < 1 || n > HA_GROUP_HEADS || n * hidden > HA_MAXN) return CN_ERR_UNSUPPORTED;
                total += n;
                widest = n > widest ? n : widest;
            }
            if (total != n_heads) return CN_ERR_UNSUPPORTED;
            for (int g = 0; g < n_groups; ++g)
                if (!groups[g].w1_packed || !groups[g].bias1 || !groups[g].w2) return CN_ERR_NULL;
            return CN_OK;
        },
        [&] {
            for (int g = 0; g < n_groups; ++g)
                if (!cn_aligned16(groups[g].w1_packed)) return false;
            return true;
        });
    if (rc) return rc;
    // the heads in their order: dep, rot, dim[, wh][, reg] -- outputs and first column in a row of dets
    const int couts[5] = {1, 8, 3, 2, 2};
    const int cols[5] = {11, 3, 12, has_wh ? 15 : 0, 0};
    a.D = has_wh ? 18 : 16;
    a.raw_depth = (flags & CN_DECODE_DDD_RAW_DEPTH) ? 1 : 0;
    a.half_group = has_reg ? -1 : 0;
    int head = 0, voff = 0;
    for (int g = 0; g < n_groups; ++g) {
        HeadsAtGroup &d = a.grp[g];
        d.w1 = (const cn_f32x4 *)groups[g].w1_packed;
        d.b1 = groups[g].bias1; d.w2 = groups[g].w2; d.b2 = groups[g].bias2;
        d.n_heads = groups[g].n_heads;
        for (int h = 0; h < d.n_heads; ++h, ++head) {
            const int t = head < 3 || has_wh ? head : 4;   // without wh the fourth head is reg
            d.cout[h] = couts[t];
            d.col[h] = cols[t];
            d.voff[h] = voff;
            voff += couts[t];
        }
    }
    a.vals_out = voff;
    ha_launch<HA_DDD>(a, widest * hidden, dim3((unsigned)cn_cdiv(K, HA_CELLS), (unsigned)B, (unsigned)n_groups),
                      dtype == CN_DTYPE_F32S, (hipStream_t)stream);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
