// cn_decode_tasks.hip -- the decoders built on the top-K of cn_decode.hip: multi_pose (keypoint matching),
// ddd, exct and agnex.  Each ranks its heat-maps through topk_run() (cn_internal.h) or the public cn_topk_f32
// and adds its own kernels behind; the exact select of exct_select_kernel is cn_select.h's.
#include "cn_internal.h"
#include "cn_select.h"

// ---------------------------------------------------------------------------
// multi_pose decode (models/decode.py:497-571)
//   stage A  top-K of the centre map, MODE_POSE: boxes, scores, regression keypoints
//   stage B  top-K per channel of hm_hp, MODE_CHANNEL: K candidates per joint (_topk_channel)
//   stage C  pose_match_kernel: nearest candidate per (detection, joint), reject rule, blend
// Arithmetic is kept in the reference's association (no FMA contraction) so the result
// is bit-identical to torch on CPU: the argmin and the threshold tests are discontinuous.
// ---------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(KMAX) void pose_match_kernel(
    const float *__restrict__ hp_scores, const int32_t *__restrict__ hp_inds,
    const float *__restrict__ hp_offset, float *__restrict__ dets, int J, int K, int H, int W,
    int det_dim)
{
    __shared__ float cs[KMAX], cx[KMAX], cy[KMAX];
    const int j = blockIdx.x, b = blockIdx.y;
    const int q = threadIdx.x;
    const int HW = H * W;
    const float thresh = 0.1f;
    if (q < K) {
        const size_t o = ((size_t)b * J + j) * K + q;
        float s = hp_scores[o];
        const int ind = hp_inds[o];
        const int yi = ind / W, xi = ind - yi * W;
        float x = (float)xi, y = (float)yi;
        if (hp_offset) {  // decode.py:534-539
            x = add_rn(x, hp_offset[((size_t)b * 2 + 0) * HW + ind]);
            y = add_rn(y, hp_offset[((size_t)b * 2 + 1) * HW + ind]);
        } else {
            x = add_rn(x, 0.5f);
            y = add_rn(y, 0.5f);
        }
        const float m = (s > thresh) ? 1.0f : 0.0f;  // decode.py:544-547
        const float im = __fsub_rn(1.0f, m);
        cs[q] = add_rn(mul_rn(im, -1.0f), mul_rn(m, s));
        cy[q] = add_rn(mul_rn(im, -10000.0f), mul_rn(m, y));
        cx[q] = add_rn(mul_rn(im, -10000.0f), mul_rn(m, x));
    }
    __syncthreads();
    if (q < K) {
        float *d = dets + ((size_t)b * K + q) * det_dim;
        const float rx = d[5 + 2 * j], ry = d[5 + 2 * j + 1];
        float best = 0.f;
        int bi = -1;
        for (int c = 0; c < K; ++c) {  // decode.py:550-551, first minimum
            const float dx = __fsub_rn(rx, cx[c]);
            const float dy = __fsub_rn(ry, cy[c]);
            const float dist = __fsqrt_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)));
            if (bi < 0 || dist < best) {
                best = dist;
                bi = c;
            }
        }
        const float sc = cs[bi], kx = cx[bi], ky = cy[bi];
        const float l = d[0], t = d[1], r = d[2], bt = d[3];
        const float bh = __fsub_rn(bt, t), bw = __fsub_rn(r, l);
        const float mx = mul_rn(fmaxf(bh, bw), 0.3f);
        const bool reject = (kx < l) || (kx > r) || (ky < t) || (ky > bt) || (sc < thresh) ||
                            (best > mx);  // decode.py:562-565
        const float m = reject ? 1.0f : 0.0f;
        const float im = __fsub_rn(1.0f, m);
        d[5 + 2 * j] = add_rn(mul_rn(im, kx), mul_rn(m, rx));  // decode.py:566
        d[5 + 2 * j + 1] = add_rn(mul_rn(im, ky), mul_rn(m, ry));
    }
}

// a pose stage as a top-K call: the centre map (MODE_POSE, C classes) or the joint maps (MODE_CHANNEL, J
// channels).  Both work in the candidate arrays at the head of the pose workspace.
TopkCall pose_stage(const float *heat, int B, int C, int H, int W, int K, int flags, int mode, void *stream)
{
    TopkCall c = {};
    c.heat = heat;
    c.B = B; c.C = C; c.H = H; c.W = W; c.K = K;
    c.flags = flags;
    c.mode = mode;
    c.cand_only = true;
    c.st = (hipStream_t)stream;
    return c;
}

// the pose workspace: candidate arrays sized for the larger of the two stages, then the joints' (B, J, K) lists
struct PoseWs {
    size_t hp_s, hp_i, total;
};
bool pose_ws_plan(const TopkCall &centre, const TopkCall &joints, PoseWs *p)
{
    const TopkPlan pa = topk_route(centre), pb = topk_route(joints);
    if (pa.rc != CN_OK || pb.rc != CN_OK) return false;
    const size_t list = cn_align_up((size_t)joints.B * joints.C * joints.K * 4, 256);
    size_t o = pa.cand_bytes > pb.cand_bytes ? pa.cand_bytes : pb.cand_bytes;   // reused by both stages
    p->hp_s = o; o += list;
    p->hp_i = o; o += list;
    p->total = o;
    return true;
}

// stages B and C on rows that hold stage A (cn_multi_pose_decode_f32 and cn_multi_pose_match_f32 both end here)
int pose_match_stages(TopkCall joints, const float *hp_offset, float *dets, void *workspace, const PoseWs &p)
{
    const int B = joints.B, J = joints.C, H = joints.H, W = joints.W, K = joints.K;
    float *hp_s = (float *)((char *)workspace + p.hp_s);
    int32_t *hp_i = (int32_t *)((char *)workspace + p.hp_i);
    // stage B: per-joint top-K of the keypoint heat-map
    joints.ea.out_scores = hp_s;
    joints.ea.inds_out = hp_i;
    joints.workspace = workspace;
    joints.workspace_bytes = p.hp_s;
    const int rc = topk_run(joints);
    if (rc != CN_OK) return rc;
    // stage C
    hipLaunchKernelGGL(pose_match_kernel, dim3(J, B), dim3(KMAX), 0, joints.st, hp_s, hp_i, hp_offset, dets, J, K,
                       H, W, 4 + 1 + 2 * J + 1);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace

extern "C" size_t cn_multi_pose_decode_workspace_bytes(int B, int C, int H, int W, int J, int K)
{
    PoseWs p;
    if (J <= 0) return 0;
    if (!pose_ws_plan(pose_stage(nullptr, B, C, H, W, K, 0, MODE_POSE, nullptr),
                      pose_stage(nullptr, B, J, H, W, K, 0, MODE_CHANNEL, nullptr), &p))
        return 0;
    return p.total;
}

extern "C" int cn_multi_pose_decode_f32(const float *heat, const float *wh, const float *kps,
                                        const float *reg, const float *hm_hp,
                                        const float *hp_offset, int B, int C, int H, int W, int J,
                                        int K, int apply_sigmoid, float *dets, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    TopkCall centre = pose_stage(heat, B, C, H, W, K, apply_sigmoid, MODE_POSE, stream);
    int rc = topk_checks(centre);
    if (rc != CN_OK) return rc;
    if (!wh || !kps || !dets || !workspace) return CN_ERR_NULL;
    if (J <= 0) return CN_ERR_SHAPE;
    const TopkCall joints = pose_stage(hm_hp, B, J, H, W, K, apply_sigmoid, MODE_CHANNEL, stream);
    PoseWs p;
    if (!pose_ws_plan(centre, joints, &p)) return CN_ERR_UNSUPPORTED;
    if (workspace_bytes < p.total) return CN_ERR_WORKSPACE;
    if (hm_hp && ((W & 3) == 0) && !cn_aligned16(hm_hp)) return CN_ERR_ALIGN;
    // stage A
    centre.ea.wh = wh;
    centre.ea.reg = reg;
    centre.ea.dets = dets;
    centre.ea.kps_map = kps;
    centre.ea.J = J;
    centre.workspace = workspace;
    centre.workspace_bytes = p.hp_s;
    rc = topk_run(centre);
    if (rc != CN_OK) return rc;
    if (!hm_hp) return CN_OK;
    return pose_match_stages(joints, hp_offset, dets, workspace, p);
}

extern "C" int cn_multi_pose_match_f32(const float *hm_hp, const float *hp_offset, int B, int J, int H, int W,
                                       int K, int flags, float *dets, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    if (J <= 0) return hm_hp ? CN_ERR_SHAPE : CN_ERR_NULL;
    const TopkCall joints = pose_stage(hm_hp, B, J, H, W, K, flags & CN_DECODE_SIGMOID, MODE_CHANNEL, stream);
    const int rc = topk_checks(joints);
    if (rc != CN_OK) return rc;
    if (!dets || !workspace) return CN_ERR_NULL;
    PoseWs p;   // the layout of cn_multi_pose_decode_f32 with a one-class centre map
    if (!pose_ws_plan(pose_stage(nullptr, B, 1, H, W, K, 0, MODE_POSE, nullptr), joints, &p)) return CN_ERR_UNSUPPORTED;
    if (workspace_bytes < p.total) return CN_ERR_WORKSPACE;
    return pose_match_stages(joints, hp_offset, dets, workspace, p);
}


// ---------------------------------------------------------------------------
// ddd_decode (models/decode.py:426-462): cn_topk_f32, then one thread per row gathers the 3-D heads
// ---------------------------------------------------------------------------
namespace {

// one thread per (b,k): [xs, ys, score, rot(8), depth, dim(3), (wh(2),) cls]  (decode.py:433-460)
__global__ void ddd_assemble_kernel(const float *__restrict__ scores, const int32_t *__restrict__ inds,
                                    const int32_t *__restrict__ clses, const float *__restrict__ rot,
                                    const float *__restrict__ depth, const float *__restrict__ dim,
                                    const float *__restrict__ wh, const float *__restrict__ reg,
                                    float *__restrict__ dets, int B, int K, int H, int W, int raw_depth)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K;
    const int HW = H * W;
    const int ind = inds[i];
    const int yi = ind / W, xi = ind - yi * W;
    float xs = (float)xi, ys = (float)yi;
    if (reg) {
        xs = xs + reg[((size_t)b * 2 + 0) * HW + ind];
        ys = ys + reg[((size_t)b * 2 + 1) * HW + ind];
    } else {
        xs = xs + 0.5f;
        ys = ys + 0.5f;
    }
    const int D = wh ? 18 : 16;
    float *d = dets + (size_t)i * D;
    d[0] = xs; d[1] = ys; d[2] = scores[i];
    for (int c = 0; c < 8; ++c) d[3 + c] = rot[((size_t)b * 8 + c) * HW + ind];
    float dep = depth[(size_t)b * HW + ind];
    // CN_DECODE_DDD_RAW_DEPTH: the head's raw value; detectors/ddd.py:60 on the K gathered cells only
    if (raw_depth) dep = 1.0f / (sigmoidf_ref(dep) + 1e-6f) - 1.0f;
    d[11] = dep;
    for (int c = 0; c < 3; ++c) d[12 + c] = dim[((size_t)b * 3 + c) * HW + ind];
    if (wh) {
        d[15] = wh[((size_t)b * 2 + 0) * HW + ind];
        d[16] = wh[((size_t)b * 2 + 1) * HW + ind];
    }
    d[D - 1] = (float)clses[i];
}

}  // namespace

extern "C" size_t cn_ddd_decode_workspace_bytes(int B, int C, int H, int W, int K)
{
    const size_t base = cn_ctdet_decode_workspace_bytes(B, C, H, W, K);
    if (!base) return 0;
    return base + 3 * cn_align_up((size_t)B * K * 4, 256);
}

extern "C" int cn_ddd_decode_f32(const float *heat, const float *rot, const float *depth,
                                 const float *dim, const float *wh, const float *reg, int B, int C,
                                 int H, int W, int K, int apply_sigmoid, float *dets,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rot || !depth || !dim || !dets || !workspace) return CN_ERR_NULL;
    const size_t base = cn_ctdet_decode_workspace_bytes(B, C, H, W, K);
    if (!base) return CN_ERR_UNSUPPORTED;
    if (workspace_bytes < cn_ddd_decode_workspace_bytes(B, C, H, W, K)) return CN_ERR_WORKSPACE;
    const size_t slot = cn_align_up((size_t)B * K * 4, 256);
    float *scores = (float *)((char *)workspace + base);
    int32_t *inds = (int32_t *)((char *)workspace + base + slot);
    int32_t *clses = (int32_t *)((char *)workspace + base + 2 * slot);
    int rc = cn_topk_f32(heat, B, C, H, W, K, apply_sigmoid & ~CN_DECODE_DDD_RAW_DEPTH, scores, inds, clses,
                         workspace, base, stream);
    if (rc != CN_OK) return rc;
    hipLaunchKernelGGL(ddd_assemble_kernel, dim3(cn_cdiv(B * K, 128)), dim3(128), 0,
                       (hipStream_t)stream, scores, inds, clses, rot, depth, dim, wh, reg, dets, B, K,
                       H, W, (apply_sigmoid & CN_DECODE_DDD_RAW_DEPTH) ? 1 : 0);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// ---------------------------------------------------------------------------
// exct_decode (models/decode.py:273-424; aggr_weight > 0: cn_exct_aggregate_f32 in front): ExtremeNet-style grouping of the
// K best top / left / bottom / right extreme points into boxes.
//   stage A  cn_topk_f32 x4 (_nms + _topk of the four extreme-point heat-maps)
//   stage B  exct_score_kernel: the K^4 candidate scores (decode.py:316-366), written once
//   stage C  exct_select_kernel: exact top-num_dets (radix select + 1024-key bitonic sort in
//            LDS) and the box / extreme-point assembly (decode.py:372-420)
//   cn_exct_decode_stream_f32: stages B and C without the K^4 array (the exct_stream_* kernels below), K <= 128
// Candidate index = ((t*K + l)*K + b)*K + r, as the reference's view(batch, -1).
// Tie order (unspecified by torch.topk): score desc, candidate index asc.
// ---------------------------------------------------------------------------
namespace {

constexpr int EXCT_MAX_DETS = 1024;

struct ExctLists {  // (B, K) arrays of the four _topk calls, order t, l, b, r
    const float *score[4];
    const int32_t *ind[4];
    const int32_t *cls[4];
};

__device__ __forceinline__ float exct_score(const ExctLists &L, const float *__restrict__ ct_heat,
                                            int b, int K, int H, int W, int C, int it, int il,
                                            int ib, int ir, float scores_thresh, float center_thresh)
{
    const int o = b * K;
    const float ts = L.score[0][o + it], ls = L.score[1][o + il], bs = L.score[2][o + ib],
                rs = L.score[3][o + ir];
    const int ti = L.ind[0][o + it], li = L.ind[1][o + il], bi = L.ind[2][o + ib],
              ri = L.ind[3][o + ir];
    const int tc = L.cls[0][o + it], lc = L.cls[1][o + il], bc = L.cls[2][o + ib],
              rc = L.cls[3][o + ir];
    const float t_y = (float)(ti / W), t_x = (float)(ti % W);
    const float l_y = (float)(li / W), l_x = (float)(li % W);
    const float b_y = (float)(bi / W), b_x = (float)(bi % W);
    const float r_y = (float)(ri / W), r_x = (float)(ri % W);
    // decode.py:331-336: centre of the box -> centre heat-map of the TOP point's class
    const int cx = (int)((l_x + r_x + 0.5f) / 2.0f);
    const int cy = (int)((t_y + b_y + 0.5f) / 2.0f);
    const float cs = ct_heat[((size_t)b * C + tc) * H * W + (size_t)cy * W + cx];
    // decode.py:343: (t + l + b + r + 2*ct) / 6, left to right
    float s = ((((ts + ls) + bs) + rs) + 2.0f * cs) / 6.0f;
    // decode.py:346-366: one unit off per violated rule, in the reference's order
    const bool sc_bad = (ts < scores_thresh) || (ls < scores_thresh) || (bs < scores_thresh) ||
                        (rs < scores_thresh) || (cs < center_thresh);
    const bool cls_bad = (tc != lc) || (tc != bc) || (tc != rc);
    const bool top_bad = (t_y > l_y) || (t_y > b_y) || (t_y > r_y);
    const bool left_bad = (l_x > t_x) || (l_x > b_x) || (l_x > r_x);
    const bool bottom_bad = (b_y < t_y) || (b_y < l_y) || (b_y < r_y);
    const bool right_bad = (r_x < t_x) || (r_x < l_x) || (r_x < b_x);
    s = s - (sc_bad ? 1.0f : 0.0f);
    s = s - (cls_bad ? 1.0f : 0.0f);
    s = s - (top_bad ? 1.0f : 0.0f);
    s = s - (left_bad ? 1.0f : 0.0f);
    s = s - (bottom_bad ? 1.0f : 0.0f);
    s = s - (right_bad ? 1.0f : 0.0f);
    return s;
}

__global__ void exct_score_kernel(const ExctLists L, const float *__restrict__ ct_heat,
                                  float *__restrict__ cand, int K, int H, int W, int C,
                                  float scores_thresh, float center_thresh)
{
    const int b = blockIdx.y;
    const size_t n = (size_t)K * K * K * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const int ir = (int)(i % K), ib = (int)((i / K) % K), il = (int)((i / ((size_t)K * K)) % K),
                  it = (int)(i / ((size_t)K * K * K));
        cand[(size_t)b * n + i] =
            exct_score(L, ct_heat, b, K, H, W, C, it, il, ib, ir, scores_thresh, center_thresh);
    }
}

struct ExctRegr {
    const float *r[4];  // t, l, b, r regression maps (B,2,H,W) or all null
};

// Row `row` of image b from its 64-bit key (decode.py:372-420): the box, the score, the four extreme points and the
// class.  ``cls_map`` (B, H, W) or null: the class-agnostic form (agnex_ct_decode, decode.py:171-187,262-263) takes a
// detection's class from the centre map's arg-max at the box centre instead of from the top point's list
__device__ __forceinline__ void exct_write_row(u64 key, const ExctLists &L, const ExctRegr &R, float *__restrict__ dets,
                                               int b, int row, int K, int H, int W, int num_dets,
                                               const int32_t *__restrict__ cls_map)
{
    const float score = key2f((uint32_t)(key >> 32));
    const uint32_t idx = 0xFFFFFFFFu - (uint32_t)key;
    const int ir = (int)(idx % K), ib = (int)((idx / K) % K), il = (int)((idx / (K * K)) % K),
              it = (int)(idx / (K * K * K));
    const int o = b * K;
    const int HW = H * W;
    const int sel[4] = {it, il, ib, ir};
    float xs[4], ys[4], gx[4], gy[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ind = L.ind[e][o + sel[e]];
        float x = (float)(ind % W), y = (float)(ind / W);
        gx[e] = x;
        gy[e] = y;
        if (R.r[0]) {  // decode.py:372-390 (all four regression maps given)
            x = x + R.r[e][((size_t)b * 2 + 0) * HW + ind];
            y = y + R.r[e][((size_t)b * 2 + 1) * HW + ind];
        } else {      // decode.py:391-399
            x = x + 0.5f;
            y = y + 0.5f;
        }
        xs[e] = x;
        ys[e] = y;
    }
    float *d = dets + ((size_t)b * num_dets + row) * 14;
    d[0] = xs[1]; d[1] = ys[0]; d[2] = xs[3]; d[3] = ys[2];  // bboxes = (l_x, t_y, r_x, b_y)
    d[4] = score;
    d[5] = xs[0]; d[6] = ys[0]; d[7] = xs[1]; d[8] = ys[1];
    d[9] = xs[2]; d[10] = ys[2]; d[11] = xs[3]; d[12] = ys[3];
    if (cls_map) {   // decode.py:171-172: the box centre on the grid, from the points BEFORE their offsets
        const int cx = (int)((gx[1] + gx[3] + 0.5f) / 2.0f);
        const int cy = (int)((gy[0] + gy[2] + 0.5f) / 2.0f);
        d[13] = (float)cls_map[(size_t)b * HW + (size_t)cy * W + cx];
    } else {
        d[13] = (float)L.cls[0][o + it];                      // clses = t_clses
    }
}

// one 1024-thread workgroup per image; ``cls_map`` as in exct_write_row
__global__ __launch_bounds__(NTM) void exct_select_kernel(
    const float *__restrict__ cand, const ExctLists L, const ExctRegr R, float *__restrict__ dets,
    int K, int H, int W, int num_dets, const int32_t *__restrict__ cls_map)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SelShared &sh = *reinterpret_cast<SelShared *>(smem);
    u64 *big = reinterpret_cast<u64 *>(smem + sizeof(SelShared));  // [EXCT_MAX_DETS]
    const int tid = threadIdx.x, b = blockIdx.x;
    const uint32_t n = (uint32_t)K * K * K * K;
    const float *cs = cand + (size_t)b * n;

    auto for_each = [&](auto &&f) {
        for (uint32_t j = tid; j < n; j += NTM) {
            const uint32_t kk = f2key(cs[j] + 0.0f);
            f(((u64)kk << 32) | (u64)(0xFFFFFFFFu - j), false);
        }
    };
    u64 prefix, mask;
    radix_select<NTM>(for_each, (uint32_t)num_dets, sh, prefix, mask);
    // collect the selected keys (exactly num_dets of them) and sort all 1024 slots descending
    __syncthreads();
    if (tid == 0) sh.cnt = 0;
    big[tid] = 0;  // pad keys sort last (NTM == EXCT_MAX_DETS)
    __syncthreads();
    for_each([&](u64 k, bool) {
        if ((k & mask) >= prefix) {
            const uint32_t pos = atomicAdd(&sh.cnt, 1u);
            if (pos < (uint32_t)EXCT_MAX_DETS) big[pos] = k;
        }
    });
    __syncthreads();
    for (int k = 2; k <= EXCT_MAX_DETS; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int partner = tid ^ j;
            if (partner > tid) {
                const u64 x = big[tid], y = big[partner];
                const bool desc = (tid & k) == 0;
                if (desc ? (x < y) : (x > y)) {
                    big[tid] = y;
                    big[partner] = x;
                }
            }
            __syncthreads();
        }
    }
    if (tid >= num_dets) return;
    exct_write_row(big[tid], L, R, dets, b, tid, K, H, W, num_dets, cls_map);
}

// ---- the streaming form of stages B and C (cn_exct_decode_stream_f32): no K^4 array.  The radix select of
// cn_select.h spread over the chip, one launch per step, the candidates scored again wherever they are read:
//   count(p)  grid (K*K, B): workgroup (t, l) scores its K*K candidates, bins digit p of the keys that match
//             the prefix found so far in LDS and adds its non-empty bins to the image's histogram of pass p
//   pick(p)   grid B: pick_bin() on that histogram -> prefix, mask and need of the image's state; `done` once
//             everything at or above the boundary bin fits the image's key list
//   collect   grid (K*K, B): appends every key with (key & mask) >= prefix to the list through a cursor
//   rows      grid B: sorts the list in LDS (full 64-bit keys, so the cursor's order does not matter), writes
//             the first num_dets rows
// count and pick of an image that is `done` return at once, so the launch sequence is the same for every input.
// No workgroup waits on another: the steps are ordered by the stream.  DESIGN.md 3.4a.
constexpr int EXCT_LIST = 2 * EXCT_MAX_DETS;   // key slots of an image's list (the rows kernel sorts all of them)
constexpr int EXCT_PASSES = 6;                 // digits of the 64-bit key (pass_shift)
static_assert(CN_EXCT_STREAM_MAX_K <= KMAX && (long)CN_EXCT_STREAM_MAX_K * CN_EXCT_STREAM_MAX_K * CN_EXCT_STREAM_MAX_K *
                      CN_EXCT_STREAM_MAX_K <= (1L << 28), "candidate indices are 32-bit, the lists come from cn_topk_f32");

struct ExctStreamState {    // per image; zeroed by the call (need == 0: not started)
    u64 prefix, mask;
    uint32_t need, done, count, pad_;
};

struct ExctStream {         // the select state in the workspace, each array per image
    uint32_t *hist;         // [B][EXCT_PASSES][HBINS], zeroed by the call
    ExctStreamState *state; // [B]
    u64 *list;              // [B][EXCT_LIST]
};

__device__ __forceinline__ u64 exct_key(float score, uint32_t idx)
{
    return ((u64)f2key(score + 0.0f) << 32) | (u64)(0xFFFFFFFFu - idx);
}

__global__ __launch_bounds__(NT) void exct_stream_count_kernel(
    const ExctLists L, const float *__restrict__ ct_heat, const ExctStream S, int K, int H, int W, int C,
    float scores_thresh, float center_thresh, int num_dets, int pass)
{
    __shared__ uint32_t hist[HBINS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const ExctStreamState st = S.state[b];
    if (st.done) return;                                    // (uniform: the whole workgroup leaves)
    for (int i = tid; i < HBINS; i += NT) hist[i] = 0;
    __syncthreads();
    const int shift = pass_shift(pass);
    const uint32_t dmask = pass_dmask(pass);
    const int it = blockIdx.x / K, il = blockIdx.x % K;
    const uint32_t first = blockIdx.x * (uint32_t)(K * K);   // index of candidate (t, l, 0, 0)
    // neighbouring candidates mostly share their leading digits: a thread adds a run of equal digits at once
    uint32_t cur = 0, run = 0;
    for (int j = tid; j < K * K; j += NT) {
        const u64 key = exct_key(exct_score(L, ct_heat, b, K, H, W, C, it, il, j / K, j % K, scores_thresh,
                                            center_thresh), first + j);
        if ((key & st.mask) != st.prefix) continue;
        const uint32_t d = (uint32_t)(key >> shift) & dmask;
        if (run && d != cur) {
            atomicAdd(&hist[cur], run);
            run = 0;
        }
        cur = d;
        ++run;
    }
    if (run) atomicAdd(&hist[cur], run);
    __syncthreads();
    uint32_t *gh = S.hist + ((size_t)b * EXCT_PASSES + pass) * HBINS;
    for (int i = tid; i < HBINS; i += NT)
        if (hist[i]) atomicAdd(&gh[i], hist[i]);            // integer sums: the order of arrival does not matter
}

__global__ __launch_bounds__(NT) void exct_stream_pick_kernel(const ExctStream S, int num_dets, int pass)
{
    __shared__ SelShared sh;
    const int tid = threadIdx.x, b = blockIdx.x;
    ExctStreamState &st = S.state[b];
    if (st.done) return;
    const uint32_t need = pass == 0 ? (uint32_t)num_dets : st.need;
    const uint32_t *gh = S.hist + ((size_t)b * EXCT_PASSES + pass) * HBINS;
    for (int i = tid; i < HBINS; i += NT) sh.hist[i] = gh[i];
    __syncthreads();
    pick_bin<NT>(sh, need);
    if (tid == 0) {
        st.prefix |= (u64)sh.digit << pass_shift(pass);
        st.mask |= (u64)pass_dmask(pass) << pass_shift(pass);
        st.need = sh.need;
        // keys above the boundary bin: num_dets - need; with the bin itself they must fit the list.  The last
        // pass always ends here: keys are distinct, so its boundary bin holds one key
        st.done = ((uint32_t)num_dets - sh.need) + sh.bincount <= (uint32_t)EXCT_LIST;
    }
}

__global__ __launch_bounds__(NT) void exct_stream_collect_kernel(
    const ExctLists L, const float *__restrict__ ct_heat, const ExctStream S, int K, int H, int W, int C,
    float scores_thresh, float center_thresh)
{
    const int tid = threadIdx.x, b = blockIdx.y;
    const ExctStreamState st = S.state[b];
    const int it = blockIdx.x / K, il = blockIdx.x % K;
    const uint32_t first = blockIdx.x * (uint32_t)(K * K);
    for (int j = tid; j < K * K; j += NT) {
        const u64 key = exct_key(exct_score(L, ct_heat, b, K, H, W, C, it, il, j / K, j % K, scores_thresh,
                                            center_thresh), first + j);
        if ((key & st.mask) >= st.prefix) {
            const uint32_t pos = atomicAdd(&S.state[b].count, 1u);
            if (pos < (uint32_t)EXCT_LIST) S.list[(size_t)b * EXCT_LIST + pos] = key;
        }
    }
}

// one 1024-thread workgroup per image, two list slots per thread
__global__ __launch_bounds__(NTM) void exct_stream_rows_kernel(
    const ExctStream S, const ExctLists L, const ExctRegr R, float *__restrict__ dets, int K, int H, int W,
    int num_dets, const int32_t *__restrict__ cls_map)
{
    __shared__ u64 big[EXCT_LIST];
    const int tid = threadIdx.x, b = blockIdx.x;
    const uint32_t n = min(S.state[b].count, (uint32_t)EXCT_LIST);
    for (int i = tid; i < EXCT_LIST; i += NTM)
        big[i] = (uint32_t)i < n ? S.list[(size_t)b * EXCT_LIST + i] : 0;   // pad keys sort last
    __syncthreads();
    for (int k = 2; k <= EXCT_LIST; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < EXCT_LIST; i += NTM) {
                const int partner = i ^ j;
                if (partner > i) {
                    const u64 x = big[i], y = big[partner];
                    const bool desc = (i & k) == 0;
                    if (desc ? (x < y) : (x > y)) {
                        big[i] = y;
                        big[partner] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid >= num_dets) return;
    exct_write_row(big[tid], L, R, dets, b, tid, K, H, W, num_dets, cls_map);
}

// agnex_ct_decode's `torch.max(ct_heat, dim=1)` (decode.py:164): per cell the largest value over the classes and
// the FIRST class that holds it
__global__ void channel_max_kernel(const float *__restrict__ heat, float *__restrict__ vmax,
                                   int32_t *__restrict__ imax, int C, int HW, size_t cells)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / HW, p = i - b * HW;
        const float *src = heat + b * (size_t)C * HW + p;
        float best = src[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = src[(size_t)c * HW];
            if (v > best) {
                best = v;
                arg = c;
            }
        }
        vmax[i] = best;
        imax[i] = arg;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Edge aggregation of exct_decode (models/decode.py:17-90, aggr_weight > 0): along a row (_h_aggregate)
// or a column (_v_aggregate) of every plane, from both ends, a running sum that continues while the
// values do not fall -- ret[i] = heat[i] + ret[i-1] * (heat[i] >= heat[i-1]) -- minus the value itself;
// out = (w * first + w * second) + heat in the reference's order of float32 operations.  One thread per
// line, two sequential passes (the recurrence is serial by definition; the maps are small).
// ---------------------------------------------------------------------------
namespace {
__global__ void exct_aggregate_kernel(const float *__restrict__ heat, float *__restrict__ out, int planes,
                                      int H, int W, int horizontal, float w)
{
    const int nline = horizontal ? H : W, len = horizontal ? W : H;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)planes * nline) return;
    const int plane = (int)(t / nline), line = (int)(t - (long)plane * nline);
    const size_t base = (size_t)plane * H * W + (horizontal ? (size_t)line * W : (size_t)line);
    const size_t step = horizontal ? 1 : (size_t)W;
    // first pass (from the start: _left / _top): out holds ret - heat
    float prev_h = heat[base], prev_r = prev_h;
    out[base] = add_rn(prev_r, -prev_h);
    for (int i = 1; i < len; ++i) {
        const float h = heat[base + i * step];
        const float r = add_rn(h, mul_rn(prev_r, (h >= prev_h) ? 1.0f : 0.0f));
        out[base + i * step] = add_rn(r, -h);
        prev_h = h;
        prev_r = r;
    }
    // second pass (from the end: _right / _bottom) and the combination
    prev_h = heat[base + (size_t)(len - 1) * step];
    prev_r = prev_h;
    {
        const size_t o = base + (size_t)(len - 1) * step;
        out[o] = add_rn(add_rn(mul_rn(w, out[o]), mul_rn(w, add_rn(prev_r, -prev_h))), prev_h);
    }
    for (int i = len - 2; i >= 0; --i) {
        const size_t o = base + i * step;
        const float h = heat[o];
        const float r = add_rn(h, mul_rn(prev_r, (h >= prev_h) ? 1.0f : 0.0f));
        out[o] = add_rn(add_rn(mul_rn(w, out[o]), mul_rn(w, add_rn(r, -h))), h);
        prev_h = h;
        prev_r = r;
    }
}
}  // namespace

extern "C" int cn_exct_aggregate_f32(const float *heat, float *out, int B, int C, int H, int W,
                                     int horizontal, float aggr_weight, void *stream)
{
    if (!heat || !out) return CN_ERR_NULL;
    if (heat == out) return CN_ERR_UNSUPPORTED;      // two passes read the input
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return CN_ERR_SHAPE;
    const long lines = (long)B * C * (horizontal ? H : W);
    hipLaunchKernelGGL(exct_aggregate_kernel, dim3((unsigned)((lines + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, heat, out, B * C, H, W, horizontal ? 1 : 0, aggr_weight);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

namespace {
// decode.py:297-305 for one edge map: heat * (max_pool2d(heat, 3, 1, 1) == heat), then values > 1 set
// to 1.  (Clamping BEFORE the peak test would turn every plateau of clamped cells into peaks.)
__global__ void exct_nms_clamp_kernel(const float *__restrict__ heat, float *__restrict__ out, int H, int W,
                                      size_t total)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const float v = heat[i];
        float m = v;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) m = fmaxf(m, heat[i + (long)dy * W + dx]);
            }
        out[i] = (m == v) ? fminf(v, 1.0f) : 0.0f;
    }
}
}  // namespace

extern "C" size_t cn_exct_decode_workspace_bytes(int B, int C, int H, int W, int K)
{
    const size_t base = cn_ctdet_decode_workspace_bytes(B, C, H, W, K);
    if (!base) return 0;
    const size_t lists = 4 * 3 * cn_align_up((size_t)B * K * 4, 256);
    const size_t cand = cn_align_up((size_t)B * K * K * K * K * sizeof(float), 256);
    const size_t map = cn_align_up((size_t)B * C * H * W * sizeof(float), 256);   // CN_EXCT_CLAMP_ONE: one peak-tested, clamped edge map
    return base + lists + cand + map;
}

// The streaming form's workspace: the top-K workspace, the twelve lists, the one clamped map and the select state --
// per image EXCT_PASSES histograms, the state words and EXCT_LIST keys (under 1 MiB); no K^4 array.
static size_t exct_stream_state_bytes(int B)
{
    return cn_align_up((size_t)B * EXCT_PASSES * HBINS * sizeof(uint32_t), 256) +
           cn_align_up((size_t)B * sizeof(ExctStreamState), 256) + cn_align_up((size_t)B * EXCT_LIST * sizeof(u64), 256);
}

extern "C" size_t cn_exct_decode_stream_workspace_bytes(int B, int C, int H, int W, int K)
{
    const size_t base = cn_ctdet_decode_workspace_bytes(B, C, H, W, K);
    if (!base || K > CN_EXCT_STREAM_MAX_K) return 0;
    const size_t lists = 4 * 3 * cn_align_up((size_t)B * K * 4, 256);
    const size_t map = cn_align_up((size_t)B * C * H * W * sizeof(float), 256);
    return base + lists + map + exct_stream_state_bytes(B);
}

// The argument checks of both forms, in the stored form's order; `streaming` only moves the K limit.
static int exct_check_args(const float *t_heat, const float *l_heat, const float *b_heat, const float *r_heat,
                           const float *ct_heat, int K, int num_dets, int flags, const float *dets,
                           const void *workspace, bool streaming)
{
    if (!t_heat || !l_heat || !b_heat || !r_heat || !ct_heat || !dets || !workspace) return CN_ERR_NULL;
    if (num_dets <= 0 || K <= 0) return CN_ERR_SHAPE;
    // stored: K^4 floats in memory; streaming: K^4 <= 2^28 candidate indices.  Both: the LDS sort
    if (K > (streaming ? CN_EXCT_STREAM_MAX_K : CN_EXCT_STORED_MAX_K) || num_dets > EXCT_MAX_DETS) return CN_ERR_UNSUPPORTED;
    if ((long)num_dets > (long)K * K * K * K) return CN_ERR_SHAPE;      // torch.topk: k out of range
    if (flags & ~CN_EXCT_CLAMP_ONE) return CN_ERR_UNSUPPORTED;  // the centre map is gathered, not scanned
    return CN_OK;
}

static int exct_decode_impl(const float *t_heat, const float *l_heat, const float *b_heat,
                            const float *r_heat, const float *ct_heat, const float *t_regr,
                            const float *l_regr, const float *b_regr, const float *r_regr,
                            int B, int C, int H, int W, int K, float scores_thresh,
                            float center_thresh, int num_dets, int flags,
                            float *dets, void *workspace, size_t workspace_bytes,
                            void *stream, const int32_t *cls_map, bool streaming)
{
    const int bad = exct_check_args(t_heat, l_heat, b_heat, r_heat, ct_heat, K, num_dets, flags, dets, workspace,
                                    streaming);
    if (bad != CN_OK) return bad;
    const bool clamp_one = (flags & CN_EXCT_CLAMP_ONE) != 0;
    const size_t base = cn_ctdet_decode_workspace_bytes(B, C, H, W, K);
    if (!base) return CN_ERR_UNSUPPORTED;
    if (workspace_bytes < (streaming ? cn_exct_decode_stream_workspace_bytes(B, C, H, W, K)
                                     : cn_exct_decode_workspace_bytes(B, C, H, W, K)))
        return CN_ERR_WORKSPACE;
    // behind the lists: the stored form's K^4 scores, then the clamped map; the streaming form has the map there
    const size_t cand_bytes = streaming ? 0 : cn_align_up((size_t)B * K * K * K * K * sizeof(float), 256);
    const bool all_regr = t_regr && l_regr && b_regr && r_regr;  // decode.py:372-373
    const size_t slot = cn_align_up((size_t)B * K * 4, 256);
    char *p = (char *)workspace + base;
    ExctLists L;
    const float *heats[4] = {t_heat, l_heat, b_heat, r_heat};
    for (int e = 0; e < 4; ++e) {
        float *s = (float *)p; p += slot;
        int32_t *i = (int32_t *)p; p += slot;
        int32_t *c = (int32_t *)p; p += slot;
        int rc;
        if (clamp_one) {
            // peak test on the raw map, survivors clamped to 1 (decode.py:297-305), then the plain _topk
            // over every cell of the result (zeros of the suppressed cells take part, as in the reference)
            const size_t cells = (size_t)B * C * H * W;
            float *tmp = (float *)((char *)workspace + base + 4 * 3 * slot + cand_bytes);
            hipLaunchKernelGGL(exct_nms_clamp_kernel, dim3((unsigned)((cells + 255) / 256 < 8192 ? (cells + 255) / 256 : 8192)),
                               dim3(256), 0, (hipStream_t)stream, heats[e], tmp, H, W, cells);
            CN_CHECK_LAUNCH();
            rc = cn_topk_f32(tmp, B, C, H, W, K, CN_DECODE_NO_PEAK_TEST, s, i, c, workspace, base, stream);
        } else {
            rc = cn_topk_f32(heats[e], B, C, H, W, K, 0, s, i, c, workspace, base, stream);
        }
        if (rc != CN_OK) return rc;
        L.score[e] = s; L.ind[e] = i; L.cls[e] = c;
    }
    hipStream_t st = (hipStream_t)stream;
    ExctRegr R;
    R.r[0] = all_regr ? t_regr : nullptr; R.r[1] = all_regr ? l_regr : nullptr;
    R.r[2] = all_regr ? b_regr : nullptr; R.r[3] = all_regr ? r_regr : nullptr;
    if (streaming) {
        char *q = p + cn_align_up((size_t)B * C * H * W * sizeof(float), 256);   // behind the clamped map
        ExctStream S;
        S.hist = (uint32_t *)q;
        q += cn_align_up((size_t)B * EXCT_PASSES * HBINS * sizeof(uint32_t), 256);
        S.state = (ExctStreamState *)q;
        q += cn_align_up((size_t)B * sizeof(ExctStreamState), 256);
        S.list = (u64 *)q;
        if (hipMemsetAsync(S.hist, 0, (size_t)((char *)S.list - (char *)S.hist), st) != hipSuccess) return CN_ERR_LAUNCH;
        const dim3 slabs((unsigned)(K * K), (unsigned)B);
        for (int pass = 0; pass < EXCT_PASSES; ++pass) {
            hipLaunchKernelGGL(exct_stream_count_kernel, slabs, dim3(NT), 0, st, L, ct_heat, S, K, H, W, C,
                               scores_thresh, center_thresh, num_dets, pass);
            CN_CHECK_LAUNCH();
            hipLaunchKernelGGL(exct_stream_pick_kernel, dim3(B), dim3(NT), 0, st, S, num_dets, pass);
            CN_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(exct_stream_collect_kernel, slabs, dim3(NT), 0, st, L, ct_heat, S, K, H, W, C,
                           scores_thresh, center_thresh);
        CN_CHECK_LAUNCH();
        hipLaunchKernelGGL(exct_stream_rows_kernel, dim3(B), dim3(NTM), 0, st, S, L, R, dets, K, H, W, num_dets,
                           cls_map);
        CN_CHECK_LAUNCH();
        return CN_OK;
    }
    float *cand = (float *)p;
    const size_t n = (size_t)K * K * K * K;
    dim3 grid((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096), B);
    hipLaunchKernelGGL(exct_score_kernel, grid, dim3(256), 0, st, L, ct_heat, cand, K, H, W, C,
                       scores_thresh, center_thresh);
    CN_CHECK_LAUNCH();
    const size_t lds = sizeof(SelShared) + EXCT_MAX_DETS * sizeof(u64);
    hipLaunchKernelGGL(exct_select_kernel, dim3(B), dim3(NTM), lds, st, cand, L, R, dets, K, H, W,
                       num_dets, cls_map);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_exct_decode_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                                  const float *r_heat, const float *ct_heat, const float *t_regr,
                                  const float *l_regr, const float *b_regr, const float *r_regr,
                                  int B, int C, int H, int W, int K, float scores_thresh,
                                  float center_thresh, int num_dets, int apply_sigmoid,
                                  float *dets, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    return exct_decode_impl(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr, B, C, H, W, K,
                            scores_thresh, center_thresh, num_dets, apply_sigmoid, dets, workspace,
                            workspace_bytes, stream, nullptr, false);
}

extern "C" int cn_exct_decode_stream_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                                         const float *r_heat, const float *ct_heat, const float *t_regr,
                                         const float *l_regr, const float *b_regr, const float *r_regr,
                                         int B, int C, int H, int W, int K, float scores_thresh,
                                         float center_thresh, int num_dets, int apply_sigmoid,
                                         float *dets, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    return exct_decode_impl(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr, B, C, H, W, K,
                            scores_thresh, center_thresh, num_dets, apply_sigmoid, dets, workspace,
                            workspace_bytes, stream, nullptr, true);
}

// agnex_ct_decode (models/decode.py:121-271): the class-agnostic form -- ONE top / left / bottom / right map per
// image, the centre map over C classes.  The grouping is exct_decode's over single-channel maps (every point is
// "class 0": the class rule never fires and subtracts an exact 0) against the per-cell maximum of the centre map;
// a detection's class is that map's arg-max at the box centre.  Workspace: the single-class exct workspace + the
// (B, H, W) maximum and arg-max planes.
extern "C" size_t cn_agnex_ct_decode_workspace_bytes(int B, int C, int H, int W, int K)
{
    const size_t base = cn_exct_decode_workspace_bytes(B, 1, H, W, K);
    if (!base || C <= 0) return 0;
    return base + 2 * cn_align_up((size_t)B * H * W * 4, 256);
}

extern "C" size_t cn_agnex_ct_decode_stream_workspace_bytes(int B, int C, int H, int W, int K)
{
    const size_t base = cn_exct_decode_stream_workspace_bytes(B, 1, H, W, K);
    if (!base || C <= 0) return 0;
    return base + 2 * cn_align_up((size_t)B * H * W * 4, 256);
}

static int agnex_ct_decode_impl(const float *t_heat, const float *l_heat, const float *b_heat,
                                const float *r_heat, const float *ct_heat, const float *t_regr,
                                const float *l_regr, const float *b_regr, const float *r_regr,
                                int B, int C, int H, int W, int K, float scores_thresh,
                                float center_thresh, int num_dets, int flags, float *dets,
                                void *workspace, size_t workspace_bytes, void *stream, bool streaming)
{
    if (!t_heat || !l_heat || !b_heat || !r_heat || !ct_heat || !dets || !workspace) return CN_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return CN_ERR_SHAPE;
    if (streaming) {    // every refusal before the first launch (the stored form keeps its order of checks)
        const int bad = exct_check_args(t_heat, l_heat, b_heat, r_heat, ct_heat, K, num_dets, flags, dets, workspace,
                                        true);
        if (bad != CN_OK) return bad;
    }
    const size_t base = streaming ? cn_exct_decode_stream_workspace_bytes(B, 1, H, W, K)
                                  : cn_exct_decode_workspace_bytes(B, 1, H, W, K);
    if (!base) return CN_ERR_UNSUPPORTED;
    if (workspace_bytes < base + 2 * cn_align_up((size_t)B * H * W * 4, 256)) return CN_ERR_WORKSPACE;
    const size_t cells = (size_t)B * H * W;
    float *vmax = (float *)((char *)workspace + base);
    int32_t *imax = (int32_t *)((char *)workspace + base + cn_align_up(cells * 4, 256));
    const unsigned grid = (unsigned)((cells + 255) / 256 < 8192 ? (cells + 255) / 256 : 8192);
    hipLaunchKernelGGL(channel_max_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ct_heat, vmax, imax, C,
                       H * W, cells);
    CN_CHECK_LAUNCH();
    return exct_decode_impl(t_heat, l_heat, b_heat, r_heat, vmax, t_regr, l_regr, b_regr, r_regr, B, 1, H, W, K,
                            scores_thresh, center_thresh, num_dets, flags, dets, workspace, base, stream, imax,
                            streaming);
}

extern "C" int cn_agnex_ct_decode_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                                      const float *r_heat, const float *ct_heat, const float *t_regr,
                                      const float *l_regr, const float *b_regr, const float *r_regr,
                                      int B, int C, int H, int W, int K, float scores_thresh,
                                      float center_thresh, int num_dets, int flags, float *dets,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    return agnex_ct_decode_impl(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr, B, C, H, W,
                                K, scores_thresh, center_thresh, num_dets, flags, dets, workspace, workspace_bytes,
                                stream, false);
}

extern "C" int cn_agnex_ct_decode_stream_f32(const float *t_heat, const float *l_heat, const float *b_heat,
                                             const float *r_heat, const float *ct_heat, const float *t_regr,
                                             const float *l_regr, const float *b_regr, const float *r_regr,
                                             int B, int C, int H, int W, int K, float scores_thresh,
                                             float center_thresh, int num_dets, int flags, float *dets,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    return agnex_ct_decode_impl(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr, B, C, H, W,
                                K, scores_thresh, center_thresh, num_dets, flags, dets, workspace, workspace_bytes,
                                stream, true);
}
