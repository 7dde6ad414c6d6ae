// cn_decode_emit.h -- one row of the large-K image-level top-K (cn_decode_large.hip): the key of a winner -> its
// outputs, the ctdet box (MODE_CTDET) or the _topk list entry (MODE_TOPK).  The float operations are those of
// emit_rows (cn_decode.hip) for these two modes, with the row and its key as arguments: the large form keeps its
// sorted keys in registers, not in SelShared::sel.  tests/test_gpu_decode_large.py holds the two to the same
// bits.  Include it behind cn_internal.h (EmitArgs, MODE_*) and cn_select.h (the keys, and the no-contraction
// pragma this code relies on).
#pragma once

namespace {

// key index = class * H*W + cell; `row` is the rank of key `k` in image `b` (0 = best)
template <int MODE>
__device__ __forceinline__ void emit_row(u64 k, int row, int b, int H, int W, int K, int C, const EmitArgs &ea)
{
    static_assert(MODE == MODE_CTDET || MODE == MODE_TOPK, "the image-level modes");
    const int HW = H * W;
    const float score = key2f((uint32_t)(k >> 32));
    const uint32_t fid = 0xFFFFFFFFu - (uint32_t)k;
    const int cls = (int)(fid / (uint32_t)HW);
    const int ind = (int)(fid - (uint32_t)cls * (uint32_t)HW);
    if (MODE == MODE_TOPK) {  // _topk (decode.py:103-119): scores, inds, clses only
        ea.out_scores[(size_t)b * K + row] = score;
        ea.inds_out[(size_t)b * K + row] = ind;
        ea.cls_out[(size_t)b * K + row] = cls;
        return;
    }
    const float *__restrict__ wh = ea.wh, *__restrict__ reg = ea.reg;
    const int yi = ind / W, xi = ind - yi * W;
    float xs = (float)xi, ys = (float)yi;
    if (reg) {  // decode.py:472-476
        xs = xs + reg[((size_t)b * 2 + 0) * HW + ind];
        ys = ys + reg[((size_t)b * 2 + 1) * HW + ind];
    } else {  // decode.py:477-479
        xs = xs + 0.5f;
        ys = ys + 0.5f;
    }
    const int whC = ea.cat_spec_wh ? 2 * C : 2;
    const int wc = ea.cat_spec_wh ? 2 * cls : 0;  // decode.py:481-486
    const float w = wh[((size_t)b * whC + wc + 0) * HW + ind];
    const float h = wh[((size_t)b * whC + wc + 1) * HW + ind];
    float *d = ea.dets + ((size_t)b * K + row) * 6;
    d[0] = xs - w / 2;  // decode.py:489-492
    d[1] = ys - h / 2;
    d[2] = xs + w / 2;
    d[3] = ys + h / 2;
    d[4] = score;
    d[5] = (float)cls;
    if (ea.inds_out) ea.inds_out[(size_t)b * K + row] = ind;
}

}  // namespace
