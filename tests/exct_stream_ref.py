"""Host reference for exct_decode / agnex_ct_decode at any K: ``oracle/cref.exct_decode`` restated in blocks.

``cref.exct_decode`` materialises (B, K^4) arrays and sorts them whole, which is 8 GB and more at K = 100.  This
helper (not a test) evaluates the same float32 statements in the same order on one slab of K^3 candidates at a
time -- all groupings of one top point -- and keeps a running top ``num_dets`` under the same key: score
descending, candidate index ascending.  Every candidate is scored; nothing is pruned.  ``nms``, ``topk`` and the
edge aggregates are ``cref``'s own."""
import numpy as np

from oracle import cref

f32 = np.float32


def _merge(best_s, best_i, s, i, num_dets):
    """The top ``num_dets`` of the running list and a slab under (score descending, index ascending)."""
    if len(best_s) >= num_dets:                       # only a slab member that reaches the current cut can enter
        keep = s >= best_s[-1]
        s, i = s[keep], i[keep]
    s, i = np.concatenate([best_s, s]), np.concatenate([best_i, i])
    order = np.lexsort((i, -s))[:num_dets]
    return s[order], i[order]


def agnex_ct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr=None, l_regr=None, b_regr=None, r_regr=None,
                    K=40, scores_thresh=0.1, center_thresh=0.1, num_dets=1000, aggr_weight=0.0):
    return exct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr, K=K,
                       scores_thresh=scores_thresh, center_thresh=center_thresh, num_dets=num_dets,
                       aggr_weight=aggr_weight, agnostic=True)


def exct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr=None, l_regr=None, b_regr=None, r_regr=None,
                K=40, scores_thresh=0.1, center_thresh=0.1, num_dets=1000, aggr_weight=0.0, agnostic=False):
    B, C, H, W = t_heat.shape
    if num_dets > K ** 4:
        raise RuntimeError("selected index k out of range")
    if aggr_weight > 0:
        t_heat, b_heat = cref.h_aggregate(t_heat, aggr_weight), cref.h_aggregate(b_heat, aggr_weight)
        l_heat, r_heat = cref.v_aggregate(l_heat, aggr_weight), cref.v_aggregate(r_heat, aggr_weight)
    tops = [cref.topk(np.minimum(cref.nms(h), f32(1.0)), K) for h in (t_heat, l_heat, b_heat, r_heat)]
    ct_all = np.ascontiguousarray(ct_heat, f32)
    if agnostic:
        ct_clses = np.argmax(ct_all, axis=1).reshape(B, -1)          # first maximum, as torch.max
        ct_flat = np.max(ct_all, axis=1).reshape(B, -1)
    else:
        ct_flat = ct_all.reshape(B, -1)
    th, cth = f32(scores_thresh), f32(center_thresh)
    regs = (t_regr, l_regr, b_regr, r_regr)
    all_regr = all(r is not None for r in regs)
    out = np.empty((B, num_dets, 14), f32)
    K3 = K ** 3
    for n in range(B):
        def ax(v, e):           # list e of image n along axis e - 1 of a (K, K, K) slab over (l, b, r)
            shape = [1, 1, 1]
            shape[e - 1] = K
            return v[n].reshape(shape)
        S = [tops[0][0][n]] + [ax(tops[e][0], e) for e in (1, 2, 3)]
        CL = [tops[0][2][n]] + [ax(tops[e][2], e) for e in (1, 2, 3)]
        Y = [tops[0][3][n]] + [ax(tops[e][3], e) for e in (1, 2, 3)]
        X = [tops[0][4][n]] + [ax(tops[e][4], e) for e in (1, 2, 3)]
        box_ct_xs = np.broadcast_to((((X[1] + X[3]) + f32(0.5)) / f32(2)).astype(np.int64), (K, K, K))
        best_s, best_i = np.empty(0, f32), np.empty(0, np.int64)
        for t in range(K):
            ts, tc, ty, tx = (a[t:t + 1].reshape(1, 1, 1) for a in (S[0], CL[0], Y[0], X[0]))
            box_ct_ys = (((ty + Y[2]) + f32(0.5)) / f32(2)).astype(np.int64)
            ct_inds = box_ct_ys * W + box_ct_xs
            if not agnostic:
                ct_inds = tc.astype(np.int64) * (H * W) + ct_inds
            ct_scores = ct_flat[n][ct_inds]
            scores = ((((ts + S[1]) + S[2]) + S[3]) + f32(2) * ct_scores) / f32(6)
            cls_inds = (tc != CL[1]) | (tc != CL[2]) | (tc != CL[3])
            top_inds = (ty > Y[1]) | (ty > Y[2]) | (ty > Y[3])
            left_inds = (X[1] > tx) | (X[1] > X[2]) | (X[1] > X[3])
            bottom_inds = (Y[2] < ty) | (Y[2] < Y[1]) | (Y[2] < Y[3])
            right_inds = (X[3] < tx) | (X[3] < X[1]) | (X[3] < X[2])
            sc_inds = (ts < th) | (S[1] < th) | (S[2] < th) | (S[3] < th) | (ct_scores < cth)
            scores = scores.astype(f32)
            rules = (sc_inds, top_inds, left_inds, bottom_inds, right_inds) if agnostic else \
                (sc_inds, cls_inds, top_inds, left_inds, bottom_inds, right_inds)
            for flag in rules:
                scores = scores - np.broadcast_to(flag, (K, K, K)).astype(f32)
            best_s, best_i = _merge(best_s, best_i, scores.reshape(-1),
                                    np.arange(t * K3, (t + 1) * K3, dtype=np.int64), num_dets)
        sel = [best_i // K3, (best_i // (K * K)) % K, (best_i // K) % K, best_i % K]
        XS, YS, GX, GY = [], [], [], []
        for e in range(4):
            x, y = tops[e][4][n], tops[e][3][n]
            if all_regr:
                g = cref.transpose_and_gather_feat(regs[e], tops[e][1])[n]
                xs, ys = x + g[:, 0], y + g[:, 1]
            else:
                xs, ys = x + f32(0.5), y + f32(0.5)
            XS.append(xs[sel[e]])
            YS.append(ys[sel[e]])
            GX.append(x[sel[e]])
            GY.append(y[sel[e]])
        cols = [XS[1], YS[0], XS[3], YS[2], best_s]
        for e in range(4):
            cols += [XS[e], YS[e]]
        if agnostic:
            cx = (((GX[1] + GX[3]) + f32(0.5)) / f32(2)).astype(np.int64)
            cy = (((GY[0] + GY[2]) + f32(0.5)) / f32(2)).astype(np.int64)
            cols.append(ct_clses[n][cy * W + cx].astype(f32))
        else:
            cols.append(tops[0][2][n][sel[0]].astype(f32))
        out[n] = np.stack(cols, axis=1).astype(f32)
    return out
