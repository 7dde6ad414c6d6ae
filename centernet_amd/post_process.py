"""Host tail of the path (mirror of src/lib/utils/post_process.py:83-114, and :10-81 for the ddd
task): map detections from the output grid back to image coordinates and split per class."""
import numpy as np

from .ddd_utils import ddd2locrot
from .image import transform_preds


def _class_order(classes, num_classes):
    """One stable sort by class instead of ``num_classes`` boolean masks: (the order that groups integer
    ``classes`` ascending, rows of a class in their original order; the num_classes + 1 class bounds in it)."""
    order = np.argsort(classes, kind='stable')
    return order, np.searchsorted(classes[order], np.arange(num_classes + 1))


def _inverse_maps(metas):
    """The frames grouped by geometry: [(indices of the frames, their (2, 3) float64 output grid -> source
    map)], one entry per distinct (centre, extent, output grid) in order of first appearance -- every frame of a
    video shares one.  ``get_affine_transform`` reads centre and extent as float32, so their float32 bytes
    decide the map.  A meta that carries its map (``'to_source'``, (2, 3) float64: a tile of a pyramid level,
    ``tiles.pyramid_maps``) is grouped by that map's bytes and keeps it."""
    from .image import get_affine_transform
    groups = {}
    for i, m in enumerate(metas):
        if 'to_source' in m:
            key = np.asarray(m['to_source'], np.float64).tobytes()
        else:
            key = (np.asarray(m['c'], np.float32).tobytes(), np.asarray(m['s'], np.float32).tobytes(),
                   int(m['out_width']), int(m['out_height']))
        groups.setdefault(key, []).append(i)

    def inverse(m):
        if 'to_source' in m:
            return np.asarray(m['to_source'], np.float64).reshape(2, 3)
        return get_affine_transform(m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1)
    return [(idx, inverse(metas[idx[0]])) for idx in groups.values()]


def _split_by_class(rows, classes, num_classes):
    """{1-based class: rows of that class in their original order}."""
    order, edges = _class_order(classes, num_classes)
    rows = rows[order]
    return {j + 1: rows[edges[j]:edges[j + 1]].tolist() for j in range(num_classes)}


def ctdet_post_process(dets, c, s, h, w, num_classes):
    """(B, K, 6) detections in output-grid units -> per image ``{class: [[x1, y1, x2, y2,
    score], ...]}`` in source-frame pixels, classes 1-based (what utils/post_process.py:83-100
    returns).  Both box corners go through one inverse map; rows are grouped by class with a
    stable sort instead of ``num_classes`` boolean masks.  ``dets`` is not modified."""
    ret = []
    for i in range(dets.shape[0]):
        corners = transform_preds(dets[i, :, 0:4].reshape(-1, 2), c[i], s[i], (w, h))
        rows = np.concatenate([corners.reshape(-1, 4).astype(np.float32),
                               dets[i, :, 4:5].astype(np.float32)], axis=1)
        ret.append(_split_by_class(rows, dets[i, :, -1].astype(np.int64), num_classes))
    return ret


def multi_pose_post_process(dets, c, s, h, w):
    """(B, K, 40) pose detections -> per image ``{1: [[x1, y1, x2, y2, score, 17 x (x, y)],
    ...]}`` in source-frame pixels (utils/post_process.py:103-114): the 2 box corners and the 17
    joints of every detection are one (K * 19, 2) point set under one inverse map."""
    ret = []
    for i in range(dets.shape[0]):
        K = dets.shape[1]
        pts = np.concatenate([dets[i, :, 0:4].reshape(K, 2, 2), dets[i, :, 5:39].reshape(K, 17, 2)],
                             axis=1)
        moved = transform_preds(pts.reshape(-1, 2), c[i], s[i], (w, h)).reshape(K, 19, 2)
        rows = np.concatenate([moved[:, :2].reshape(K, 4), dets[i, :, 4:5],
                               moved[:, 2:].reshape(K, 34)], axis=1).astype(np.float32)
        ret.append({1: rows.tolist()})
    return ret


def get_alpha(rot):
    """(n, 8) orientation head [bin 1: 2 class logits, sin, cos | bin 2: the same] -> observation
    angle (utils/post_process.py:13-21): the bin whose second logit is larger wins; bin 1 is centred
    on -pi / 2, bin 2 on +pi / 2.  The blend is written with the reference's 0 / 1 products (a float64
    result, as there)."""
    first = rot[:, 1] > rot[:, 5]
    a1 = np.arctan2(rot[:, 2], rot[:, 3]) + (-0.5 * np.pi)
    a2 = np.arctan2(rot[:, 6], rot[:, 7]) + (0.5 * np.pi)
    return a1 * first + a2 * (1 - first)


def ddd_post_process_2d(dets, c, s, opt):
    """(B, K, 16 | 18) rows of ``ddd_decode`` [x, y, score, rot 8, depth, dim 3, (w, h), class] ->
    per image {1-based class: (n, 8 | 10) float32 [x, y, score, alpha, depth, h, w, l, (w, h)]} with
    the centre in source pixels (utils/post_process.py:24-51).  The reference sends the (w, h) pair
    through the same point map as the centre -- translation included; so does this.  Writes the
    moved centres into ``dets`` (callers pass a copy, as the reference's detector does)."""
    out = []
    has_wh = dets.shape[2] > 16
    grid = (opt.output_w, opt.output_h)
    for i in range(dets.shape[0]):
        dets[i, :, :2] = transform_preds(dets[i, :, 0:2], c[i], s[i], grid)
        cls = dets[i, :, -1]
        per_class = {}
        for j in range(opt.num_classes):
            rows = dets[i, cls == j]
            cols = [rows[:, :3].astype(np.float32),
                    get_alpha(rows[:, 3:11])[:, np.newaxis].astype(np.float32),
                    rows[:, 11:12].astype(np.float32), rows[:, 12:15].astype(np.float32)]
            if has_wh:
                cols.append(transform_preds(rows[:, 15:17], c[i], s[i], grid).astype(np.float32))
            per_class[j + 1] = np.concatenate(cols, axis=1)
        out.append(per_class)
    return out


def ddd_post_process_3d(dets, calibs):
    """The 2-D stage's rows -> per image {class: (n, 13) float32 [alpha, x1, y1, x2, y2, h, w, l,
    x, y, z, rotation_y, score]}, an EMPTY class being a (0,) array (utils/post_process.py:53-79).
    Every image is lifted with ``calibs[0]``, as in the reference (its detector is single-image)."""
    out = []
    for per_class in dets:
        lifted = {}
        for cls, rows in per_class.items():
            preds = []
            for r in rows:
                center, score, alpha, depth, dims, wh = r[:2], r[2], r[3], r[4], r[5:8], r[8:10]
                location, rotation_y = ddd2locrot(center, alpha, dims, depth, calibs[0])
                box = [center[0] - wh[0] / 2, center[1] - wh[1] / 2,
                       center[0] + wh[0] / 2, center[1] + wh[1] / 2]
                preds.append([alpha] + box + dims.tolist() + location.tolist() + [rotation_y, score])
            lifted[cls] = np.array(preds, dtype=np.float32)
        out.append(lifted)
    return out


def ddd_post_process(dets, c, s, calibs, opt):
    """utils/post_process.py:81-86."""
    return ddd_post_process_3d(ddd_post_process_2d(dets, c, s, opt), calibs)


def ctdet_results_batch(dets, metas, num_classes, scale=1, max_per_image=100):
    """Vectorised host tail for a batch, single scale, no NMS: for every image exactly what
    ``merge_outputs([post_process(dets[i], meta_i, scale)])`` returns (detectors/ctdet.py:47-73)
    -- same float64 affine, same float32 rounding, same per-class row order -- without the
    80-class Python loop per image.  Images that share their geometry (every frame of a video:
    same centre, extent and output grid) share ONE inverse map and go through it together; the
    class grouping of the whole batch is one stable sort."""
    from .image import apply_affine
    dets = np.asarray(dets)
    B, K, _ = dets.shape
    xy = np.empty((B, K, 4), np.float32)
    for idx, to_source in _inverse_maps(metas):
        sel = idx if len(idx) < B else slice(None)
        pts = dets[sel, :, 0:4].reshape(-1, 2)
        xy[sel] = apply_affine(pts, to_source).astype(np.float32).reshape(-1, K, 4)
    rows = np.concatenate([xy, dets[:, :, 4:5].astype(np.float32)], axis=2)
    rows[:, :, :4] /= scale
    cls = dets[:, :, 5].astype(np.int64)
    stray = bool(((cls < 0) | (cls >= num_classes)).any())
    if K > max_per_image or stray:
        # keep the max_per_image best of every image (ties at the threshold kept, as the
        # reference's np.partition test does): rare, handled image by image.  The same path
        # serves class ids outside [0, num_classes) (a head with more channels than
        # opt.num_classes): such rows match no `classes == j` of the reference
        # (post_process.py:93-99) and are dropped, never moved into another image's rows.
        out = []
        for i in range(B):
            keep = np.ones(K, bool)
            if K > max_per_image:
                kth = K - max_per_image
                thresh = np.partition(rows[i, :, 4], kth)[kth]
                keep = rows[i, :, 4] >= thresh
            order, bounds = _class_order(cls[i][keep], num_classes)
            r = rows[i][keep][order]
            out.append({j + 1: r[bounds[j]:bounds[j + 1]] for j in range(num_classes)})
        return out
    order = np.argsort(cls, axis=1, kind='stable')
    rows = np.take_along_axis(rows, order[:, :, None], axis=1)
    cls = np.take_along_axis(cls, order, axis=1)
    # class boundaries of every image at once: position of (image, class) in the flattened keys
    flat = (cls + np.arange(B, dtype=np.int64)[:, None] * num_classes).reshape(-1)
    bounds = np.searchsorted(flat, np.arange(B * num_classes + 1)).tolist()
    rows = rows.reshape(B * K, 5)
    out = []
    for i in range(B):
        b0 = i * num_classes
        out.append({j + 1: rows[bounds[b0 + j]:bounds[b0 + j + 1]] for j in range(num_classes)})
    return out


def ctdet_merge(detections, num_classes, nms, max_per_image):
    """``CtdetDetector.merge_outputs`` as a function (detectors/ctdet.py; reference ctdet.py:58-73):
    ``detections`` = [{class: (n, 5) float32}] of one image in merge order (test scales, or the tiles of
    ``run_tiles``), ``nms`` = the reference's ``len(self.scales) > 1 or self.opt.nms``.  Per class the
    concatenation, soft-NMS when ``nms`` (in place: the whole array is kept), then the ``max_per_image`` best
    over all classes by score threshold -- ``>=``, so ties may exceed the cap."""
    classes = range(1, num_classes + 1)
    if len(detections) == 1 and not nms:
        results = {c: detections[0][c] for c in classes}     # nothing to merge, nothing edited
    else:
        results = {c: np.concatenate([d[c] for d in detections], axis=0).astype(np.float32)
                   for c in classes}
    if nms:
        from .soft_nms import soft_nms
        for c in classes:
            soft_nms(results[c], Nt=0.5, method=2)
    scores = np.hstack([results[c][:, 4] for c in classes])
    if len(scores) > max_per_image:
        kth = len(scores) - max_per_image
        thresh = np.partition(scores, kth)[kth]
        for c in classes:
            results[c] = results[c][results[c][:, 4] >= thresh]
    return results


def ctdet_tiles_results(per_tile, cores, num_classes, nms, max_per_frame):
    """The tile merge of ``run_tiles`` for one frame -- the specification ``cn_ctdet_tiles_merge_f32`` restates
    on the device.  ``per_tile``: [T] ``post_process`` results {class: (n, 5) float32} in FRAME pixels, in tile
    order; ``cores`` (T, 4) float32 (``tiles.tile_grid``).  A row of tile t survives when its centre lies in
    the tile's core (``tiles.in_core``: float32, lower edges closed, upper edges open); the survivors go through
    ``ctdet_merge`` with the tiles in the place of test scales: soft-NMS when ``T > 1 or nms``, then the
    ``max_per_frame`` cut with ties kept."""
    from .tiles import in_core
    T = len(per_tile)
    kept = []
    for tile, core in zip(per_tile, cores):
        one = {}
        for c in range(1, num_classes + 1):
            rows = np.asarray(tile[c], np.float32).reshape(-1, 5)
            one[c] = rows[in_core(rows, core)]
        kept.append(one)
    return ctdet_merge(kept, num_classes, T > 1 or bool(nms), max_per_frame)


def ctdet_pyramid_results(per_tile, cores, gates, num_classes, nms, max_per_frame):
    """The merge of a tile pyramid for one frame -- the specification ``cn_ctdet_tiles_merge_gated_f32``
    restates on the device: ``ctdet_tiles_results`` with the size gate in the filter.  ``per_tile``, ``cores``:
    as there, all tiles of all levels in ``tiles.pyramid_grid`` order; ``gates`` (T, 2) float32 [lo, hi) in
    frame pixels.  A row of tile t survives when its centre lies in the tile's core AND its size lies in the
    tile's gate (``tiles.in_gate``: w = x2 - x1, h = y2 - y1 in float32, a NaN in either fails, else
    lo <= max(w, h) < hi); then ``ctdet_merge`` with ``T > 1 or nms``."""
    from .tiles import in_core, in_gate
    T = len(per_tile)
    kept = []
    for tile, core, gate in zip(per_tile, cores, gates):
        one = {}
        for c in range(1, num_classes + 1):
            rows = np.asarray(tile[c], np.float32).reshape(-1, 5)
            one[c] = rows[in_core(rows, core) & in_gate(rows, gate)]
        kept.append(one)
    return ctdet_merge(kept, num_classes, T > 1 or bool(nms), max_per_frame)


def multi_pose_tiles_results(per_tile, cores, nms, max_per_frame, min_score=None):
    """The tile merge of multi_pose ``run_tiles`` for one frame -- the specification
    ``cn_multi_pose_tiles_merge_f32`` restates on the device, the host tail and the hand-back route.
    ``per_tile``: [T] (n, 39) float32 rows [x1, y1, x2, y2, score, 17 x (x, y)] in FRAME pixels, in tile order
    (``MultiPoseDetector._post_batch`` with the tile's meta); ``cores`` (T, 4) float32 (``tiles.tile_grid``).
    (a) a row of tile t survives when its box centre lies in the tile's core (``tiles.in_core``: float32, lower
    edges closed, upper edges open) and, with a ``min_score``, ``score >= float32(min_score)`` -- a NaN score
    fails; ``None``: no score test; (b) the survivors of all tiles in tile order, each tile's in their order;
    (c) when ``T > 1 or nms``: ``soft_nms_39(rows, Nt=0.5, method=2)`` in place with the WHOLE array kept, what
    ``MultiPoseDetector.merge_outputs`` does with test scales; (d) when more than ``max_per_frame`` rows are
    left, the rows with score >= the ``max_per_frame``-th largest score: duplicates counted, ties kept, order
    kept (ctdet's cut).  -> ``{1: (n, 39) float32}``.
    Rows past the kept count of the soft-NMS are stale copies (the box and score they last held, the joints the
    exchanges left there) and can pass the cut: inherited from ``merge_outputs`` on purpose, it keeps one tile
    per frame equal to ``run_frames``."""
    from .tiles import in_core
    T = len(per_tile)
    kept = []
    for tile, core in zip(per_tile, cores):
        rows = np.asarray(tile, np.float32).reshape(-1, 39)
        keep = in_core(rows[:, :5], core)
        if min_score is not None:
            with np.errstate(invalid='ignore'):
                keep &= rows[:, 4] >= np.float32(min_score)
        kept.append(rows[keep])
    rows = np.ascontiguousarray(np.concatenate(kept, axis=0), np.float32) if T else np.zeros((0, 39), np.float32)
    if (T > 1 or nms) and len(rows) > 1:                # (soft-NMS does nothing to fewer than two rows)
        from .soft_nms import soft_nms_39
        soft_nms_39(rows, Nt=0.5, method=2)
    if len(rows) > max_per_frame:
        kth = len(rows) - max_per_frame
        thresh = np.partition(rows[:, 4], kth)[kth]
        rows = rows[rows[:, 4] >= thresh]
    return {1: rows}


def ddd_norm_table(mean, std):
    """(3, 256) float32: ``(level / 255 - mean[c]) / std[c]`` with the ddd class's float32 chain
    (detectors/ddd.py:45-46) for every uint8 level -- what ``DddDetector.pre_process`` indexes on the
    host and ``cn_warp_table_u8_f32_batch`` on the device."""
    levels = np.arange(256, dtype=np.float32).reshape(256, 1, 1) / 255.
    table = (levels - np.asarray(mean, np.float32).reshape(1, 1, 3)) / np.asarray(std, np.float32).reshape(1, 1, 3)
    return np.ascontiguousarray(table.reshape(256, 3).T)                     # float32 throughout


def ddd_lift_rows(dets, to_source, calibs):
    """(B, K, 18) raw rows of ``ddd_decode``, the (2, 3) inverse map(s) ((B, 2, 3): one per image) and the
    (B, 3, 4) float32 matrices -> (B, K, 13) float32 [alpha, x1, y1, x2, y2, h, w, l, x, y, z, rotation_y,
    score] in the raw row order: ``ddd_post_process_2d`` + ``ddd_post_process_3d`` row by row, as array
    arithmetic with the reference's types (float64 point map; float32 everything else)."""
    from .image import apply_affine
    dets = np.asarray(dets, np.float32)
    B, K, _ = dets.shape
    to_source = np.asarray(to_source, np.float64)
    centre, wh = np.empty((B, K, 2), np.float32), np.empty((B, K, 2), np.float32)
    if to_source.ndim == 2:
        centre[:] = apply_affine(dets[:, :, 0:2], to_source).astype(np.float32).reshape(B, K, 2)
        wh[:] = apply_affine(dets[:, :, 15:17], to_source).astype(np.float32).reshape(B, K, 2)
    else:
        for i in range(B):
            centre[i] = apply_affine(dets[i, :, 0:2], to_source[i]).astype(np.float32)
            wh[i] = apply_affine(dets[i, :, 15:17], to_source[i]).astype(np.float32)
    alpha = get_alpha(dets.reshape(B * K, 18)[:, 3:11]).astype(np.float32).reshape(B, K)
    depth, dims = dets[:, :, 11], dets[:, :, 12:15]
    P = np.asarray(calibs, np.float32).reshape(B, 1, 3, 4)
    # unproject_2d_to_3d + "location[1] += h / 2" (ddd_utils.py:68-78, :111)
    z = depth - P[:, :, 2, 3]
    x = (centre[:, :, 0] * depth - P[:, :, 0, 3] - P[:, :, 0, 2] * z) / P[:, :, 0, 0]
    y = (centre[:, :, 1] * depth - P[:, :, 1, 3] - P[:, :, 1, 2] * z) / P[:, :, 1, 1]
    y = y + dims[:, :, 0] / 2
    # alpha2rot_y (ddd_utils.py:80-92); np.pi is a weak scalar: float32 comparisons and sums
    ray = np.arctan2(np.ascontiguousarray(centre[:, :, 0] - P[:, :, 0, 2]),
                     np.ascontiguousarray(np.broadcast_to(P[:, :, 0, 0], (B, K))))
    rot_y = alpha + ray
    rot_y = np.where(rot_y > np.pi, rot_y - 2 * np.pi, rot_y)
    rot_y = np.where(rot_y < -np.pi, rot_y + 2 * np.pi, rot_y)
    half_w, half_h = wh[:, :, 0] / 2, wh[:, :, 1] / 2
    rows = np.stack([alpha, centre[:, :, 0] - half_w, centre[:, :, 1] - half_h, centre[:, :, 0] + half_w,
                     centre[:, :, 1] + half_h, dims[:, :, 0], dims[:, :, 1], dims[:, :, 2], x, y, z, rot_y,
                     dets[:, :, 2]], axis=2)
    assert rows.dtype == np.float32
    return rows


def ddd_results_batch(dets, metas, num_classes, peak_thresh):
    """Vectorised host tail of the ddd task for a batch: for every image exactly what
    ``DddDetector.merge_outputs([ddd_post_process(dets[i], c_i, s_i, [calib_i], opt)[0]])`` returns -- same
    bits, angles included (both are NumPy), same shapes: ``{class: (n, 13) float32}``, a class without rows a
    ``(0,)`` array, a class whose rows were all cut ``(0, 13)``.  ``metas[i]``: 'c', 's', 'out_width',
    'out_height' and image i's own 'calib' (the reference lifts a batch with ``calibs[0]``; its detector is
    single-image).  Rows whose class is no integer in [0, num_classes) match no ``cls == j`` and are dropped."""
    dets = np.asarray(dets, np.float32)
    if dets.ndim != 3 or dets.shape[2] != 18:
        raise ValueError("ddd_results_batch needs (B, K, 18) rows: the 3-D stage reads the (w, h) columns "
                         "(--not_reg_bbox rows have none; the reference cannot lift them either)")
    B, K, _ = dets.shape
    maps = _inverse_maps(metas)
    to_source = np.empty((B, 2, 3), np.float64)
    for idx, t in maps:
        to_source[idx] = t
    calibs = np.stack([np.asarray(m['calib'], np.float32).reshape(3, 4) for m in metas])
    rows = ddd_lift_rows(dets, to_source[0] if len(maps) == 1 else to_source, calibs)
    cls = dets[:, :, 17]
    out = []
    for i in range(B):
        per_class = {}
        for j in range(num_classes):
            r = rows[i][cls[i] == j]
            if len(r) == 0:
                r = np.array([], dtype=np.float32)               # np.array([]) of the 3-D stage: shape (0,)
            else:
                r = r[r[:, -1] > peak_thresh]
            per_class[j + 1] = r
        out.append(per_class)
    return out


def exdet_post_batch(dets, metas, scale=1):
    """``ExdetDetector.post_process`` of every frame of a host batch: (n, R, 14) raw rows -- R = the frame's
    decode rows and, with flip-test, its mirror image's behind them -> (n, R, 14) float32, a copy: the
    second half of every frame's rows un-mirrored (``x1' = out_w - x2``, ``x2' = out_w - x1`` in float32),
    both box corners through the float64 inverse map and rounded once to float32, then ``/ scale`` in
    float32.  Frames that share their geometry go through one inverse map together."""
    from .image import apply_affine
    rows = np.array(dets, dtype=np.float32)
    n, R, _ = rows.shape
    half = R // 2
    for idx, to_source in _inverse_maps(metas):
        sel = idx if len(idx) < n else slice(None)
        out_w = metas[idx[0]]['out_width']
        left, right = rows[sel, half:, 0].copy(), rows[sel, half:, 2].copy()
        rows[sel, half:, 0], rows[sel, half:, 2] = out_w - right, out_w - left
        pts = rows[sel, :, 0:4].reshape(-1, 2)
        rows[sel, :, 0:4] = apply_affine(pts, to_source).astype(np.float32).reshape(-1, R, 4)
    rows[:, :, 0:4] /= scale
    return rows


def exdet_merge_rows(rows, num_classes, max_per_image=100):
    """``ExdetDetector.merge_outputs`` of one frame, (N, 14) post-processed rows of all its test scales in
    scale order -> ``{class: (n, 5) float32}``: one stable sort instead of ``num_classes`` boolean masks,
    soft-NMS only where a class has two rows or more (it does nothing to fewer), the same bits."""
    from .soft_nms import soft_nms
    score, cls = rows[:, 4], rows[:, 13]
    with np.errstate(invalid='ignore'):
        keep = (score > 0) & (cls >= 0) & (cls < num_classes) & (cls == np.floor(cls))    # `classes == j`
    kept = rows[keep]
    order, edges = _class_order(kept[:, 13].astype(np.int64), num_classes)
    boxes = np.ascontiguousarray(kept[order][:, 0:5])
    edges = edges.tolist()
    for j in range(num_classes):
        if edges[j + 1] - edges[j] > 1:
            soft_nms(boxes[edges[j]:edges[j + 1]], Nt=0.5, method=2)       # in place, on the class's slice
    results = {j + 1: boxes[edges[j]:edges[j + 1]] for j in range(num_classes)}
    if len(boxes) > max_per_image:
        kth = len(boxes) - max_per_image
        thresh = np.partition(boxes[:, 4], kth)[kth]
        results = {j: r[r[:, 4] >= thresh] for j, r in results.items()}
    return results


def exdet_results_batch(per_scale, num_classes, max_per_image=100):
    """Vectorised host tail of the exdet task for a batch.  ``per_scale``: [(raw rows (n, R, 14), the frames'
    metas, scale)] in test-scale order -> for every frame exactly what ``merge_outputs([post_process(...)
    per scale])`` returns (detectors/exdet.py:51-81), bit for bit.  Post-process AND merge: this task merges
    always (soft-NMS of every class and the ``max_per_image`` cut, one scale or several)."""
    posts = [exdet_post_batch(d, metas, scale) for d, metas, scale in per_scale]
    return [exdet_merge_rows(np.concatenate([p[i] for p in posts], axis=0), num_classes, max_per_image)
            for i in range(posts[0].shape[0])]
