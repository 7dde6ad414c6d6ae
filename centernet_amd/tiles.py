"""Tile geometry of ``run_tiles`` (no device needed): a frame larger than the network input is cut into
overlapping network-sized tiles at native resolution; every tile keeps the detections whose centre lies in its
CORE, and the cores (without margin) partition the plane, so an object in an overlap is reported once."""
import types

import numpy as np


def _pair(v):
    """``v`` or (v_y, v_x) -> (v_y, v_x)"""
    try:
        y, x = v
    except TypeError:
        y = x = v
    return y, x


def axis_origins(L, t, o):
    """Origins of the tiles of length ``t`` along an axis of length ``L`` at overlap ``o``: one tile at 0 when
    the axis fits it, else ``ceil((L - t) / (t - o)) + 1`` tiles ``min(i * (t - o), L - t)`` -- the last one
    flush with the edge."""
    L, t = int(L), int(t)
    if L <= 0 or t <= 0:
        raise ValueError("tile_grid needs positive sizes, got an axis of %d and a tile of %d" % (L, t))
    if o != int(o) or not 0 <= int(o) <= t // 2:
        raise ValueError("overlap must be an integer in [0, tile // 2] = [0, %d], got %r" % (t // 2, o))
    o = int(o)
    if L <= t:
        return [0]
    step = t - o
    n = -(-(L - t) // step) + 1
    return [min(i * step, L - t) for i in range(n)]


def axis_cores(origins, t, m):
    """(n, 2) float32 [lo, hi) of the tiles' cores along one axis, margin applied: the boundary between tiles
    i - 1 and i is the middle of their overlap, ``(x_i + x_{i-1} + t) / 2``; tile i keeps ``b_i - m <= u <
    b_{i+1} + m`` in float32; the outer boundaries are -inf and +inf."""
    m = np.float32(m)
    if not m >= 0:
        raise ValueError("margin must be >= 0, got %r" % (m,))
    n = len(origins)
    b = np.empty((n + 1,), np.float32)
    b[0], b[n] = -np.inf, np.inf
    for i in range(1, n):
        b[i] = np.float32((origins[i] + origins[i - 1] + t) / 2.0)
    out = np.empty((n, 2), np.float32)
    out[:, 0] = b[:-1] - m
    out[:, 1] = b[1:] + m
    return out


def tile_grid(H, W, th, tw, overlap, margin=None):
    """The tiles of an (H, W) frame at tile size (th, tw).  ``overlap``: pixels two neighbours share, one
    integer or (y, x), each in [0, tile // 2]; ``margin``: how far a core reaches past the middle of the
    overlap, one number or (y, x), >= 0, by default a quarter of the overlap.  ``ValueError`` otherwise.
    -> ``ny, nx, T``; ``ys, xs`` the origins per axis; ``origins`` [(y0, x0)] row-major, tile ``iy * nx + ix``;
    ``cores`` (T, 4) float32 [x_lo, y_lo, x_hi, y_hi], what cn_ctdet_tiles_merge_f32 reads."""
    oy, ox = _pair(overlap)
    ys, xs = axis_origins(H, th, oy), axis_origins(W, tw, ox)
    my, mx = (oy / 4.0, ox / 4.0) if margin is None else _pair(margin)
    cy, cx = axis_cores(ys, th, my), axis_cores(xs, tw, mx)
    ny, nx = len(ys), len(xs)
    cores = np.empty((ny * nx, 4), np.float32)
    origins = []
    for iy in range(ny):
        for ix in range(nx):
            cores[iy * nx + ix] = (cx[ix, 0], cy[iy, 0], cx[ix, 1], cy[iy, 1])
            origins.append((ys[iy], xs[ix]))
    return types.SimpleNamespace(H=int(H), W=int(W), th=int(th), tw=int(tw), ny=ny, nx=nx, T=ny * nx, ys=ys, xs=xs,
                                 origins=origins, cores=cores)


def tile_meta(y0, x0, th, tw, down_ratio):
    """The reference's meta of the tile at (y0, x0): centre of the tile, extent ``tw`` -- with
    ``get_affine_transform(c, s, 0, [tw, th])`` the translation by (-x0, -y0) at scale 1."""
    return {'c': np.array([x0 + tw / 2., y0 + th / 2.], dtype=np.float32), 's': float(tw),
            'out_height': th // down_ratio, 'out_width': tw // down_ratio}


def tile_maps(grid, down_ratio):
    """Per tile of ``grid``: ([T] metas, (T, 6) float64 network input -> frame matrices (the warp's
    ``dst_to_src``), (T, 6) float64 output grid -> frame maps (the post-process kernel's ``to_source``)), from
    ``get_affine_transform`` / ``invert_affine`` as for any other image."""
    from .image import get_affine_transform, invert_affine
    metas = [tile_meta(y0, x0, grid.th, grid.tw, down_ratio) for y0, x0 in grid.origins]
    dst_to_src = np.empty((grid.T, 6), np.float64)
    to_source = np.empty((grid.T, 6), np.float64)
    for t, m in enumerate(metas):
        dst_to_src[t] = invert_affine(get_affine_transform(m['c'], m['s'], 0, [grid.tw, grid.th])).reshape(-1)
        to_source[t] = np.asarray(get_affine_transform(m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1),
                                  np.float64).reshape(-1)
    return metas, dst_to_src, to_source


def check_levels(levels):
    """``levels`` of a tile pyramid as a tuple of ints, or ``ValueError``."""
    try:
        lv = tuple(levels)
    except TypeError:
        lv = None
    if not lv or any(isinstance(l, bool) or not isinstance(l, (int, np.integer)) or not 0 <= l <= 3 for l in lv) \
            or any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError("levels must be a non-empty, strictly increasing tuple of integers in [0, 3], got %r"
                         % (levels,))
    return tuple(int(l) for l in lv)


def level_gates(levels, size_gate, gate_slack=0.25):
    """(len(levels), 2) float32 [lo, hi) of the object sizes each listed level answers for, in frame pixels.
    ``size_gate`` = g, in pixels of a tile: the largest object some tile of a level is sure to see whole.  For
    consecutive listed levels a < b the boundary is ``g * 2**a``; level a keeps sizes below ``boundary * (1 +
    gate_slack)``, level b from ``boundary * (1 - gate_slack)`` on -- the bands overlap, and the soft-NMS of the
    merge removes what both report.  The first level's lo is -inf, the last one's hi +inf.  Formed in float64,
    rounded once to float32."""
    levels = check_levels(levels)
    g, slack = float(size_gate), float(gate_slack)
    if not g > 0 or not np.isfinite(g):
        raise ValueError("size_gate must be > 0, got %r" % (size_gate,))
    if not 0 <= slack < 1:
        raise ValueError("gate_slack must lie in [0, 1), got %r" % (gate_slack,))
    out = np.empty((len(levels), 2), np.float64)
    out[0, 0], out[-1, 1] = -np.inf, np.inf
    for i, a in enumerate(levels[:-1]):
        beta = g * 2.0 ** a
        out[i, 1] = beta * (1.0 + slack)
        out[i + 1, 0] = beta * (1.0 - slack)
    return out.astype(np.float32)


def pyramid_grid(H, W, th, tw, overlap, margin=None, levels=(0,), size_gate=None, gate_slack=0.25,
                 down_ratio=None):
    """The tiles of a tile PYRAMID over an (H, W) frame: level l of ``levels`` (non-empty, strictly increasing,
    integers in [0, 3]) is the frame box-filtered by f = 2**l, an image of ceil(H / f) x ceil(W / f), tiled by
    ``tile_grid(Hl, Wl, th, tw, overlap, margin)`` -- overlap and margin in that level's pixels; a level image
    smaller than a tile is one tile padded with zeros.  Tile order: all tiles of the first listed level in
    ``tile_grid`` order, then the next level's.  Level pixel v -> frame pixel u (integer = pixel centre):
    ``u = v * f + (f - 1) / 2``.
    -> ``tile_grid``'s kind of namespace: ``H, W, th, tw, T``; ``levels``; per level ``grids`` (its
    ``tile_grid``), ``level_lo`` (its first tile) and ``level_T`` (its tile count); per tile ``level``, ``origins``
    [(y0, x0)] in LEVEL pixels, ``cores`` (T, 4) float32 in FRAME pixels (the level grid's float32 bounds mapped
    in float64, rounded once; +-inf stay), ``gates`` (T, 2) float32 [lo, hi) in frame pixels (``level_gates`` of
    ``size_gate``, by default min(overlap_y, overlap_x); the level's band repeated for its tiles).  With a
    ``down_ratio`` also ``metas`` and ``to_source`` (``pyramid_maps``).  ``ValueError`` for anything else.
    ``levels=(0,)`` is ``tile_grid`` / ``tile_maps`` bit for bit, with the gate (-inf, +inf)."""
    levels = check_levels(levels)
    oy, ox = _pair(overlap)
    if size_gate is None and len(levels) == 1:
        size_gate = max(min(oy, ox), 1)      # (one level has no boundary: also at overlap 0)
    band = level_gates(levels, min(oy, ox) if size_gate is None else size_gate, gate_slack)
    grids, level_lo, level_T, level, origins, cores, gates = [], [], [], [], [], [], []
    for i, l in enumerate(levels):
        f = 1 << l
        g = tile_grid(-(-int(H) // f), -(-int(W) // f), th, tw, overlap, margin)
        grids.append(g)
        level_lo.append(len(origins))
        level_T.append(g.T)
        level += [l] * g.T
        origins += g.origins
        cores.append(g.cores if f == 1 else
                     (g.cores.astype(np.float64) * f + (f - 1) / 2.0).astype(np.float32))
        gates.append(np.repeat(band[i:i + 1], g.T, axis=0))
    out = types.SimpleNamespace(H=int(H), W=int(W), th=int(th), tw=int(tw), T=len(origins), levels=levels,
                                grids=grids, level_lo=level_lo, level_T=level_T, level=level, origins=origins,
                                cores=np.ascontiguousarray(np.concatenate(cores, axis=0)),
                                gates=np.ascontiguousarray(np.concatenate(gates, axis=0)), bands=band)
    if down_ratio is not None:
        out.metas, out.to_source = pyramid_maps(out, down_ratio)
    return out


def pyramid_maps(grid, down_ratio):
    """Per tile of a ``pyramid_grid``: ([T] metas, (T, 6) float64 output grid -> FRAME maps).  The map is
    ``tile_maps``' output grid -> level image map of the tile composed in float64 with the level map: both rows
    times f, translation ``t * f + (f - 1) / 2``; a meta is the tile's ``tile_meta`` in level pixels plus that map
    as ``'to_source'`` (2, 3), which the host post-process then takes instead of deriving one."""
    metas, maps = [], []
    for l, g in zip(grid.levels, grid.grids):
        f = 1 << l
        ms, _, to_level = tile_maps(g, down_ratio)
        if f > 1:
            to_level = to_level * float(f)
            to_level[:, 2] += (f - 1) / 2.0
            to_level[:, 5] += (f - 1) / 2.0
        maps.append(to_level)
        metas += [dict(m, to_source=to_level[t].reshape(2, 3)) for t, m in enumerate(ms)]
    return metas, np.ascontiguousarray(np.concatenate(maps, axis=0))


def check_pyramid_rows(T, K, max_rows=65536):
    """``ValueError`` when the T tiles of a pyramid with K detections each are more rows per frame than the
    gated merge takes (``CN_TILES_MAX_ROWS``): fewer levels, larger tiles or a smaller K."""
    if int(T) * int(K) > int(max_rows):
        raise ValueError("run_tiles: %d tiles of K = %d detections are %d rows per frame, above the merge's %d"
                         % (T, K, int(T) * int(K), max_rows))


def in_gate(rows, gate):
    """The rows [x1, y1, x2, y2, ...] (float32) whose size lies in ``gate`` = [lo, hi): a boolean mask.  With
    w = x2 - x1 and h = y2 - y1 in float32 a NaN in either fails; otherwise s = max(w, h), lo <= s < hi."""
    rows = np.asarray(rows, np.float32).reshape(-1, 5) if np.size(rows) else np.zeros((0, 5), np.float32)
    lo, hi = (np.float32(v) for v in gate)
    with np.errstate(invalid='ignore'):
        w, h = rows[:, 2] - rows[:, 0], rows[:, 3] - rows[:, 1]
        ok = ~(np.isnan(w) | np.isnan(h))
        s = np.where(w > h, w, h)
        return ok & (s >= lo) & (s < hi)


def in_core(rows, core):
    """The rows [x1, y1, x2, y2, ...] (float32) whose centre lies in ``core`` = [x_lo, y_lo, x_hi, y_hi]:
    a boolean mask; centre and comparisons in float32, lower edges closed, upper edges open."""
    rows = np.asarray(rows, np.float32).reshape(-1, 5) if np.size(rows) else np.zeros((0, 5), np.float32)
    cx = (rows[:, 0] + rows[:, 2]) * np.float32(0.5)
    cy = (rows[:, 1] + rows[:, 3]) * np.float32(0.5)
    x_lo, y_lo, x_hi, y_hi = (np.float32(v) for v in core)
    with np.errstate(invalid='ignore'):
        return (cx >= x_lo) & (cx < x_hi) & (cy >= y_lo) & (cy < y_hi)
