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


def in_core(rows, core):
    """The rows [x1, y1, x2, y2, ...] (float32) whose centre lies in ``core`` = [x_lo, y_lo, x_hi, y_hi]:
    a boolean mask; centre and comparisons in float32, lower edges closed, upper edges open."""
    rows = np.asarray(rows, np.float32).reshape(-1, 5) if np.size(rows) else np.zeros((0, 5), np.float32)
    cx = (rows[:, 0] + rows[:, 2]) * np.float32(0.5)
    cy = (rows[:, 1] + rows[:, 3]) * np.float32(0.5)
    x_lo, y_lo, x_hi, y_hi = (np.float32(v) for v in core)
    with np.errstate(invalid='ignore'):
        return (cx >= x_lo) & (cx < x_hi) & (cy >= y_lo) & (cy < y_hi)
