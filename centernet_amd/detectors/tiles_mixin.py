"""``run_tiles`` / ``run_tiles_stream``: frames much larger than the network input, cut into
overlapping input-sized tiles at native resolution and merged per frame on the device.  What is the same for
every task that tiles -- the argument checks, the pipe cache, the synchronous comparison path and the two public
loops -- lives here; a task adds ``_tiles_tail(pipe)`` (its ``DeviceTail`` of ``TilePipe``, or None) and
``_tiles_host_tail(dets, grid, B, max_per_frame, **options)`` (the host specification on the raw detections of
the tile batch).  ``CtdetDetector`` and ``MultiPoseDetector`` use it; ``BaseDetector`` does not have the entries.
The mixin keeps no state of its own (the pipes live in the detector's ``_pipes``, as ``run_frames``' do)."""
import collections
import ctypes

import numpy as np
import torch

from .. import native


class TilesMixin(object):
    def _tiles_args(self, overlap, margin, tile_batch, max_per_frame):
        """Argument check of ``run_tiles`` / ``run_tiles_stream`` (no device needed) -> the arguments with
        their defaults filled in: overlap (y, x), margin (y, x), tile_batch, max_per_frame."""
        opt = self.opt
        if not opt.fix_res:
            raise ValueError("run_tiles: not with --keep_res (the tiles ARE the fixed-resolution network input)")
        if len(self.scales) != 1 or float(self.scales[0]) != 1.0:
            raise ValueError("run_tiles: one test scale, 1, got --test_scales %s" % (list(self.scales),))
        if opt.flip_test:
            raise ValueError("run_tiles: not with --flip_test")
        if int(tile_batch) != tile_batch or tile_batch < 1:
            raise ValueError("run_tiles: tile_batch must be an integer >= 1, got %r" % (tile_batch,))
        if max_per_frame is None:
            max_per_frame = self.max_per_image
        if int(max_per_frame) != max_per_frame or max_per_frame < 1:
            raise ValueError("run_tiles: max_per_frame must be an integer >= 1, got %r" % (max_per_frame,))
        th, tw = int(opt.input_h), int(opt.input_w)
        if overlap is None:
            overlap = (th // 4, tw // 4)
        try:
            oy, ox = overlap
        except TypeError:
            oy = ox = overlap
        for o, t in ((oy, th), (ox, tw)):
            if int(o) != o or not 0 <= o <= t // 2:
                raise ValueError("run_tiles: overlap must be an integer in [0, tile // 2] = [0, %d], got %r"
                                 % (t // 2, o))
        if margin is None:
            margin = (oy / 4.0, ox / 4.0)
        try:
            my, mx = margin
        except TypeError:
            my = mx = margin
        if not (my >= 0 and mx >= 0):
            raise ValueError("run_tiles: margin must be >= 0, got %r" % (margin,))
        return (int(oy), int(ox)), (float(my), float(mx)), int(tile_batch), int(max_per_frame)

    def _pyramid_options(self, args, levels, size_gate, gate_slack):
        """The pyramid arguments of ctdet's ``run_tiles`` (no device needed) -> the pipe's ``options``: nothing
        without ``levels`` (today's path, today's pipe key), else the three with their defaults filled in."""
        if levels is None:
            return {}
        from ..tiles import check_levels, level_gates
        levels = check_levels(levels)
        if size_gate is None:      # (as tiles.pyramid_grid: one level has no boundary, also at overlap 0)
            size_gate = max(min(args[0]), 1) if len(levels) == 1 else min(args[0])
        level_gates(levels, size_gate, gate_slack)          # (the checks; ValueError)
        return dict(levels=levels, size_gate=float(size_gate), gate_slack=float(gate_slack))

    def _tiles_grid(self, H, W, overlap, margin, options):
        """``tile_grid`` of the frame, or with ``levels`` among the options its ``pyramid_grid`` (with maps);
        there ``T * K`` above the merge's row cap is refused, before any device work."""
        from ..tiles import check_pyramid_rows, pyramid_grid, tile_grid
        th, tw = int(self.opt.input_h), int(self.opt.input_w)
        if options.get('levels') is None:
            return tile_grid(H, W, th, tw, overlap, margin)
        grid = pyramid_grid(H, W, th, tw, overlap, margin, options['levels'], options.get('size_gate'),
                            options.get('gate_slack', 0.25), down_ratio=self.opt.down_ratio)
        check_pyramid_rows(grid.T, int(self.opt.K), native.TILES_MAX_ROWS)
        return grid

    def _tiles_frames(self, frames, pixel_format):
        if torch.is_tensor(frames):
            raise ValueError("run_tiles takes host frames (a list of uint8 arrays)")
        return self._frames_geometry(frames, pixel_format)

    def _tile_pipe_for(self, frames, depth, overlap, margin, tile_batch, max_per_frame, pixel_format, **options):
        """The cached ``TilePipe`` of this batch geometry and these arguments.  ``options``: what the task's tail
        and host tail take beyond ``max_per_frame`` (multi_pose: ``min_score``), part of the key."""
        from ..frame_pipe import TilePipe
        B, H, W = self._tiles_frames(frames, pixel_format)
        key = ("tiles", B, H, W, overlap, margin, tile_batch, max_per_frame, bool(self.opt.nms), int(self.opt.K),
               depth, pixel_format) + tuple(sorted(options.items()))
        pipes = self.__dict__.setdefault("_pipes", {})
        if key not in pipes:
            if options.get('levels') is not None:
                self._tiles_grid(H, W, overlap, margin, options)     # (its refusals, before the pipe is built)
            if len(pipes) >= 4:
                pipes.pop(next(iter(pipes))).pool.shutdown(wait=False)
            pipes[key] = TilePipe(self, B, H, W, overlap, margin, tile_batch, max_per_frame, depth, pixel_format,
                                  options)
        return pipes[key]

    def _run_tiles_sync(self, frames, overlap, margin, tile_batch, max_per_frame, **options):
        """One batch of BGR frames, synchronously: every tile through the single-image warp
        (``cn_warp_normalize_u8_f32`` with the tile's matrix on its frame: ``pre_process_device`` for a tile),
        the chunks of ``tile_batch`` tiles of ``TilePipe`` -- a short last chunk in a zeroed batch of the full
        size -- through ``_forward_checked``, host tail (``options``: the task's).  With ``levels`` among the
        options the tiles are ``tiles.pyramid_grid``'s and every tile goes through a single-tile
        ``cn_tile_box_normalize_u8_f32`` launch instead.  The comparison path of the tile pipe and its re-run
        path."""
        from ..tiles import tile_maps
        B, H, W = self._frames_geometry(frames)
        th, tw, dev = int(self.opt.input_h), int(self.opt.input_w), self.opt.device
        grid = self._tiles_grid(H, W, overlap, margin, options)
        pyramid = options.get('levels') is not None
        if pyramid:      # one cn_tile_box_desc per tile of a frame; the frame's offset is added per launch
            desc = np.zeros((grid.T,), native.TILE_BOX_DESC)
            desc['H'], desc['W'], desc['pitch'], desc['level'] = H, W, 3 * W, grid.level
            desc['y0'], desc['x0'] = [o[0] for o in grid.origins], [o[1] for o in grid.origins]
            desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
        else:
            dst_to_src = tile_maps(grid, self.opt.down_ratio)[1]
        uploaded = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(dev)
        mean = (ctypes.c_float * 3)(*[float(v) for v in self.mean.reshape(-1)])
        std = (ctypes.c_float * 3)(*[float(v) for v in self.std.reshape(-1)])
        N = B * grid.T
        C = min(int(tile_batch), N)
        dets = []
        for lo in range(0, N, C):
            n = min(C, N - lo)
            batch = torch.zeros((C, 3, th, tw), device=dev, dtype=torch.float32)
            for j in range(n):
                b, t = divmod(lo + j, grid.T)
                if pyramid:
                    native.check(native.lib().cn_tile_box_normalize_u8_f32(
                        native.ptr(uploaded[b]), ctypes.c_void_p(desc_dev.data_ptr() + t * desc.itemsize), 1, th, tw,
                        mean, std, native.ptr(batch[j:j + 1]), native.stream_ptr()), "cn_tile_box_normalize_u8_f32")
                    continue
                native.check(native.lib().cn_warp_normalize_u8_f32(
                    native.ptr(uploaded[b]), H, W, W * 3, (ctypes.c_double * 6)(*dst_to_src[t]), th, tw, mean, std,
                    0, native.ptr(batch[j:j + 1]), native.stream_ptr()), "cn_warp_normalize_u8_f32")
            dets.append(self._forward_checked(batch, False)[:n])
        return self._tiles_host_tail(np.concatenate(dets, axis=0), grid, B, max_per_frame, **options)

    def _tiles_run(self, frames, args, pixel_format, arrays=False, **options):
        """One batch through the depth-1 pipe of these (checked) arguments."""
        pipe = self._tile_pipe_for(frames, 1, *args, pixel_format, **options)
        pipe.submit(0, frames)
        return pipe.collect(0, frames, arrays)

    def _tiles_stream(self, batches, depth, args, pixel_format, arrays=False, **options):
        """The batches through one pipe of ``depth`` slots, results in order (a generator)."""
        pipe, pending, n = None, collections.deque(), 0
        for frames in batches:
            if pipe is None:
                pipe = self._tile_pipe_for(frames, depth, *args, pixel_format, **options)
            elif self._tiles_frames(frames, pixel_format) != (pipe.B, pipe.H, pipe.W):
                raise ValueError("run_tiles_stream needs batches of one size, frame geometry and pixel format "
                                 "(%d %s frames of shape %s)" % (pipe.B, pipe.pixel_format, pipe.frame_shape))
            if len(pending) == depth:
                j, fr = pending.popleft()
                yield pipe.collect(j, fr, arrays)
            pipe.submit(n, frames)
            pending.append((n, frames))
            n += 1
        while pending:
            j, fr = pending.popleft()
            yield pipe.collect(j, fr, arrays)

    def run_tiles(self, frames, overlap=None, margin=None, tile_batch=32, max_per_frame=None, pixel_format='bgr'):
        """A list of (H, W, 3) uint8 BGR frames of one size, much larger than the network input -> per frame
        the task's results in frame pixels.  Every frame is cut into overlapping (input_h, input_w)
        tiles at native resolution (``tiles.tile_grid``: ``overlap`` pixels shared by neighbours, one integer or
        (y, x), by default a quarter of the tile; the last tile flush with the frame's edge; a frame smaller
        than a tile is padded with zeros), the tiles of all frames run as batches of ``tile_batch`` through ONE
        plan whatever the frame size, every tile contributes its own K candidates, and the boxes are merged
        on the device (ctdet: ``cn_ctdet_tiles_merge_f32``): a tile keeps the detections whose centre lies in its
        core (the cores meet in the middle of the overlaps; ``margin`` pixels past it on both sides, by default
        a quarter of the overlap), Gaussian soft-NMS per class removes what the margins let through twice, and
        the ``max_per_frame`` (default ``max_per_image``) best rows are kept, ties included.  Fixed-resolution
        mode, test scale 1, no flip-test: anything else, a bad ``overlap`` / ``margin`` / ``tile_batch`` and
        frames of mixed sizes raise ``ValueError``.  ``pixel_format='nv12'``: as ``run_frames``, host frames
        only.  With one tile per frame the result is ``run_frames``', bit for bit."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        return self._tiles_run(frames, args, pixel_format)

    def run_tiles_stream(self, batches, depth=3, overlap=None, margin=None, tile_batch=32, max_per_frame=None,
                         pixel_format='bgr'):
        """``run_tiles`` over an iterable of batches (lists of frames, all batches of one length and frame
        size), pipelined as ``run_frames_stream``.  Yields the per-frame results batch by batch, in order."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        yield from self._tiles_stream(batches, depth, args, pixel_format)
