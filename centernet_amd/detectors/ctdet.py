"""ctdet task (public behaviour of src/lib/detectors/ctdet.py:23-73): centre heat-map, box size
and sub-pixel offset decoded by the fused ``cn_ctdet_decode_f32`` kernels (``run_batch``: top-K on ``hm``,
then the ``wh`` / ``reg`` heads at the K cells only, ``cn_ctdet_heads_at_cells_f32``).  New surface:
``run_batch`` (device-resident batches), ``run_frames`` (lists of uint8 frames) and ``run_tiles`` (frames much
larger than the network input, tiled and merged on the device)."""
import collections
import ctypes
import time

import numpy as np
import torch

from .. import native
from ..decode import ctdet_decode, ctdet_decode_at_cells
from ..frame_pipe import DeviceTail
from ..post_process import ctdet_merge, ctdet_results_batch, ctdet_tiles_results
from ..utils import flip_average, flip_average_batch
from .base_detector import BaseDetector


def deferred_ctdet_heads(opt):
    """The heads ``run_batch`` leaves to the decode: ``wh`` (and ``reg``) are only gathered at the K
    decoded centres (decode.py:472-486), so their dense maps are not computed.  Not with flip-test
    (the averaged maps are needed), ``cat_spec_wh`` (2 x classes outputs) or K > 128; the network
    side (fp32 compute mode, fusable 3x3 + 1x1 heads) is the plan builder's decision."""
    if opt.flip_test or opt.cat_spec_wh or opt.K > 128 or 'wh' not in opt.heads:
        return ()
    if 'reg' in opt.heads:
        return ('wh', 'reg') if opt.reg_offset else ()
    return ('wh',)


class CtdetDetector(BaseDetector):
    def _deferred_heads(self):
        return deferred_ctdet_heads(self.opt)

    def _decode_batch(self, out):
        late = out.get('_deferred')
        if late is not None:
            return ctdet_decode_at_cells(out['hm'], late, K=self.opt.K, apply_sigmoid=True)
        return self._decode(out['hm'], out['wh'], out['reg'] if self.opt.reg_offset else None, True)

    def _decode(self, hm, wh, reg, logits):
        return ctdet_decode(hm, wh, reg=reg, cat_spec_wh=self.opt.cat_spec_wh, K=self.opt.K,
                            apply_sigmoid=logits)

    def process(self, images, return_time=False):
        """Network + decode of one pre-processed batch (ctdet.py:28-45).  Without flip-test the
        sigmoid of ctdet.py:31 is fused into the decode kernel (``hm`` stays logits); with it,
        the mirrored frame (image 1) is averaged in after the sigmoid, as in the reference."""
        with torch.no_grad():
            # consumed before the next run; check=True: f32s range words read here (the
            # reference synchronises at this point too), re-calibrate + re-run on a clamped value
            output = self.model(images, borrow=True, check=True)[-1]
            hm, wh = output['hm'], output['wh']
            reg = output['reg'] if self.opt.reg_offset else None
            logits = not self.opt.flip_test
            if self.opt.flip_test:
                hm = flip_average(hm, sigmoid=True)      # (sigmoid_() of both images in place, as ctdet.py:31)
                wh = flip_average(wh)
                reg = None if reg is None else reg[0:1]
            torch.cuda.synchronize()
            forward_time = time.time()
            dets = self._decode(hm, wh, reg, logits)
        return (output, dets, forward_time) if return_time else (output, dets)

    def post_process(self, dets, meta, scale=1):
        """(1, K, 6) in output-grid units -> {class: (n, 5) float32} in the coordinates of the
        unscaled frame (ctdet.py:47-56)."""
        host = dets.detach().cpu().numpy()
        host = host.reshape(1, -1, host.shape[2])
        # the batch tail with a batch of one and no cap: same rows, same order, same float32
        # rounding as ctdet_post_process + the per-class np.array / "/= scale" loop, without
        # the trip through Python lists
        return ctdet_results_batch(host, [meta], self.opt.num_classes, scale,
                                   max_per_image=host.shape[1])[0]

    def merge_outputs(self, detections):
        """Concatenate the test scales per class, soft-NMS when asked or when there are several,
        then keep the ``max_per_image`` best over all classes by score threshold -- ``>=``, so
        ties may exceed the cap, as in the reference (ctdet.py:58-73)."""
        return ctdet_merge(detections, self.num_classes, len(self.scales) > 1 or bool(self.opt.nms),
                           self.max_per_image)

    # ------------------------------------------------------------------ new surface
    _canvas_task = True

    def _run_scale(self, images, flip, rects=None):
        """One test scale of the frame pipeline: ``run_batch``, or with ``flip`` the (2B, 3, H, W)
        frame / mirror pairs -> network -> batched flip average (``hm`` after the sigmoid, ``reg`` of
        the un-mirrored frame, as ``process``) -> decode: (B, K, 6), asynchronous.  ``rects``: a canvas
        batch; with ``flip`` the mirror image's rectangle sits at the canvas' right edge, and the whole-width
        flip average brings it back onto the frame's."""
        if not flip:
            return self.run_batch(images, rects=rects)
        self._note_unchecked_forward()
        self._sync_deferral()        # flip-test defers nothing: plan_for(...) is then this dense plan
        with torch.no_grad():
            out = self.model(images, borrow=True, **({} if rects is None else {"rects": rects}))[-1]
            hm = flip_average_batch(out['hm'], sigmoid=True)
            wh = flip_average_batch(out['wh'])
            reg = flip_average_batch(out['reg'], first=True) if self.opt.reg_offset else None
            return self._decode(hm, wh, reg, False)

    def _device_tail(self, pipe):
        return CtdetTail(pipe) if CtdetTail.admits(pipe) else None

    def results_batch(self, dets, metas, scale):
        """Host tail of ``run_frames``: (B, K, 6) host array -> per-image ``{class: (n, 5)}``."""
        return ctdet_results_batch(dets, metas, self.opt.num_classes, scale, self.max_per_image)

    def _post_batch(self, dets, metas, scale):
        """``post_process`` of every image of a (B, K, 6) host array (no cut: merge_outputs makes it)."""
        return ctdet_results_batch(dets, metas, self.opt.num_classes, scale, max_per_image=dets.shape[1])


    # ------------------------------------------------------------------ run_tiles: large frames, tiled
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

    def _tiles_frames(self, frames, pixel_format):
        if torch.is_tensor(frames):
            raise ValueError("run_tiles takes host frames (a list of uint8 arrays)")
        return self._frames_geometry(frames, pixel_format)

    def _tile_pipe_for(self, frames, depth, overlap, margin, tile_batch, max_per_frame, pixel_format):
        from ..frame_pipe import TilePipe
        B, H, W = self._tiles_frames(frames, pixel_format)
        key = ("tiles", B, H, W, overlap, margin, tile_batch, max_per_frame, bool(self.opt.nms), int(self.opt.K),
               depth, pixel_format)
        pipes = self.__dict__.setdefault("_pipes", {})
        if key not in pipes:
            if len(pipes) >= 4:
                pipes.pop(next(iter(pipes))).pool.shutdown(wait=False)
            pipes[key] = TilePipe(self, B, H, W, overlap, margin, tile_batch, max_per_frame, depth, pixel_format)
        return pipes[key]

    def _tiles_tail(self, pipe):
        return TilesTail(pipe) if TilesTail.admits(pipe) else None

    def _tiles_host_tail(self, dets, grid, B, max_per_frame):
        """Host tail of ``run_tiles``: (B * T, K, 6) host raw detections of the tile batch -> per frame
        ``{class: (n, 5) float32}`` in frame pixels: ``post_process`` of every tile with the tile's meta, then
        ``post_process.ctdet_tiles_results`` (core filter, ``merge_outputs``' steps with tiles for scales)."""
        from ..tiles import tile_maps
        metas = tile_maps(grid, self.opt.down_ratio)[0]
        posts = self._post_batch(np.asarray(dets), metas * B, 1.0)
        return [ctdet_tiles_results(posts[b * grid.T:(b + 1) * grid.T], grid.cores, self.opt.num_classes,
                                    self.opt.nms, max_per_frame) for b in range(B)]

    def _run_tiles_sync(self, frames, overlap, margin, tile_batch, max_per_frame):
        """One batch of BGR frames, synchronously: every tile through the single-image warp
        (``cn_warp_normalize_u8_f32`` with the tile's matrix on its frame: ``pre_process_device`` for a tile),
        the chunks of ``tile_batch`` tiles of ``TilePipe`` -- a short last chunk in a zeroed batch of the full
        size -- through ``_forward_checked``, host tail.  The comparison path of the tile pipe and its re-run
        path."""
        from ..tiles import tile_grid, tile_maps
        B, H, W = self._frames_geometry(frames)
        th, tw, dev = int(self.opt.input_h), int(self.opt.input_w), self.opt.device
        grid = tile_grid(H, W, th, tw, overlap, margin)
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
                native.check(native.lib().cn_warp_normalize_u8_f32(
                    native.ptr(uploaded[b]), H, W, W * 3, (ctypes.c_double * 6)(*dst_to_src[t]), th, tw, mean, std,
                    0, native.ptr(batch[j:j + 1]), native.stream_ptr()), "cn_warp_normalize_u8_f32")
            dets.append(self._forward_checked(batch, False)[:n])
        return self._tiles_host_tail(np.concatenate(dets, axis=0), grid, B, max_per_frame)

    def run_tiles(self, frames, overlap=None, margin=None, tile_batch=32, max_per_frame=None, pixel_format='bgr'):
        """A list of (H, W, 3) uint8 BGR frames of one size, much larger than the network input -> per frame
        ``{class: (n, 5) float32}`` in frame pixels.  Every frame is cut into overlapping (input_h, input_w)
        tiles at native resolution (``tiles.tile_grid``: ``overlap`` pixels shared by neighbours, one integer or
        (y, x), by default a quarter of the tile; the last tile flush with the frame's edge; a frame smaller
        than a tile is padded with zeros), the tiles of all frames run as batches of ``tile_batch`` through ONE
        plan whatever the frame size, every tile contributes its own K candidates, and the boxes are merged
        on the device (``cn_ctdet_tiles_merge_f32``): a tile keeps the detections whose centre lies in its
        core (the cores meet in the middle of the overlaps; ``margin`` pixels past it on both sides, by default
        a quarter of the overlap), Gaussian soft-NMS per class removes what the margins let through twice, and
        the ``max_per_frame`` (default ``max_per_image``) best rows are kept, ties included.  Fixed-resolution
        mode, test scale 1, no flip-test: anything else, a bad ``overlap`` / ``margin`` / ``tile_batch`` and
        frames of mixed sizes raise ``ValueError``.  ``pixel_format='nv12'``: as ``run_frames``, host frames
        only.  With one tile per frame the result is ``run_frames``', bit for bit."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        pipe = self._tile_pipe_for(frames, 1, *args, pixel_format)
        pipe.submit(0, frames)
        return pipe.collect(0, frames)

    def run_tiles_stream(self, batches, depth=3, overlap=None, margin=None, tile_batch=32, max_per_frame=None,
                         pixel_format='bgr'):
        """``run_tiles`` over an iterable of batches (lists of frames, all batches of one length and frame
        size), pipelined as ``run_frames_stream``.  Yields the per-frame results batch by batch, in order."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        pipe, pending, n = None, collections.deque(), 0
        for frames in batches:
            if pipe is None:
                pipe = self._tile_pipe_for(frames, depth, *args, pixel_format)
            elif self._tiles_frames(frames, pixel_format) != (pipe.B, pipe.H, pipe.W):
                raise ValueError("run_tiles_stream needs batches of one size, frame geometry and pixel format "
                                 "(%d %s frames of shape %s)" % (pipe.B, pipe.pixel_format, pipe.frame_shape))
            if len(pending) == depth:
                j, fr = pending.popleft()
                yield pipe.collect(j, fr)
            pipe.submit(n, frames)
            pending.append((n, frames))
            n += 1
        while pending:
            j, fr = pending.popleft()
            yield pipe.collect(j, fr)


class TilesTail(DeviceTail):
    """The tail of ``TilePipe``: per chunk cn_ctdet_post_process_f32 with one inverse map per tile into the
    chunk's slice of the (B * T, K, 5) tile rows; behind the last chunk cn_ctdet_tiles_merge_f32: final rows in
    frame pixels grouped by class, the class bounds, and one status word per frame."""

    @classmethod
    def admits(cls, pipe):
        """Not with more detections per tile, rows per frame or classes than the kernels take."""
        K, nc = pipe.det.opt.K, pipe.det.opt.num_classes
        return K <= 128 and nc <= native.MERGE_MAX_CLASSES and pipe.T * K <= native.TILES_MAX_ROWS

    def __init__(self, pipe):
        super(TilesTail, self).__init__(pipe)        # (``pipe.to_source_dev`` is set: no per-level maps)
        K, nc, B, T = self.det.opt.K, self.det.opt.num_classes, pipe.B, pipe.T
        self.output('rows', (B, T * K, 5), torch.float32)
        self.output('bounds', (B, nc + 1), torch.int32)
        self.output('status', (B,), torch.int32)
        self.tile_rows = torch.empty((B * T, K, 5), device=self.device, dtype=torch.float32)
        self.tile_bounds = torch.empty((B * T, nc + 1), device=self.device, dtype=torch.int32)
        self.ws_bytes = int(native.lib().cn_ctdet_tiles_merge_workspace_bytes(B, T, K, nc))
        self.ws = torch.empty((self.ws_bytes,), device=self.device, dtype=torch.uint8)

    def run(self, slot, level, dets):
        """Chunk ``level``: the raw detections of its tiles -> frame pixels, grouped by class, into its slice."""
        pipe, opt, lv = self.pipe, self.det.opt, self.pipe.levels[level]
        dets = dets.contiguous()
        native.check(native.lib().cn_ctdet_post_process_f32(
            native.ptr(dets), lv.n, opt.K, opt.num_classes, native.ptr(pipe.to_source_dev[lv.lo:]), 1, 1.0,
            native.ptr(self.tile_rows[lv.lo:]), native.ptr(self.tile_bounds[lv.lo:]), native.stream_ptr()),
            "cn_ctdet_post_process_f32")

    def finish(self, slot):
        pipe, opt = self.pipe, self.det.opt
        native.check(native.lib().cn_ctdet_tiles_merge_f32(
            native.ptr(self.tile_rows), native.ptr(self.tile_bounds), pipe.B, pipe.T, opt.K, opt.num_classes,
            native.ptr(pipe.cores_dev), int(bool(opt.nms)), pipe.max_per_frame, native.ptr(self.out['rows']),
            native.ptr(self.out['bounds']), native.ptr(self.out['status']), native.ptr(self.ws), self.ws_bytes,
            native.stream_ptr()), "cn_ctdet_tiles_merge_f32")
        super(TilesTail, self).finish(slot)

    def results(self, slot, n):
        """Per frame ``{class: (n, 5) float32}``, or None when a frame's status is set: a class with more
        survivors than one soft-NMS holds, the batch goes back to the host tail."""
        if self.host('status', slot).numpy().any():
            return None
        return self.class_slices(self.host('rows', slot).numpy().copy(), self.host('bounds', slot).numpy().tolist(),
                                 n, self.det.opt.num_classes)


class CtdetTail(DeviceTail):
    """cn_ctdet_post_process_f32 per test scale and, when the pipe merges, cn_ctdet_merge_f32
    (``merge_outputs`` on the device): final rows in source pixels grouped by class, and the class bounds."""

    @classmethod
    def admits(cls, pipe):
        """Not with more detections than the kernels take or than max_per_image keeps."""
        det, K, S = pipe.det, pipe.det.opt.K, len(pipe.scales)
        if K > 128 or K > det.max_per_image:
            return False
        return not (pipe.merge and (S * K > native.MERGE_MAX_ROWS or det.opt.num_classes > native.MERGE_MAX_CLASSES))

    def __init__(self, pipe):
        super(CtdetTail, self).__init__(pipe)
        K, nc, B, S = self.det.opt.K, self.det.opt.num_classes, pipe.B, len(pipe.scales)
        rows = self.output('rows', (B, S * K if pipe.merge else K, 5), torch.float32)
        bounds = self.output('bounds', (B, nc + 1), torch.int32)
        # one slice per test scale; a pipe without a merge has one scale, and its slice is the result
        self.scale_rows, self.scale_bounds = rows[None], bounds[None]
        if pipe.merge:
            self.scale_rows = torch.empty((S, B, K, 5), device=self.device, dtype=torch.float32)
            self.scale_bounds = torch.empty((S, B, nc + 1), device=self.device, dtype=torch.int32)

    def run(self, slot, level, dets):
        """Raw detections -> source pixels / scale, grouped by class, into slice ``level``."""
        pipe, opt = self.pipe, self.det.opt
        dets = dets.contiguous()
        native.check(native.lib().cn_ctdet_post_process_f32(
            native.ptr(dets), pipe.B, opt.K, opt.num_classes, *self.source_map(slot, level),
            float(pipe.levels[level].scale), native.ptr(self.scale_rows[level]), native.ptr(self.scale_bounds[level]),
            native.stream_ptr()), "cn_ctdet_post_process_f32")

    def finish(self, slot):
        pipe, det = self.pipe, self.det
        if pipe.merge:
            native.check(native.lib().cn_ctdet_merge_f32(
                native.ptr(self.scale_rows), native.ptr(self.scale_bounds), len(pipe.scales), pipe.B, det.opt.K,
                det.opt.num_classes, int(bool(det.opt.nms)), det.max_per_image, native.ptr(self.out['rows']),
                native.ptr(self.out['bounds']), native.stream_ptr()), "cn_ctdet_merge_f32")
        super(CtdetTail, self).finish(slot)

    def results(self, slot, n):
        """Per image ``{class: (n, 5) float32}``: what is left is 80 slices per image."""
        return self.class_slices(self.host('rows', slot).numpy().copy(), self.host('bounds', slot).numpy().tolist(),
                                 n, self.det.opt.num_classes)
