"""ctdet task (public behaviour of src/lib/detectors/ctdet.py:23-73): centre heat-map, box size
and sub-pixel offset decoded by the fused ``cn_ctdet_decode_f32`` kernels (``run_batch``: top-K on ``hm``,
then the ``wh`` / ``reg`` heads at the K cells only, ``cn_ctdet_heads_at_cells_f32``).  New surface:
``run_batch`` (device-resident batches), ``run_frames`` (lists of uint8 frames) and ``run_tiles`` (frames much
larger than the network input, tiled and merged on the device)."""
import time

import numpy as np
import torch

from .. import native
from ..decode import ctdet_decode, ctdet_decode_at_cells
from ..frame_pipe import DeviceTail
from ..post_process import ctdet_merge, ctdet_pyramid_results, ctdet_results_batch, ctdet_tiles_results
from ..utils import flip_average, flip_average_batch
from .base_detector import BaseDetector
from .tiles_mixin import TilesMixin


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


class CtdetDetector(TilesMixin, BaseDetector):
    def __init__(self, opt):
        # K <= 128: the one-launch top-K, the heads at the K cells, the device tails.  128 < K <= 1024: the large-K
        # top-K (csrc/cn_decode_large.hip) on the dense wh / reg maps, host tails.  More is nobody's path.
        if opt.K > native.DECODE_LARGE_MAX_K:
            raise ValueError("the ctdet task needs --K <= %d, got %d" % (native.DECODE_LARGE_MAX_K, opt.K))
        super(CtdetDetector, self).__init__(opt)

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
    # (the entries, their argument checks and the synchronous path: TilesMixin)
    def _tiles_tail(self, pipe):
        return TilesTail(pipe) if TilesTail.admits(pipe) else None

    def _tiles_host_tail(self, dets, grid, B, max_per_frame, levels=None, size_gate=None, gate_slack=0.25):
        """Host tail of ``run_tiles``: (B * T, K, 6) host raw detections of the tile batch -> per frame
        ``{class: (n, 5) float32}`` in frame pixels: ``post_process`` of every tile with the tile's meta, then
        ``post_process.ctdet_tiles_results`` (core filter, ``merge_outputs``' steps with tiles for scales).  With
        ``levels`` ``grid`` is the ``tiles.pyramid_grid`` of these options: its metas carry the output grid ->
        frame map of their level, and the merge is ``post_process.ctdet_pyramid_results`` (the size gate)."""
        from ..tiles import tile_maps
        if levels is not None:
            posts = self._post_batch(np.asarray(dets), grid.metas * B, 1.0)
            return [ctdet_pyramid_results(posts[b * grid.T:(b + 1) * grid.T], grid.cores, grid.gates,
                                          self.opt.num_classes, self.opt.nms, max_per_frame) for b in range(B)]
        metas = tile_maps(grid, self.opt.down_ratio)[0]
        posts = self._post_batch(np.asarray(dets), metas * B, 1.0)
        return [ctdet_tiles_results(posts[b * grid.T:(b + 1) * grid.T], grid.cores, self.opt.num_classes,
                                    self.opt.nms, max_per_frame) for b in range(B)]

    def run_tiles(self, frames, overlap=None, margin=None, tile_batch=32, max_per_frame=None, pixel_format='bgr',
                  levels=None, size_gate=None, gate_slack=0.25):
        """``TilesMixin.run_tiles``, and with ``levels`` a tile PYRAMID for objects larger than
        the overlap, which no native-resolution tile sees whole: ``levels`` is a strictly increasing tuple of
        integers in [0, 3]; level l is the frame box-filtered by 2**l (``cn_tile_box_normalize_u8_f32``, straight
        from the frame) and tiled like the frame itself, ``overlap`` and ``margin`` in that level's pixels
        (``tiles.pyramid_grid``).  Every level answers for the object sizes it sees whole: with s = max(w, h) of
        a box in frame pixels and g = ``size_gate`` (pixels of a tile, by default min(overlap)), the boundary
        between consecutive listed levels a < b is g * 2**a; level a keeps s below boundary * (1 + gate_slack),
        level b from boundary * (1 - gate_slack) on, and the soft-NMS of the merge
        (``cn_ctdet_tiles_merge_gated_f32``) removes what both bands report.  The defaults are definitions from
        the geometry, not tuned values.  ``levels=None``: no pyramid, exactly the call without the keyword;
        ``levels=(0,)`` gives the same results through the pyramid's kernels.  More than 65536 rows per frame
        (tiles x K) and bad ``levels`` / ``size_gate`` / ``gate_slack`` raise ``ValueError``."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        return self._tiles_run(frames, args, pixel_format, **self._pyramid_options(args, levels, size_gate, gate_slack))

    def run_tiles_stream(self, batches, depth=3, overlap=None, margin=None, tile_batch=32, max_per_frame=None,
                         pixel_format='bgr', levels=None, size_gate=None, gate_slack=0.25):
        """``run_tiles`` over an iterable of batches, pipelined (``TilesMixin.run_tiles_stream``)."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        yield from self._tiles_stream(batches, depth, args, pixel_format,
                                      **self._pyramid_options(args, levels, size_gate, gate_slack))


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
        if pipe.gates_dev is not None:       # a tile pyramid: the size gate of every tile's level in the filter
            native.check(native.lib().cn_ctdet_tiles_merge_gated_f32(
                native.ptr(self.tile_rows), native.ptr(self.tile_bounds), pipe.B, pipe.T, opt.K, opt.num_classes,
                native.ptr(pipe.cores_dev), native.ptr(pipe.gates_dev), int(bool(opt.nms)), pipe.max_per_frame,
                native.ptr(self.out['rows']), native.ptr(self.out['bounds']), native.ptr(self.out['status']),
                native.ptr(self.ws), self.ws_bytes, native.stream_ptr()), "cn_ctdet_tiles_merge_gated_f32")
            return super(TilesTail, self).finish(slot)
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
