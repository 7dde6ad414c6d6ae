"""exdet task -- ExtremeNet-style detection (public behaviour of src/lib/detectors/exdet.py:23-118):
four extreme-point heat-maps + a centre map per class on the HIP network, grouped into boxes by
``cn_exct_decode_f32`` (K^4 candidate scoring with the edge aggregation of --aggr_weight in front);
--agnostic_ex: one extreme-point map per edge for all classes, ``cn_agnex_ct_decode_f32``;
--ex_stream: the ``_stream_f32`` forms of both, which keep no K^4 array and take the reference's --K 100.

Two things the reference's class does are kept as they are, because they ARE its results:
* ``post_process`` reads the decode's rows as TWO images -- the frame and its mirror image -- and
  un-mirrors the second half's box (exdet.py:87-91): the task is meant to run with --flip_test (its
  batch is then [frame, mirrored frame]); without it the second half of the single image's rows is
  mirrored all the same;
* only the box corners go through the inverse affine; the eight extreme-point coordinates of a row
  stay in output-grid units (exdet.py:92-96) and are dropped by ``merge_outputs``.
One thing differs: the reference's ``merge_outputs`` calls ``soft_nms`` without importing it
(exdet.py:110 -- a NameError as shipped); here it is the library's (external/nms.pyx:77-170).
New surface: ``run_batch`` (device-resident batches) and ``run_frames`` / ``run_frames_stream`` with the
task's tail on the device (``cn_exdet_post_process_f32`` + ``cn_exdet_merge_f32``)."""
import functools
import time

import numpy as np
import torch

from ..decode import agnex_ct_decode, exct_decode
from .. import native
from ..frame_pipe import DeviceTail
from ..image import transform_preds
from ..post_process import exdet_post_batch, exdet_results_batch
from ..soft_nms import soft_nms
from .base_detector import BaseDetector

EDGE_MAPS = ('hm_t', 'hm_l', 'hm_b', 'hm_r', 'hm_c')
EDGE_OFFSETS = ('reg_t', 'reg_l', 'reg_b', 'reg_r')


class ExdetDetector(BaseDetector):
    def __init__(self, opt):
        self.ex_stream = bool(getattr(opt, 'ex_stream', False))
        if self.ex_stream:
            if opt.K > native.EXCT_STREAM_MAX_K:
                raise ValueError("the exdet task with --ex_stream needs --K <= %d (K^4 candidate indices)"
                                 % native.EXCT_STREAM_MAX_K)
        elif opt.K > native.EXCT_STORED_MAX_K:
            # the reference would score K^4 = 10^8 groupings per image at the --K default of 100; the stored
            # kernel takes K <= 64 (cn_exct_decode_f32), ExtremeNet's own setting is 40
            raise ValueError("the exdet task needs --K <= 64 (K^4 candidate groupings per image); use --K 40, "
                             "or --ex_stream for --K up to %d" % native.EXCT_STREAM_MAX_K)
        super(ExdetDetector, self).__init__(opt)
        decode = agnex_ct_decode if opt.agnostic_ex else exct_decode           # exdet.py:26
        # --ex_stream: the streaming grouping at every K; without it the decode's own choice (the stored form here)
        self.decode = functools.partial(decode, stream=True) if self.ex_stream else decode

    def process(self, images, return_time=False):
        """exdet.py:28-55: the five maps post-sigmoid (in place, as there), then ``exct_decode`` with
        the sub-pixel offsets of the four edges when the network has them -> (B, 1000, 14)."""
        with torch.no_grad():
            output = self.model(images, borrow=True, check=True)[-1]
            heats = [output[n].sigmoid_() for n in EDGE_MAPS]
            torch.cuda.synchronize()
            forward_time = time.time()
            offsets = [output[n] for n in EDGE_OFFSETS] if self.opt.reg_offset else []
            dets = self.decode(*(heats + offsets), K=self.opt.K, scores_thresh=self.opt.scores_thresh,
                               center_thresh=self.opt.center_thresh, aggr_weight=self.opt.aggr_weight)
        return (output, dets, forward_time) if return_time else (output, dets)

    def post_process(self, dets, meta, scale=1):
        """(B, 1000, 14) rows [x1, y1, x2, y2, score, 8 extreme-point coords, class] -> ONE (n, 14)
        array: second half un-mirrored, box corners in source pixels of the unscaled frame."""
        out_w, out_h = meta['out_width'], meta['out_height']
        rows = dets.detach().cpu().numpy().reshape(2, -1, 14)
        left, right = rows[1, :, 0].copy(), rows[1, :, 2].copy()
        rows[1, :, 0], rows[1, :, 2] = out_w - right, out_w - left
        rows = rows.reshape(1, -1, 14)
        rows[0, :, 0:2] = transform_preds(rows[0, :, 0:2], meta['c'], meta['s'], (out_w, out_h))
        rows[0, :, 2:4] = transform_preds(rows[0, :, 2:4], meta['c'], meta['s'], (out_w, out_h))
        rows[:, :, 0:4] /= scale
        return rows[0]

    def merge_outputs(self, detections):
        """All scales together, rows with a positive score only, soft-NMS (Gaussian, Nt 0.5) per class,
        then the ``max_per_image`` best over all classes, ties kept (exdet.py:99-123)."""
        rows = np.concatenate(list(detections), axis=0).astype(np.float32)
        rows = rows[rows[:, 4] > 0]
        classes = rows[:, -1]
        results = {}
        for j in range(self.num_classes):
            boxes = np.ascontiguousarray(rows[classes == j][:, 0:5])    # (the routine touches columns 0-4 only)
            soft_nms(boxes, Nt=0.5, method=2)
            results[j + 1] = boxes
        scores = np.hstack([results[j][:, -1] for j in range(1, self.num_classes + 1)])
        if len(scores) > self.max_per_image:
            kth = len(scores) - self.max_per_image
            thresh = np.partition(scores, kth)[kth]
            for j in range(1, self.num_classes + 1):
                results[j] = results[j][results[j][:, -1] >= thresh]
        return results

    # ------------------------------------------------------------------ new surface
    def run_batch(self, images):
        """``images`` (N, 3, H, W) fp32, already normalised, on the device -> raw (N, 1000, 14) rows of the
        decode in output-grid units (device tensor); the five maps are left post-sigmoid, as ``process``
        leaves them.  Asynchronous, as ``CtdetDetector.run_batch``: nothing here waits for the device, the
        caller owes a ``range_ok()`` where it consumes the rows."""
        self._note_unchecked_forward()
        with torch.no_grad():
            output = self.model(images, borrow=True)[-1]
            heats = [output[n].sigmoid_() for n in EDGE_MAPS]
            offsets = [output[n] for n in EDGE_OFFSETS] if self.opt.reg_offset else []
            return self.decode(*(heats + offsets), K=self.opt.K, scores_thresh=self.opt.scores_thresh,
                               center_thresh=self.opt.center_thresh, aggr_weight=self.opt.aggr_weight)

    def _run_scale(self, images, flip):
        """One test scale of the frame pipeline: ``run_batch``, the rows seen per FRAME -- (B, R, 14) with
        R = 2000 under ``flip`` ((2B, 3, H, W) frame / mirror pairs: a frame's rows, then its mirror
        image's, the ``reshape(2, -1, 14)`` of ``post_process``) and 1000 without.  This task has no flip
        average: the mirror image's rows are rows."""
        dets = self.run_batch(images)
        return dets.view(-1, (2 if flip else 1) * dets.shape[1], dets.shape[2])

    # ---- host tail of the frame pipeline: the fallback, and the comparison side of the device tail
    def results_batch(self, dets, metas, scale):
        """(n, R, 14) host rows of one test scale -> per frame ``{class: (n, 5) float32}``."""
        return exdet_results_batch([(dets, metas, scale)], self.num_classes, self.max_per_image)

    def _post_batch(self, dets, metas, scale):
        """``post_process`` of every frame of a (n, R, 14) host array: a list of (R, 14) arrays."""
        return list(exdet_post_batch(dets, metas, scale))

    def _device_tail(self, pipe):
        return ExdetTail(pipe) if ExdetTail.admits(pipe) else None


class ExdetTail(DeviceTail):
    """cn_exdet_post_process_f32 per test scale and cn_exdet_merge_f32 -- always, whatever ``pipe.merge`` says:
    soft-NMS and the cut are this task's ``merge_outputs`` for one scale too."""

    @classmethod
    def admits(cls, pipe):
        """Not with more classes than the kernels take.  The row cap is not decided here: it holds for the rows
        with a positive score, which only the batch itself tells (``status``)."""
        return pipe.det.num_classes <= native.MERGE_MAX_CLASSES

    def __init__(self, pipe):
        super(ExdetTail, self).__init__(pipe)
        nc, B, S = self.det.num_classes, pipe.B, len(pipe.scales)
        self.R = R = (2 if pipe.flip else 1) * 1000          # (num_dets of exct_decode / agnex_ct_decode)
        self.scale_rows = torch.empty((S, B, R, 5), device=self.device, dtype=torch.float32)
        self.scale_bounds = torch.empty((S, B, nc + 1), device=self.device, dtype=torch.int32)
        self.output('rows', (B, min(S * R, native.MERGE_MAX_ROWS), 5), torch.float32)
        self.output('bounds', (B, nc + 1), torch.int32)
        self.output('status', (B,), torch.int32)

    def run(self, slot, level, dets):
        """Raw rows -> un-mirrored, in source pixels / scale, positive scores only, grouped by class, into
        slice ``level``."""
        pipe, lv = self.pipe, self.pipe.levels[level]
        dets = dets.contiguous()
        if tuple(dets.shape) != (pipe.B, self.R, 14):
            raise native.NativeError("exdet tail: rows of shape %s, expected %s"
                                     % (tuple(dets.shape), (pipe.B, self.R, 14)))
        native.check(native.lib().cn_exdet_post_process_f32(
            native.ptr(dets), pipe.B, self.R, self.det.num_classes, int(lv.meta['out_width']),
            *self.source_map(slot, level), float(lv.scale), native.ptr(self.scale_rows[level]),
            native.ptr(self.scale_bounds[level]), native.stream_ptr()), "cn_exdet_post_process_f32")

    def finish(self, slot):
        pipe, det, out = self.pipe, self.det, self.out
        native.check(native.lib().cn_exdet_merge_f32(
            native.ptr(self.scale_rows), native.ptr(self.scale_bounds), len(pipe.scales), pipe.B, self.R,
            det.num_classes, det.max_per_image, native.ptr(out['rows']), native.ptr(out['bounds']),
            native.ptr(out['status']), native.stream_ptr()), "cn_exdet_merge_f32")
        super(ExdetTail, self).finish(slot)

    def results(self, slot, n):
        """Per frame ``{class: (n, 5) float32}``, slices of a copy of the merged rows -- or None when a frame of
        the batch had more positive rows than the merge kernel holds: the pipe then runs the batch through the
        host tail."""
        if self.host('status', slot).numpy().any():
            return None
        return self.class_slices(self.host('rows', slot).numpy().copy(), self.host('bounds', slot).numpy().tolist(),
                                 n, self.det.num_classes)
