"""ddd task -- monocular 3-D detection (public behaviour of src/lib/detectors/ddd.py:22-91): centre
heat-map + depth + orientation bins + box dimensions (+ 2-D size and sub-pixel offset) on the HIP
network, decoded by ``cn_ddd_decode_f32`` (``run_batch`` and the frame pipe: top-K on ``hm``, then the other heads at
the K cells only, ``cn_ddd_heads_at_cells_f32``), lifted to camera coordinates on the host
(``post_process.ddd_post_process``).  ``run(image, calib)``: the second argument is the frame's
3 x 4 projection matrix (test.py:37-39,105-106); without it the detector's KITTI default is used.
New surface: ``run_frames(frames, calibs)`` / ``run_frames_stream`` -- batches of frames, each with its
own matrix, pre-processed (``cn_warp_table_u8_f32_batch``) and lifted (``cn_ddd_post_process_f32``) on the
device -- and ``run_images(images, calibs)`` / ``run_images_stream``, the same for images of mixed sizes (KITTI
has several): the pre-process never resizes, so a mixed-size batch is the ``run_frames`` batch with one map in
(``cn_warp_table_u8_f32_ragged``) and one map out per image."""
import ctypes
import itertools
import time

import numpy as np
import torch

from .. import native
from ..decode import ddd_decode, ddd_decode_at_cells
from ..frame_pipe import DeviceTail
from ..image import get_affine_transform, invert_affine, warp_affine
from ..post_process import ddd_norm_table, ddd_post_process, ddd_results_batch
from .base_detector import BaseDetector, InputGeometry


def deferred_ddd_heads(opt):
    """The heads ``run_batch`` (and with it the frame pipe) leaves to the decode: ``ddd_decode`` scans only
    ``hm`` densely and gathers ``dep``, ``rot``, ``dim`` (``wh`` with --reg_bbox, ``reg`` with --reg_offset) at the
    K decoded centres (decode.py:426-462), so their dense maps are not computed.  Nothing with K > 128 or when a
    head the options ask for is missing; the network side (fp32 compute mode, fusable 3x3 + 1x1 heads) is the
    plan builder's decision."""
    names = ('dep', 'rot', 'dim') + (('wh',) if opt.reg_bbox else ()) + (('reg',) if opt.reg_offset else ())
    if opt.K > 128 or any(n not in opt.heads for n in names):
        return ()
    return names


class DddDetector(BaseDetector):
    def __init__(self, opt):
        super(DddDetector, self).__init__(opt)
        self.calib = np.array([[707.0493, 0, 604.0814, 45.75831],
                               [0, 707.0493, 180.5066, -0.3454157],
                               [0, 0, 1., 0.004981016]], dtype=np.float32)     # ddd.py:25-27

    # ------------------------------------------------------------------ pre-process
    def _frame_geometry(self, height, width):
        """Centre, extent and the frame -> network-input map (ddd.py:31-42): the frame is NOT resized
        or padded to a multiple; it is warped straight onto the fixed input size, the extent being
        the frame's own (width, height) -- or the input's under --keep_res -- as int32, x first."""
        inp_h, inp_w = self.opt.input_h, self.opt.input_w
        c = np.array([width / 2, height / 2], dtype=np.float32)
        s = np.array([inp_w, inp_h] if self.opt.keep_res else [width, height], dtype=np.int32)
        return c, s, get_affine_transform(c, s, 0, [inp_w, inp_h])

    def _meta(self, c, s, calib):
        return {'c': c, 's': s, 'out_height': self.opt.input_h // self.opt.down_ratio,
                'out_width': self.opt.input_w // self.opt.down_ratio,
                'calib': self.calib if calib is None else np.array(calib, dtype=np.float32)}

    def pre_process(self, image, scale, calib=None):
        """Host form (ddd.py:30-54); ``scale`` is accepted and unused, as in the reference.  The
        normalisation is the ddd class's own FLOAT32 chain ``(u8 / 255 - mean) / std`` (ddd.py:45-46) --
        not the float64-then-round of the other tasks (base_detector.py:56) -- taken through a 256-entry
        table per channel built with exactly those float32 operations."""
        c, s, to_input = self._frame_geometry(image.shape[0], image.shape[1])
        warped = warp_affine(image, to_input, (self.opt.input_w, self.opt.input_h))
        table = self.norm_table()
        batch = np.stack([table[ch][warped[:, :, ch]] for ch in range(3)])[None]
        return torch.from_numpy(np.ascontiguousarray(batch)), self._meta(c, s, calib)

    def norm_table(self, device=False):
        """The (3, 256) float32 table of the ddd normalisation (``post_process.ddd_norm_table``), built
        once per detector; ``device``: its copy in HBM (what ``cn_warp_table_u8_f32_batch`` reads)."""
        d = self.__dict__
        if "_norm_table" not in d:
            d["_norm_table"] = ddd_norm_table(self.mean, self.std)
        if not device:
            return d["_norm_table"]
        if "_norm_table_dev" not in d:
            d["_norm_table_dev"] = torch.from_numpy(d["_norm_table"]).to(self.opt.device)
        return d["_norm_table_dev"]

    def _warp_table(self, frames, to_input, out, stream=None):
        """(N, H, W, 3) uint8 frames on the device -> ``out`` (N, 3, input_h, input_w), one launch."""
        N, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        dst_to_src = to_input if isinstance(to_input, ctypes.Array) else \
            (ctypes.c_double * 6)(*invert_affine(to_input).reshape(-1))
        native.check(native.lib().cn_warp_table_u8_f32_batch(
            native.ptr(frames), N, H * W * 3, H, W, W * 3, dst_to_src, self.opt.input_h, self.opt.input_w,
            native.ptr(self.norm_table(device=True)), native.ptr(out),
            native.stream_ptr() if stream is None else stream), "cn_warp_table_u8_f32_batch")

    def pre_process_device(self, image, scale, calib=None, out=None, pixel_format='bgr'):
        """The same on the device: the uint8 frame (a numpy array, or a uint8 HIP tensor that is already
        uploaded) through ``cn_warp_table_u8_f32_batch`` -- the warp of the other tasks with the float32
        normalisation looked up in ``norm_table``.  Bit-identical to ``pre_process``.  ``pixel_format``: as
        ``BaseDetector.pre_process_device`` ('nv12': an (H * 3 // 2, W) frame, converted on the device first)."""
        dev = self.opt.device
        frame = self._device_frame(image, pixel_format)
        shape = (1, 3, self.opt.input_h, self.opt.input_w)
        if out is None:
            out = torch.empty(shape, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("pre_process_device: `out` must be a contiguous %s tensor" % (shape,))
        c, s, to_input = self._frame_geometry(int(frame.shape[0]), int(frame.shape[1]))
        self._warp_table(frame[None], to_input, out)
        return out, self._meta(c, s, calib)

    # ------------------------------------------------------------------ network + decode
    def _deferred_heads(self):
        return deferred_ddd_heads(self.opt)

    def _decode_batch(self, o, raw_depth=False):
        """Raw (B, K, 18) rows of ``ddd_decode``, the centre map's sigmoid fused into the decode: from a
        deferred-heads forward the top-K on ``hm`` and the other heads at the K cells only, the depth transform
        of the K values in that kernel.  From dense maps ``run_batch`` transforms the depth map on the host side
        as ``process`` does; the frame pipe (``raw_depth``) leaves the K gathered values to ``cn_ddd_decode_f32``."""
        opt = self.opt
        if '_deferred' in o:
            return ddd_decode_at_cells(o['hm'], o['_deferred'], K=opt.K, apply_sigmoid=True, raw_depth=True)
        dep = o['dep'] if raw_depth else 1. / (o['dep'].sigmoid() + 1e-6) - 1.
        return ddd_decode(o['hm'], o['rot'], dep, o['dim'], wh=o['wh'] if opt.reg_bbox else None,
                          reg=o['reg'] if opt.reg_offset else None, K=opt.K, apply_sigmoid=True,
                          raw_depth=raw_depth)

    def process(self, images, return_time=False):
        """ddd.py:56-73: post-sigmoid centre map, depth = 1 / (sigmoid(dep) + 1e-6) - 1, then
        ``ddd_decode``.  The returned ``output`` holds the maps in that transformed state."""
        with torch.no_grad():
            output = self.model(images, borrow=True, check=True)[-1]
            output['hm'] = output['hm'].sigmoid_()
            output['dep'] = 1. / (output['dep'].sigmoid() + 1e-6) - 1.
            wh = output['wh'] if self.opt.reg_bbox else None
            reg = output['reg'] if self.opt.reg_offset else None
            torch.cuda.synchronize()
            forward_time = time.time()
            dets = ddd_decode(output['hm'], output['rot'], output['dep'], output['dim'], wh=wh, reg=reg,
                              K=self.opt.K)
        return (output, dets, forward_time) if return_time else (output, dets)

    def post_process(self, dets, meta, scale=1):
        """(1, K, 18) rows in output-grid units -> {class: (n, 13) float32 [alpha, x1, y1, x2, y2, h, w,
        l, x, y, z, rotation_y, score]} in source pixels / camera metres (ddd.py:75-80)."""
        host = dets.detach().cpu().numpy()
        per_image = ddd_post_process(host.copy(), [meta['c']], [meta['s']], [meta['calib']], self.opt)
        self.this_calib = meta['calib']
        return per_image[0]

    def merge_outputs(self, detections):
        """Single scale: the first entry, every class cut at --peak_thresh (ddd.py:82-88)."""
        results = detections[0]
        for j in range(1, self.num_classes + 1):
            if len(results[j]) > 0:
                results[j] = results[j][results[j][:, -1] > self.opt.peak_thresh]
        return results

    # ------------------------------------------------------------------ frame pipe
    _pipe_side_shape = (3, 4)        # one projection matrix per frame rides with the batch

    def _calibs_for(self, frames, calibs):
        """``run_frames``' ``calibs`` -> (n, 3, 4) float32, one matrix per frame: a single (3, 4) matrix
        serves every frame; a sequence gives one per frame, ``None`` entries meaning the detector's default."""
        n = len(frames)
        if calibs is None:
            raise NotImplementedError(
                "run_frames / run_frames_stream of the ddd task need the frames' projection matrices: pass "
                "calibs= (one (3, 4) matrix for all frames, or one per frame; a None entry = the detector's "
                "KITTI default).  Lifting a whole video with an assumed default would return wrong metres.")
        try:
            if not isinstance(calibs, np.ndarray):
                calibs = [self.calib if m is None else m for m in calibs]
            arr = np.array(calibs, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("calibs: a (3, 4) matrix, or a sequence of %d of them (None = default)" % n)
        if arr.shape == (3, 4):
            arr = np.broadcast_to(arr, (n, 3, 4))
        if arr.shape != (n, 3, 4):
            raise ValueError("calibs: a (3, 4) matrix or %d of them for %d frames, got shape %s"
                             % (n, n, arr.shape))
        return np.ascontiguousarray(arr)

    def _frames_and_side(self, batch):
        try:
            frames, calibs = batch
        except (TypeError, ValueError):
            raise ValueError("run_frames_stream of the ddd task takes (frames, calibs) pairs")
        return frames, self._calibs_for(frames, calibs)

    def _pipe_scales(self):
        return self.scales[:1]       # ddd.py:82-88: the first scale is the result

    def _pipe_level(self, height, width, scale):
        """No resize, no padding: the frame is warped straight onto the fixed input (``_frame_geometry``)."""
        c, s, to_input = self._frame_geometry(height, width)
        g = InputGeometry(height, width, height, width, self.opt.input_h, self.opt.input_w, c, s)
        return g, to_input, self._meta(c, s, None)

    def _pipe_pre_process(self, pipe, lv, src, stream):
        self._warp_table(src, lv.dst_to_src, lv.batch, stream)

    def run_frames(self, frames, calibs=None, pixel_format='bgr'):
        """A list of (H, W, 3) uint8 BGR frames of one size and their projection matrices -> per frame what
        ``run(frame_i, calib_i)['results']`` returns: ``{class: (n, 13) float32}``, a class without rows a
        ``(0,)`` array, a class whose rows were all cut at --peak_thresh ``(0, 13)``.  ``calibs``: one
        (3, 4) matrix for all frames, or a sequence with one per frame (``None`` = the detector's default
        matrix); every frame is lifted with ITS matrix (the reference's single-image detector lifts with
        ``calibs[0]``).  One uint8 upload, one pre-process launch, one network step, one decode (the
        depth transform inside it) and one tail launch per batch; the host slices the rows.
        ``pixel_format='nv12'``: (H * 3 // 2, W) NV12 frames, or one (B, H * 3 // 2, W) uint8 HIP tensor, as
        ``BaseDetector.run_frames`` takes them; converted on the device in front of the warp."""
        side = self._calibs_for(frames, calibs)
        pipe = self._pipe_for(frames, 1, pixel_format)
        pipe.submit(0, frames, side)
        return pipe.collect(0, frames)

    def run_frames_stream(self, batches, depth=3, pixel_format='bgr'):
        """``run_frames`` over an iterable of ``(frames, calibs)`` pairs (all batches of one size and frame
        geometry), pipelined as ``BaseDetector.run_frames_stream``; the matrices are staged in pinned
        memory and uploaded on the copy stream with their frames.  ``pixel_format``: as ``run_frames``."""
        return super(DddDetector, self).run_frames_stream(batches, depth, pixel_format=pixel_format)

    # ------------------------------------------------------------------ images of mixed sizes
    def _fixed_input(self):
        return True      # --keep_res changes the extent only (_frame_geometry): the input size never follows the image

    def _pipe_pre_process_images(self, pipe, lv, src, descs, stream):
        native.check(native.lib().cn_warp_table_u8_f32_ragged(
            native.ptr(src), descs, pipe.B, self.opt.input_h, self.opt.input_w,
            native.ptr(self.norm_table(device=True)), native.ptr(lv.batch), stream), "cn_warp_table_u8_f32_ragged")

    def _images_and_side(self, batch):
        """An item of ``run_images_stream`` -> (images, their (n, 3, 4) matrices); an item that is no
        ``(images, calibs)`` pair, or has no matrices, is refused as ``run_frames`` refuses missing matrices."""
        try:
            images, calibs = batch
        except (TypeError, ValueError):
            images, calibs = batch, None
        if isinstance(images, np.ndarray) and images.ndim == 3:      # a list of two images, not a pair
            images, calibs = batch, None
        return images, self._calibs_for(images, calibs)

    def run_images(self, images, calibs=None):
        """A list of (H_i, W_i, 3) uint8 BGR images of ANY sizes and their projection matrices -> per image what
        ``run(image_i, calib_i)['results']`` returns (the result shapes of ``run_frames``).  ``calibs``: as
        ``run_frames`` takes them.  The images are packed back to back into one uint8 upload with a table of
        per-image descriptors, warped by ONE ``cn_warp_table_u8_f32_ragged`` launch (no level resizes), and the
        tail lifts image b with its own inverse map and matrix b.  --keep_res changes only the extent, the
        network input stays (input_h, input_w): mixed sizes are valid with it too."""
        side = self._calibs_for(images, calibs)
        self._images_one_size(images, "run_images")
        pipe = self._image_pipe_for(images, 1)
        pipe.submit(0, images, side)
        return pipe.collect(0, images)

    def run_images_stream(self, batches, depth=3):
        """``run_images`` over an iterable of ``(images, calibs)`` pairs, every batch of one length, pipelined as
        ``run_frames_stream``.  The first item is looked at here, at the call: a stream without matrices is
        refused before anything is yielded."""
        batches = iter(batches)
        first = list(itertools.islice(batches, 1))
        for batch in first:
            self._images_and_side(batch)
        return super(DddDetector, self).run_images_stream(itertools.chain(first, batches), depth)

    def _run_scale(self, images, flip):
        """Network + decode of the frame pipeline: the centre map's sigmoid and the depth transform of
        the K gathered cells are inside the decode kernels; raw (B, K, 18) rows, asynchronous."""
        self._note_unchecked_forward()
        with torch.no_grad():
            return self._decode_batch(self._forward_deferred(images), raw_depth=True)

    def _run_frames_sync(self, frames, scales, side=None):
        """One batch synchronously (the pipe's re-run path after an f32s re-calibration)."""
        uploaded = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(self.opt.device)
        return self._run_uploaded_sync(uploaded, scales, side=side)

    def _run_uploaded_sync(self, uploaded, scales, side=None):
        """``_run_frames_sync`` of a (n, H, W, 3) uint8 batch that is on the device."""
        n = int(uploaded.shape[0])
        c, s, to_input = self._frame_geometry(int(uploaded.shape[1]), int(uploaded.shape[2]))
        batch = torch.empty((n, 3, self.opt.input_h, self.opt.input_w), device=self.opt.device, dtype=torch.float32)
        self._warp_table(uploaded, to_input, batch)
        dets = self._forward_checked(batch, False)
        return self.results_batch(dets, [self._meta(c, s, None)] * n, 1.0, side=side)

    def _run_images_sync(self, images, scales, side=None):
        """``_run_frames_sync`` for images of any sizes: each image uploaded on its own, warped into its slice
        of the batch, with its own meta (the comparison path of ``run_images`` and its re-run path)."""
        batch = torch.empty((len(images), 3, self.opt.input_h, self.opt.input_w), device=self.opt.device,
                            dtype=torch.float32)
        metas = [self.pre_process_device(f, 1.0, out=batch[i:i + 1])[1] for i, f in enumerate(images)]
        dets = self._forward_checked(batch, False)
        return self.results_batch(dets, metas, 1.0, side=side)

    def results_batch(self, dets, metas, scale, side=None):
        """Host tail of ``run_frames``: (n, K, 18) host rows, the frames' metas and their (n, 3, 4) matrices
        (``side``; else each meta's own 'calib') -> per image what ``run(frame, calib)['results']`` returns."""
        if side is not None:
            metas = [dict(m, calib=p) for m, p in zip(metas, side)]
        return ddd_results_batch(dets, metas, self.num_classes, self.opt.peak_thresh)

    def _device_tail(self, pipe):
        return DddTail(pipe) if DddTail.admits(pipe) else None


class DddTail(DeviceTail):
    """cn_ddd_post_process_f32: lifted rows grouped by class, the class bounds and per class the length of
    the --peak_thresh prefix; image b with matrix b of the slot's uploaded batch of matrices.  No merge."""

    @classmethod
    def admits(cls, pipe):
        """Not with more rows than the kernel takes, or rows without the (w, h) columns."""
        return not (pipe.det.opt.K > 128 or not pipe.det.opt.reg_bbox)

    def __init__(self, pipe):
        super(DddTail, self).__init__(pipe)
        K, nc, B = self.det.opt.K, self.det.num_classes, pipe.B
        self.output('rows', (B, K, 13), torch.float32)
        self.output('bounds', (B, nc + 1), torch.int32)
        self.output('kept', (B, nc), torch.int32)

    def run(self, slot, level, dets):
        pipe, det, out = self.pipe, self.det, self.out
        dets = dets.contiguous()
        to_source, per_image = self.source_map(slot, level)
        native.check(native.lib().cn_ddd_post_process_f32(
            native.ptr(dets), pipe.B, det.opt.K, int(dets.shape[2]), det.num_classes, to_source,
            per_image, native.ptr(pipe.side_dev[slot]), float(det.opt.peak_thresh), native.ptr(out['rows']),
            native.ptr(out['bounds']), native.ptr(out['kept']), native.stream_ptr()), "cn_ddd_post_process_f32")

    def results(self, slot, n):
        """Per image ``{class: (n, 13) float32}``: slices of the grouped rows (a copy of the pinned
        buffer), the empty class a (0,) array as the reference's ``np.array([])``."""
        nc = self.det.num_classes
        rows = self.host('rows', slot).numpy().copy()        # (the pinned buffer is reused by a later batch)
        bounds = self.host('bounds', slot).numpy().tolist()
        kept = self.host('kept', slot).numpy().tolist()
        out = []
        for i in range(n):
            r, bd, kp = rows[i], bounds[i], kept[i]
            out.append({j + 1: r[bd[j]:bd[j] + kp[j]] if bd[j + 1] > bd[j] else np.array([], dtype=np.float32)
                        for j in range(nc)})
        return out
