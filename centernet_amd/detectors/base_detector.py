"""Task API base class.

Public surface and semantics follow the reference's ``BaseDetector``
(src/lib/detectors/base_detector.py:16-143): ``pre_process``, ``process``, ``post_process``,
``merge_outputs`` and ``run(image_or_path_or_tensor, meta=None)`` which returns
``{'results', 'tot', 'load', 'pre', 'net', 'dec', 'post', 'merge'}``.  The implementation is
organised differently: the input geometry lives in one helper shared by the host and the device
pre-process, the time buckets are kept by a small phase clock, and ``run`` sends uint8 frames
through the device pre-process (``cn_resize_bilinear_u8`` + ``cn_warp_normalize_u8_f32``).
New surface (the reference is single-image only): ``run_batch`` / ``run_frames`` in the task
classes.
"""
import collections
import ctypes
import time

import numpy as np
import torch

from .. import native
from ..frame_pipe import FramePipe, ImagePipe, ImageTables
from ..image import (check_pixel_format, get_affine_transform, invert_affine, normalize_chw, nv12_size,
                     resize_bilinear, warp_affine)
from ..model import create_model, load_model

InputGeometry = collections.namedtuple(
    "InputGeometry", "src_h src_w scaled_h scaled_w inp_h inp_w center extent")


class _PhaseClock(object):
    """Wall-clock buckets of ``run`` ('load', 'pre', 'net', 'dec', 'post', 'merge', 'tot').
    A lap synchronises the device first -- the reference's explicit
    ``torch.cuda.synchronize()`` calls (base_detector.py:112-134)."""

    def __init__(self):
        self.t = dict.fromkeys(("load", "pre", "net", "dec", "post", "merge", "tot"), 0.0)
        self._start = self._last = time.time()

    def lap(self, bucket, sync=True, until=None):
        if sync:
            torch.cuda.synchronize()
        now = time.time() if until is None else until
        self.t[bucket] += now - self._last
        self._last = now

    def finish(self):
        self.t["tot"] = self._last - self._start
        return self.t


class BaseDetector(object):
    def __init__(self, opt):
        if opt.gpus[0] < 0:
            raise native.NativeError("--gpus -1 (CPU) is not supported: centernet_amd is the "
                                     "MI355X path and has no CPU fallback")
        opt.device = torch.device('cuda')
        print('Creating model...')
        net = create_model(opt.arch, opt.heads, opt.head_conv)
        if opt.load_model:
            net = load_model(net, opt.load_model)
        self.model = net.to(opt.device).eval()
        if getattr(opt, 'fp32_mfma', False):
            self.model.fp32_mfma()
        if getattr(opt, 'fp16', False):
            self.model.half_compute()
        self.opt = opt
        self.mean = np.asarray(opt.mean, np.float32).reshape(1, 1, 3)
        self.std = np.asarray(opt.std, np.float32).reshape(1, 1, 3)
        self.scales = opt.test_scales
        self.num_classes = opt.num_classes
        self.max_per_image = int(getattr(opt, 'max_per_image', 100))     # (--max_per_image; the reference: 100)
        if self.max_per_image < 1:
            raise ValueError("--max_per_image must be at least 1, got %d" % self.max_per_image)
        self.pause = True
        self.tail_fallbacks = 0      # batches of the frame pipe that its device tail handed back to the host
        self.model.defer_heads(self._deferred_heads())

    # ------------------------------------------------------------------ input geometry
    def input_geometry(self, height, width, scale):
        """Network input size, centre and extent for one test scale (base_detector.py:38-50):
        the fixed resolution, or the scaled image size rounded up to a multiple of pad + 1."""
        scaled_h, scaled_w = int(height * scale), int(width * scale)
        if self.opt.fix_res:
            inp_h, inp_w = self.opt.input_h, self.opt.input_w
            center = np.array([scaled_w / 2., scaled_h / 2.], dtype=np.float32)
            extent = max(height, width) * 1.0
        else:
            inp_h, inp_w = (scaled_h | self.opt.pad) + 1, (scaled_w | self.opt.pad) + 1
            center = np.array([scaled_w // 2, scaled_h // 2], dtype=np.float32)
            extent = np.array([inp_w, inp_h], dtype=np.float32)
        return InputGeometry(height, width, scaled_h, scaled_w, inp_h, inp_w, center, extent)

    def _meta(self, g):
        return {'c': g.center, 's': g.extent,
                'out_height': g.inp_h // self.opt.down_ratio,
                'out_width': g.inp_w // self.opt.down_ratio}

    # ------------------------------------------------------------------ frame pipe: geometry + pre-process
    _pipe_side_shape = None      # shape of a task's per-frame side input (ddd: (3, 4)), see FramePipe

    def _pipe_scales(self):
        """Task hook of the frame pipeline: the test scales a pipe runs."""
        return self.scales

    def _device_tail(self, pipe):
        """Task hook of the frame pipeline: the task's ``DeviceTail`` for ``pipe``, or None when the host
        tail (``results_batch`` / ``_results_merged``) serves it."""
        return None

    def _pipe_level(self, height, width, scale):
        """Task hook of the frame pipeline: (InputGeometry, frame -> network-input map, meta) of one test
        scale for (height, width) frames."""
        g = self.input_geometry(height, width, scale)
        return g, get_affine_transform(g.center, g.extent, 0, [g.inp_w, g.inp_h]), self._meta(g)

    def _pipe_pre_process(self, pipe, lv, src, stream):
        """Task hook of the frame pipeline: the batched device pre-process of level ``lv``, (B, h, w, 3)
        uint8 ``src`` on the device -> ``lv.batch``, one launch."""
        g = lv.g
        native.check(native.lib().cn_warp_normalize_u8_f32_batch(
            native.ptr(src), pipe.B, g.scaled_h * g.scaled_w * 3, g.scaled_h, g.scaled_w, g.scaled_w * 3,
            lv.dst_to_src, g.inp_h, g.inp_w, pipe.mean, pipe.std, int(pipe.flip), native.ptr(lv.batch), stream),
            "cn_warp_normalize_u8_f32_batch")

    def _pipe_pre_process_images(self, pipe, lv, src, descs, stream):
        """Task hook of the frame pipeline, ``_pipe_pre_process`` for a batch of mixed-size images: the packed
        uint8 images ``src`` on the device as the B ``cn_image_desc`` at ``descs`` (device memory) describe them
        -> ``lv.batch``, one launch."""
        native.check(native.lib().cn_warp_normalize_u8_f32_ragged(
            native.ptr(src), descs, pipe.B, int(lv.batch.shape[2]), int(lv.batch.shape[3]), pipe.mean, pipe.std,
            int(pipe.flip), native.ptr(lv.batch), stream), "cn_warp_normalize_u8_f32_ragged")

    # ------------------------------------------------------------------ pre-process
    def pre_process(self, image, scale, meta=None):
        """Host form (base_detector.py:37-65): resize, affine warp, normalise, CHW, flip concat.
        Usable from DataLoader workers; returns a CPU tensor and the meta dict."""
        g = self.input_geometry(image.shape[0], image.shape[1], scale)
        to_input = get_affine_transform(g.center, g.extent, 0, [g.inp_w, g.inp_h])
        warped = warp_affine(resize_bilinear(image, (g.scaled_w, g.scaled_h)), to_input,
                             (g.inp_w, g.inp_h))
        batch = normalize_chw(warped, self.mean, self.std)[None]
        if self.opt.flip_test:
            batch = np.concatenate((batch, batch[:, :, :, ::-1]), axis=0)
        return torch.from_numpy(np.ascontiguousarray(batch)), self._meta(g)

    def _nv12_to_bgr_device(self, nv12, out=None, stream=None):
        """(N, H * 3 // 2, W) uint8 NV12 frames on the device -> (N, H, W, 3) uint8 BGR on the device (``out``
        when given), one ``cn_nv12_to_bgr_u8_batch`` launch on ``stream`` (the current one by default)."""
        N = int(nv12.shape[0])
        H, W = nv12_size(tuple(nv12.shape[1:]))
        if out is None:
            out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=nv12.device)
        native.check(native.lib().cn_nv12_to_bgr_u8_batch(
            native.ptr(nv12), N, H * 3 // 2 * W, H, W, W, native.ptr(out),
            native.stream_ptr() if stream is None else stream), "cn_nv12_to_bgr_u8_batch")
        return out

    def _device_frame(self, image, pixel_format='bgr'):
        """``pre_process_device``'s frame on the device: a contiguous (H, W, 3) uint8 HIP tensor as it is, a
        uint8 numpy image uploaded; with ``pixel_format='nv12'`` an (H * 3 // 2, W) uint8 frame (numpy, or a
        contiguous HIP tensor), converted to BGR on the device."""
        if check_pixel_format(pixel_format) == 'nv12':
            if torch.is_tensor(image):
                if image.dtype != torch.uint8 or image.dim() != 2 or not image.is_cuda or not image.is_contiguous():
                    raise ValueError("pre_process_device needs a contiguous (H * 3 // 2, W) uint8 HIP tensor "
                                     "as an NV12 frame")
            elif not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim != 2:
                raise ValueError("pre_process_device needs an (H * 3 // 2, W) uint8 array as an NV12 frame")
            nv12_size(tuple(image.shape))
            if not torch.is_tensor(image):
                image = torch.from_numpy(np.ascontiguousarray(image)).to(self.opt.device)
            return self._nv12_to_bgr_device(image[None])[0]
        if torch.is_tensor(image):
            if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or \
                    not image.is_cuda or not image.is_contiguous():
                raise ValueError("pre_process_device needs a contiguous (H, W, 3) uint8 HIP tensor")
            return image
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("pre_process_device needs an (H, W, 3) uint8 BGR image")
        return torch.from_numpy(np.ascontiguousarray(image)).to(self.opt.device)

    def pre_process_device(self, image, scale, meta=None, out=None, pixel_format='bgr'):
        """The same steps on the device: the uint8 frame (a numpy array, or a uint8 HIP tensor
        that is already uploaded) goes through ``cn_resize_bilinear_u8`` (scale != 1) and
        ``cn_warp_normalize_u8_f32``; the fp32 (1|2,3,H,W) batch is produced in HBM -- into
        ``out`` when given.  Bit-identical to ``pre_process``.  ``pixel_format='nv12'``: ``image`` is an
        (H * 3 // 2, W) uint8 NV12 frame (numpy, or a contiguous HIP tensor), converted on the device first
        (``cn_nv12_to_bgr_u8_batch``); the result is that of ``image.nv12_to_bgr(frame)``, bit for bit.  Any
        other value raises ``ValueError``."""
        check_pixel_format(pixel_format)
        lib = native.lib()
        dev = self.opt.device
        frame = self._device_frame(image, pixel_format)
        g = self.input_geometry(int(frame.shape[0]), int(frame.shape[1]), scale)
        stream = native.stream_ptr()
        if (g.scaled_h, g.scaled_w) != (g.src_h, g.src_w):
            scaled = torch.empty((g.scaled_h, g.scaled_w, 3), device=dev, dtype=torch.uint8)
            native.check(lib.cn_resize_bilinear_u8(native.ptr(frame), g.src_h, g.src_w, g.src_w * 3,
                                                   g.scaled_h, g.scaled_w, native.ptr(scaled), stream),
                         "cn_resize_bilinear_u8")
            frame = scaled
        shape = (2 if self.opt.flip_test else 1, 3, g.inp_h, g.inp_w)
        if out is None:
            out = torch.empty(shape, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("pre_process_device: `out` must be a contiguous %s tensor" % (shape,))
        to_input = get_affine_transform(g.center, g.extent, 0, [g.inp_w, g.inp_h])
        dst_to_src = (ctypes.c_double * 6)(*invert_affine(to_input).reshape(-1))
        mean = (ctypes.c_float * 3)(*[float(v) for v in self.mean.reshape(-1)])
        std = (ctypes.c_float * 3)(*[float(v) for v in self.std.reshape(-1)])
        native.check(lib.cn_warp_normalize_u8_f32(native.ptr(frame), g.scaled_h, g.scaled_w,
                                                  g.scaled_w * 3, dst_to_src, g.inp_h, g.inp_w,
                                                  mean, std, int(self.opt.flip_test),
                                                  native.ptr(out), stream),
                     "cn_warp_normalize_u8_f32")
        return out, self._meta(g)

    # ------------------------------------------------------------------ task hooks
    def process(self, images, return_time=False):
        raise NotImplementedError

    def post_process(self, dets, meta, scale=1):
        raise NotImplementedError

    def merge_outputs(self, detections):
        raise NotImplementedError

    def _no_debugger(self):
        # the reference's Debugger (utils/debugger.py: cv2 / matplotlib windows) is outside the hot
        # path and not built: --debug >= 1 runs the detector as --debug 0 does and says so once
        if not self.__dict__.get("_debug_warned"):
            self.__dict__["_debug_warned"] = True
            import warnings
            warnings.warn("--debug %d: visual debugging is not part of centernet_amd; results are "
                          "computed and returned as with --debug 0" % self.opt.debug)

    def debug(self, debugger, images, dets, output, scale=1):
        self._no_debugger()

    def show_results(self, debugger, image, results):
        self._no_debugger()

    # ------------------------------------------------------------------ run
    @staticmethod
    def _read_bgr(path):
        from PIL import Image  # cv2.imread replacement: BGR uint8
        rgb = np.asarray(Image.open(path).convert('RGB'))
        return np.ascontiguousarray(rgb[:, :, ::-1])

    def _inputs_for_scale(self, image, prefetched, scale, meta):
        """(images on the device, meta) of one test scale."""
        if prefetched is not None:   # test.py's PrefetchDataset dict (base_detector.py:104-110)
            meta = {k: v.numpy()[0] for k, v in prefetched['meta'][scale].items()}
            return prefetched['images'][scale][0].to(self.opt.device), meta
        on_device = getattr(self.opt.device, 'type', str(self.opt.device)) == 'cuda'
        if on_device and image.dtype == np.uint8 and not getattr(self.opt, 'host_pre_process', False):
            return self.pre_process_device(image, scale, meta)
        images, meta = self.pre_process(image, scale, meta)
        return images.to(self.opt.device), meta

    def results_batch(self, dets, metas, scale):
        """Host tail of ``run_frames`` (task specific): host array of raw detections + the
        frames' metas -> what ``run(frame)['results']`` returns, per image."""
        raise NotImplementedError

    # the task's result rows are nested lists, and its host tail (results_batch, merge_outputs) takes
    # ``arrays=True`` to return them as float32 arrays instead
    _list_results = False

    def _arrays_kw(self, arrays):
        return {"arrays": True} if arrays and self._list_results else {}

    def _run_scale(self, images, flip, rects=None):
        """Task hook of the frame pipeline: network + (with ``flip``: the batched flip average of the
        (2B, 3, H, W) frame / mirror pairs) + decode of one test scale -> raw (B, K, .) detections in
        output-grid units, asynchronously (as ``run_batch``).  ``rects``: the rectangles of a canvas batch
        (tasks with ``_canvas_task``), handed to the network as they are."""
        raise NotImplementedError

    def _results_merged(self, per_scale, **kw):
        """Host tail of a merging frame pipeline: ``per_scale`` = [(host raw detections (n, K, .),
        metas, scale)] in test-scale order -> per image ``merge_outputs([post_process(...) per
        scale])``, what ``run(frame)['results']`` returns (``kw``: ``_arrays_kw``)."""
        posts = [self._post_batch(d, metas, scale) for d, metas, scale in per_scale]
        return [self.merge_outputs([p[i] for p in posts], **kw) for i in range(len(posts[0]))]

    def _post_batch(self, dets, metas, scale):
        """``post_process`` of every image of a host batch of raw detections (task specific)."""
        raise NotImplementedError

    def _forward_checked(self, batch, flip):
        """``_run_scale`` of one batch with the f32s range words looked at: the raw detections on the host; after
        a clamped value the network is re-calibrated on this batch and run once more."""
        dets = self._run_scale(batch, flip).detach().cpu().numpy()
        if not self.range_ok(batch):
            dets = self._run_scale(batch, flip).detach().cpu().numpy()
            if not self.range_ok(batch):
                raise native.NativeError("f32s forward clamps values after re-calibration")
        return dets

    def _run_frames_sync(self, frames, scales, **kw):
        """One batch, synchronously, frame by frame through ``pre_process_device`` at every test scale
        (the comparison path of the pipeline, and its re-run path after an f32s re-calibration)."""
        uploaded = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(self.opt.device)
        return self._run_uploaded_sync(uploaded, scales, **kw)

    def _run_images_sync(self, images, scales, **kw):
        """``_run_frames_sync`` for images of any sizes in the fixed-resolution mode (every image gives the same
        network input size): each image uploaded on its own, pre-processed into its slice of the batch, with
        its own meta."""
        return self._run_uploaded_sync([self._device_frame(f) for f in images], scales, **kw)

    def _run_images_sync_keep_res(self, images, scales, **kw):
        """``_run_images_sync`` under --keep_res, where every image has its own network input size: each image
        through its own single-image forward at every test scale, host tail (the comparison path of the canvas
        pipe, and its re-run path after an f32s re-calibration)."""
        return [self._run_uploaded_sync([self._device_frame(f)], scales, **kw)[0] for f in images]

    def _run_uploaded_sync(self, uploaded, scales, **kw):
        flip = bool(self.opt.flip_test)
        k = 2 if flip else 1
        per_scale = []
        for scale in scales:
            g = self.input_geometry(int(uploaded[0].shape[0]), int(uploaded[0].shape[1]), scale)
            batch = torch.empty((k * len(uploaded), 3, g.inp_h, g.inp_w), device=self.opt.device,
                                dtype=torch.float32)
            metas = [self.pre_process_device(frame, scale, out=batch[k * i:k * i + k])[1]
                     for i, frame in enumerate(uploaded)]
            per_scale.append((self._forward_checked(batch, flip), metas, scale))
        if len(per_scale) == 1 and not getattr(self.opt, "nms", False):
            return self.results_batch(*per_scale[0], **kw)
        return self._results_merged(per_scale, **kw)

    @staticmethod
    def _frames_geometry(frames, pixel_format='bgr'):
        """Argument check of ``run_frames`` / ``run_frames_stream`` (no device needed): (B, H, W) of a batch of
        frames in ``pixel_format``."""
        if check_pixel_format(pixel_format) == 'nv12' and torch.is_tensor(frames):
            if frames.dtype != torch.uint8 or frames.dim() != 3 or frames.shape[0] == 0 or not frames.is_cuda \
                    or not frames.is_contiguous():
                raise ValueError("run_frames takes device-resident NV12 frames as one contiguous "
                                 "(B, H * 3 // 2, W) uint8 HIP tensor")
            return (int(frames.shape[0]),) + nv12_size(tuple(frames.shape[1:]))
        if torch.is_tensor(frames) or len(frames) == 0:
            raise ValueError("run_frames needs a list of frames")
        shapes = {tuple(f.shape) for f in frames}
        if len(shapes) != 1:
            raise ValueError("run_frames needs frames of one size")
        shape, = shapes
        if pixel_format == 'nv12':
            if len(shape) != 2 or any(f.dtype != np.uint8 for f in frames):
                raise ValueError("run_frames with pixel_format='nv12' needs (H * 3 // 2, W) uint8 NV12 frames")
            return (len(frames),) + nv12_size(shape)
        if len(shape) != 3 or shape[2] != 3 or any(f.dtype != np.uint8 for f in frames):
            raise ValueError("run_frames needs (H, W, 3) uint8 BGR frames")
        return len(frames), shape[0], shape[1]

    def _pipe_for(self, frames, depth, pixel_format='bgr'):
        B, H, W = self._frames_geometry(frames, pixel_format)
        flip = bool(self.opt.flip_test)
        scales = self._pipe_scales()
        key = (B, H, W, tuple(scales), flip, bool(getattr(self.opt, "nms", False)), depth, pixel_format)
        pipes = self.__dict__.setdefault("_pipes", {})
        if key not in pipes:
            if len(pipes) >= 4:
                pipes.pop(next(iter(pipes))).pool.shutdown(wait=False)
            pipes[key] = FramePipe(self, B, H, W, scales, flip, depth, pixel_format)
        return pipes[key]

    def _frames_and_side(self, batch):
        """One item of ``run_frames_stream``'s iterable -> (frames, the pipe's side array or None)."""
        return batch, None

    def run_frames(self, frames, arrays=False, pixel_format='bgr'):
        """A list of (H, W, 3) uint8 BGR frames of one size -> list of per-image results, what
        ``run(frame)['results']`` returns for each (every test scale, flip-test and --nms as set).
        The reference's test loop is batch_size = 1 (test.py:60-62); here the frames are uploaded as
        ONE uint8 copy, pre-processed on the device in one launch per test scale straight into one
        batch tensor (with flip-test: frame, mirror, frame, mirror, ...), each scale's batch goes
        through the network + flip average + decode once and through the task's device tail (inverse
        affine; ctdet, exdet: + class grouping) and the device scale merge (exdet: always, and there
        is no flip average -- the mirror image's rows are rows); the host slices the result.
        ``arrays=True``: a task whose rows are nested lists (multi_pose: ``{1: [[39 floats], ...]}``)
        returns them as a float32 array (``{1: (n, 39) ndarray}``, the same bits, a copy of its own)
        and saves the ``.tolist()``.  ctdet returns arrays either way.
        ``pixel_format='nv12'``: the frames as a video decoder delivers them, every frame an (H * 3 // 2, W)
        uint8 array (H rows of luma, then H / 2 rows of interleaved U, V; H and W even).  Half the bytes are
        staged and uploaded, ``cn_nv12_to_bgr_u8_batch`` converts the batch on the device and everything
        behind it is unchanged: the results are those of ``run_frames([image.nv12_to_bgr(f) for f in
        frames])``, bit for bit.  With 'nv12' ``frames`` may also be ONE contiguous (B, H * 3 // 2, W) uint8 HIP
        tensor, what a GPU decoder leaves behind: nothing is staged or uploaded, the converter reads the
        tensor on the current stream -- the caller must not overwrite it before the batch has been collected
        (here: before the call returns).  Any other ``pixel_format`` raises ``ValueError``."""
        pipe = self._pipe_for(frames, 1, pixel_format)
        pipe.submit(0, frames)
        return pipe.collect(0, frames, arrays)

    def run_frames_stream(self, batches, depth=3, arrays=False, pixel_format='bgr'):
        """``run_frames`` over an iterable of batches (lists of frames, all batches of one size and
        frame geometry), pipelined: while batch i is on the device the host stages batch i + 1
        (pinned uint8 copy by a few threads, asynchronous upload on a copy stream) and builds the
        result dictionaries of batch i - 1.  Yields the per-image results batch by batch, in order.
        ``arrays``: as ``run_frames``.  ``pixel_format``: as ``run_frames``, one format for the whole stream
        (a batch in the other format raises ``ValueError``); a device-resident NV12 batch must stay untouched
        until its results have been yielded, i.e. for ``depth`` further batches."""
        check_pixel_format(pixel_format)
        pipe, pending = None, collections.deque()
        n = 0
        for batch in batches:
            frames, side = self._frames_and_side(batch)
            if pipe is None:
                pipe = self._pipe_for(frames, depth, pixel_format)
            elif self._frames_geometry(frames, pixel_format) != (pipe.B, pipe.H, pipe.W):
                raise ValueError("run_frames_stream needs batches of one size, frame geometry and pixel format "
                                 "(%d %s frames of shape %s)" % (pipe.B, pipe.pixel_format, pipe.frame_shape))
            if len(pending) == depth:
                j, fr = pending.popleft()
                yield pipe.collect(j, fr, arrays)
            pipe.submit(n, frames, side)
            pending.append((n, frames))
            n += 1
        while pending:
            j, fr = pending.popleft()
            yield pipe.collect(j, fr, arrays)

    # ------------------------------------------------------------------ images of mixed sizes
    def _fixed_input(self):
        """Whether images of any sizes give ONE network input size, ``run_images``' condition: not with
        --keep_res (a task whose input never follows the image says otherwise: ddd)."""
        return self.opt.fix_res

    def _images_and_side(self, batch):
        """One item of ``run_images_stream``'s iterable -> (images, the pipe's side array or None)."""
        return batch, None

    _canvas_task = False     # the task batches mixed input sizes on a canvas (ctdet, multi_pose)

    def _canvas_batches(self):
        """Whether --keep_res batches of mixed sizes run on a canvas (``ImagePipe`` with ``canvas=True``): the
        task takes rectangles (``_canvas_task``) and the --keep_res option is set."""
        return self._canvas_task and bool(getattr(self.opt, "keep_res", False)) and not self.opt.fix_res

    def _images_one_size(self, images, what):
        """Argument check of ``run_images`` / ``run_images_stream``; True when the images have one size."""
        if len(images) == 0:
            raise ValueError("%s needs at least one image" % what)
        for f in images:
            if not isinstance(f, np.ndarray) or f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
                raise ValueError("%s needs (H, W, 3) uint8 BGR images" % what)
        one = len({f.shape for f in images}) == 1
        if not self._fixed_input() and not one and not self._canvas_batches():
            raise ValueError("%s with --keep_res: images of mixed sizes give network inputs of mixed sizes, which "
                             "one batch cannot hold (drop --keep_res, or batch images of one size)" % what)
        return one

    def _image_pipe_for(self, images, depth, canvas=False, pinned=None):
        flip = bool(self.opt.flip_test)
        scales = self._pipe_scales()
        key = ("images", len(images), tuple(scales), flip, bool(getattr(self.opt, "nms", False)), depth)
        if canvas:
            key += ("canvas", pinned)
        pipes = self.__dict__.setdefault("_pipes", {})
        if key not in pipes:
            if len(pipes) >= 4:
                pipes.pop(next(iter(pipes))).pool.shutdown(wait=False)
            pipes[key] = ImagePipe(self, len(images), scales, flip, depth, canvas, pinned)
        return pipes[key]

    def _canvas_pipe_for(self, images, depth, canvas, what):
        """The canvas pipe of a --keep_res batch; ``canvas``: ``run_images``' argument, checked here against
        the batch (``ImageTables.check_canvas``)."""
        if not self._canvas_batches():
            raise ValueError("%s: canvas= is for --keep_res batches of the ctdet and multi_pose tasks" % what)
        if canvas is not None:
            canvas = ImageTables(self, ()).check_canvas([(int(f.shape[0]), int(f.shape[1])) for f in images], canvas)
        return self._image_pipe_for(images, depth, True, canvas)

    def run_images(self, images, arrays=False, canvas=None):
        """A list of (H_i, W_i, 3) uint8 BGR images of ANY sizes -> list of per-image results, what
        ``run(image)['results']`` returns for each (every test scale, flip-test and --nms as set) -- ``run_frames``
        for a dataset instead of a video.  Fixed-resolution mode: every image is warped into the same network
        input, so the batch is ``run_frames``' batch; the images are packed back to back into ONE uint8 upload
        with a table of per-image descriptors, pre-processed in one launch per test scale (plus one resize
        launch where the scale resizes), and the tail kernels map every image back with its own inverse map.
        With --keep_res the network input follows the image: images of one size go to ``run_frames``; images of
        mixed sizes share, per test scale, a CANVAS -- the maxima of the batch's input heights and widths --
        in which every image's own padded input sits at the origin of its slice, and the network runs a plan
        whose masks keep each image apart from the rest of the canvas (ctdet and multi_pose; the other tasks
        raise ``ValueError`` for mixed sizes).  ``canvas=(h, w)`` pins the canvas of scale 1 -- multiples of
        pad + 1, at least every image's input at scale 1; other test scales take the pinned canvas through the
        images' own rule -- so that a data set runs ONE plan per test scale, one-size batches included; anything
        else raises ``ValueError``.  Without it every new canvas is a new plan (the plans are an LRU of
        ``CN_PLAN_CACHE`` shapes, 8 by default: raise it for a data set of many sizes).
        ``arrays``: as ``run_frames``."""
        one = self._images_one_size(images, "run_images")
        if canvas is None and not self._fixed_input() and one:
            return self.run_frames(images, arrays)
        if canvas is not None or not self._fixed_input():
            pipe = self._canvas_pipe_for(images, 1, canvas, "run_images")
        else:
            pipe = self._image_pipe_for(images, 1)
        pipe.submit(0, images)
        return pipe.collect(0, images, arrays)

    def run_images_stream(self, batches, depth=3, arrays=False, canvas=None):
        """``run_images`` over an iterable of batches (lists of images of any sizes, every batch of one length
        B -- another length raises ``ValueError``), pipelined as ``run_frames_stream``.  Yields the per-image
        results batch by batch, in order.  With --keep_res a task without canvas batches sends every batch to
        ``run_frames`` on its own; ctdet and multi_pose pipeline the mixed-size batches on their canvases
        (``run_images``) and send a one-size batch to ``run_frames`` once the batches before it are out.
        ``canvas``: as ``run_images``, one canvas for the whole stream, one-size batches included; without it
        the stream may see a new canvas, which means a new plan, with every batch (``CN_PLAN_CACHE`` bounds the
        plans kept: raise it for a data set of many sizes, or pin the canvas)."""
        pipe, B, pending, n = None, None, collections.deque(), 0
        for batch in batches:
            images, side = self._images_and_side(batch)
            one = self._images_one_size(images, "run_images_stream")
            if B is None:
                B = len(images)
            elif len(images) != B:
                raise ValueError("run_images_stream needs batches of one length (%d, then %d)" % (B, len(images)))
            keep_res = canvas is not None or not self._fixed_input()
            if keep_res and canvas is None and (one or not self._canvas_batches()):
                while pending:                             # (canvas batches still on the device come first)
                    j, fr = pending.popleft()
                    yield pipe.collect(j, fr, arrays)
                yield self.run_frames(images, arrays)      # (images of one size, or the check above has raised)
                continue
            if keep_res:
                pipe = self._canvas_pipe_for(images, depth, canvas, "run_images_stream")
            elif pipe is None:
                pipe = self._image_pipe_for(images, depth)
            if len(pending) == depth:
                j, fr = pending.popleft()
                yield pipe.collect(j, fr, arrays)
            pipe.submit(n, images, side)
            pending.append((n, images))
            n += 1
        while pending:
            j, fr = pending.popleft()
            yield pipe.collect(j, fr, arrays)

    # ------------------------------------------------------------------ run_batch: deferred heads
    def _deferred_heads(self):
        """Task hook: the heads ``run_batch`` leaves to the decode, which evaluates them at the K decoded
        centres only (a task's ``deferred_*_heads(opt)``); the network side (fp32 compute mode, fusable
        3x3 + 1x1 heads) is the plan builder's decision.  Nothing by default."""
        return ()

    def _sync_deferral(self):
        """Keep the module's mode in step with the options (one may have changed after construction): the
        frame pipe reads the range words of ``plan_for(...)``, which must be the plan that ran."""
        names = self._deferred_heads()
        if names != self.model.deferral():
            self.model.defer_heads(names)

    def _forward_deferred(self, images, probe=None, rects=None):
        """The network of ``run_batch``: the deferred-heads plan where it applies, else the dense one.
        ``probe``: see ``run_batch``; its ``net_events`` are filled here.  ``rects``: see ``run_batch``."""
        self._sync_deferral()
        kw = {} if rects is None else {"rects": rects}
        if probe is None:
            return self.model(images, borrow=True, deferred=True, **kw)[-1]
        probe['net_events'] = []
        return self.model(images, borrow=True, deferred=True, events=probe['net_events'],
                          event_after=probe.get('event_after'), **kw)[-1]

    def _decode_batch(self, out):
        """Task hook: decode of ``_forward_deferred``'s output -- at the cells where the plan deferred heads
        (``out['_deferred']``), else the dense decode; the maps are logits, the sigmoids are in the kernels."""
        raise NotImplementedError

    def run_batch(self, images, probe=None, rects=None):
        """``images`` (B,3,H,W) fp32, already normalised, on the device -> the task's raw (B,K,.)
        detections in output-grid units (device tensor).  Asynchronous: nothing here waits for
        the device, so the f32s range words of the forward are NOT looked at yet -- call
        ``range_ok()`` where the results are consumed (``run_frames`` does; a pipeline checks
        once per synchronisation point, the words accumulate over the forwards in between).
        ``probe``: optional dict for measurement (bench.py): ``event_after`` (set of launch
        indices) in, ``net_events`` (HIP events at those launch boundaries) and ``dec_events``
        (before / after the decode) out.
        ``rects``: a canvas batch (``PlannedModule.forward``): image b is the rectangle ``rects[b]`` =
        (x0, y0, x1, y1) of ``images``, a host (B, 4) integer array with every edge a multiple of pad + 1;
        its detections are those of the image alone, in the output-grid units of the canvas.  ``images`` is
        zeroed outside the rectangles in place."""
        self._note_unchecked_forward()
        with torch.no_grad():
            out = self._forward_deferred(images, probe, rects)
            if probe is None:
                return self._decode_batch(out)
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
            dets = self._decode_batch(out)
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            probe['dec_events'] = (e0, e1)
            return dets

    UNCHECKED_LIMIT = 4096     # run_batch forwards without a look at the range words before a warning

    def _note_unchecked_forward(self):
        """``run_batch`` does not look at the f32s range words (it never synchronises): the caller
        owes a ``range_ok()`` where it consumes results.  A caller that never pays gets told, once."""
        n = self.__dict__.get("_unchecked", 0) + 1
        self.__dict__["_unchecked"] = n
        if n == self.UNCHECKED_LIMIT and self.model.uses_f32s():
            import warnings
            warnings.warn("%d run_batch() forwards without a range_ok() look: a clamped f32s value "
                          "would go unnoticed (call detector.range_ok() where results are consumed)" % n)

    def range_ok(self, images=None):
        """Synchronising look at the f32s range words of every forward since the last look
        (``PlannedModule.range_ok``): False = a value was clamped, those results are invalid and
        the network has been re-calibrated (on ``images`` when given) -- run the batch again."""
        self.__dict__["_unchecked"] = 0
        return self.model.range_ok(images)

    def run(self, image_or_path_or_tensor, meta=None):
        """One image (array, path, or the prefetch dict) through every test scale
        (base_detector.py:82-143, debug == 0 path); returns the results and the time buckets."""
        clock = _PhaseClock()
        prefetched = None
        if isinstance(image_or_path_or_tensor, np.ndarray):
            image = image_or_path_or_tensor
        elif isinstance(image_or_path_or_tensor, str):
            image = self._read_bgr(image_or_path_or_tensor)
        else:
            prefetched = image_or_path_or_tensor
            image = prefetched['image'][0].numpy()
        clock.lap("load", sync=False)

        per_scale = []
        for scale in self.scales:
            images, meta = self._inputs_for_scale(image, prefetched, scale, meta)
            clock.lap("pre")
            output, dets, forward_done = self.process(images, return_time=True)
            clock.lap("net", until=forward_done)   # process() took this stamp after its own sync
            clock.lap("dec")
            if self.opt.debug >= 2:
                self.debug(None, images, dets, output, scale)
            per_scale.append(self.post_process(dets, meta, scale))
            clock.lap("post")
        results = self.merge_outputs(per_scale)
        clock.lap("merge")
        if self.opt.debug >= 1:
            self.show_results(None, image, results)
        out = {'results': results}
        out.update(clock.finish())
        return out
