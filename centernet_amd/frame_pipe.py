"""The frame pipe of ``run_frames`` / ``run_frames_stream`` (``FramePipe``), its form for batches of images of
mixed sizes (``ImagePipe`` with ``ImageTables``: ``run_images`` / ``run_images_stream``), its form for frames cut
into overlapping tiles (``TilePipe``: ctdet's ``run_tiles`` / ``run_tiles_stream``) and the base class of a
task's device tail (``DeviceTail``): what runs behind the decode of every test scale, on the launch stream, so
that the host only slices pinned rows.  The task classes (``detectors/*.py``) supply a ``DeviceTail``
subclass each -- the admission test, the kernel calls and the result shape -- through one hook,
``BaseDetector._device_tail(pipe)``, and the pre-process launch through ``_pipe_pre_process`` (frames of one size)
and ``_pipe_pre_process_images`` (mixed sizes); ddd, with its own warp kernels and one matrix per image, runs
through both pipes like the other tasks."""
import concurrent.futures
import ctypes
import types

import numpy as np
import torch

from . import native
from .image import get_affine_transform, invert_affine, nv12_to_bgr


class DeviceTail(object):
    """A task's tail of the frame pipe on the device, for one pipe.  The pipe calls ``run(slot, level, dets)``
    behind the decode of every test scale, ``finish(slot)`` behind the last one and ``results(slot, n)`` when
    the batch is collected.  Written once, here: the per-level inverse maps, the output buffers with their
    ``depth`` pinned copies, the copies out and the class slicing.  ``arrays`` is ``run_frames``' option, set by
    the pipe before ``results``; a task with per-frame side inputs reads ``pipe.side_dev[slot]``."""
    arrays = False

    @classmethod
    def admits(cls, pipe):
        """Whether the tail kernels take this pipe's shapes (what can be told before any batch is seen); the
        task's ``_device_tail`` builds the tail when they do and returns None, the host tail, when not."""
        raise NotImplementedError

    def __init__(self, pipe):
        self.pipe, self.det, self.device = pipe, pipe.det, pipe.det.opt.device
        self.out, self._host = {}, {}
        # output grid -> source pixels of every test scale, float64 (2, 3) row-major, on the device (a pipe of
        # mixed-size images keeps one map per image, per slot, itself: ``source_map``)
        self.to_source = []
        for lv in ([] if pipe.to_source_dev is not None else pipe.levels):
            m = lv.meta
            t = get_affine_transform(m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1)
            self.to_source.append(torch.from_numpy(np.ascontiguousarray(t, np.float64).reshape(-1)).to(self.device))

    def source_map(self, slot, level):
        """(device pointer, per_image) of test scale ``level`` for the post-process kernels: the level's one map,
        or under a pipe of mixed-size images the (B, 6) maps of the batch in ``slot``."""
        per_slot = self.pipe.to_source_dev
        if per_slot is None:
            return native.ptr(self.to_source[level]), 0
        return native.ptr(per_slot[slot][level]), 1

    def output(self, name, shape, dtype):
        """Declare a final buffer: its device tensor (returned, and ``self.out[name]``) and one pinned host
        copy per pipe slot, which ``finish`` fills and ``host`` reads."""
        self.out[name] = torch.empty(shape, device=self.device, dtype=dtype)
        self._host[name] = [torch.empty(shape, dtype=dtype).pin_memory() for _ in range(self.pipe.depth)]
        return self.out[name]

    def host(self, name, slot):
        """The slot's pinned copy of a declared buffer (reused by a later batch: copy what is kept)."""
        return self._host[name][slot]

    def run(self, slot, level, dets):
        """Test scale ``level``: the raw detections of the decode through the task's post-process kernel."""
        raise NotImplementedError

    def finish(self, slot):
        """After the last test scale (a subclass enqueues its merge first): the declared buffers into the
        slot's pinned copies."""
        for name, t in self.out.items():
            self._host[name][slot].copy_(t, non_blocking=True)

    def results(self, slot, n):
        """Per image what ``run(frame)['results']`` returns, or None to hand the batch back to the host tail."""
        raise NotImplementedError

    @staticmethod
    def class_slices(rows, bounds, n, nc):
        """Rows grouped by class and their (., nc + 1) class bounds -> per image ``{class: rows of it}``, classes
        1-based; ``rows``: the caller's own copy (the dictionaries hold views of it)."""
        out = []
        for i in range(n):
            r, bd = rows[i], bounds[i]
            out.append({j + 1: r[bd[j]:bd[j + 1]] for j in range(nc)})
        return out


class FramePipe(object):
    """Persistent resources of ``run_frames`` / ``run_frames_stream`` for one batch geometry
    (B frames of (H, W, 3) uint8, the detector's test scales and flip setting): per test scale the
    input geometry and meta, the resize buffer and the network batch ((B or 2B, 3, h, w): with
    flip-test every frame is followed by its mirror image); ``depth`` sets of a pinned uint8 staging
    buffer, its device copy and pinned result buffers, one copy stream, a few staging threads.

    Per batch: the frames are copied into the pinned buffer by the staging threads (numpy releases
    the GIL), go to the device as ONE asynchronous uint8 copy on the copy stream, and everything
    else -- per test scale the batched device pre-process, network + flip average + decode
    (``_run_scale``) and the task's device tail (``tail.run``: the post-process kernel into the scale's
    slice), then ``tail.finish`` (the scale merge where the task has one to do, and the copies of the
    rows / class bounds into pinned memory) and the copies of the f32s
    range digests into pinned memory -- is enqueued on the launch stream without a single host
    synchronisation.  The host waits for batch i - depth + 1 only when it collects it, i.e. while
    later batches are on the device.  Shapes the tail kernels do not take (``det._device_tail(pipe)``
    returns None, ``pipe.tail is None``) copy the raw detections out and keep the host tail; a tail can
    also hand ONE batch back when only the batch's own data tell that it does not fit (``tail.results``
    returns None: exdet, more positive rows in a frame than the merge kernel holds) -- ``collect`` then
    drains the device, runs that batch through ``_run_frames_sync`` and counts it in ``det.tail_fallbacks``.

    Two more task hooks keep the pipe free of task geometry: ``_pipe_level`` (input geometry, frame ->
    input map and meta of one test scale) and ``_pipe_pre_process`` (the batched pre-process launch;
    ``_pipe_pre_process_images`` is its twin for ``ImagePipe``'s packed images and descriptors).
    A task with per-frame side inputs (ddd: one 3 x 4 calibration matrix per frame) sets
    ``_pipe_side_shape``: the pipe then keeps ``depth`` pinned (B, *shape) float32 buffers and their device
    copies, ``submit`` takes the batch's side array, uploads it on the copy stream with the frames, and the
    tail reads ``pipe.side_dev[slot]`` / ``pipe.side_host[slot]``.

    ``pixel_format='nv12'``: the frames are (H * 3 // 2, W) uint8 NV12, and so are the pinned buffers and their
    device copies (1.5 bytes per pixel staged and uploaded instead of 3).  ``submit`` converts the uploaded
    batch with one ``cn_nv12_to_bgr_u8_batch`` launch on the launch stream into ``self.bgr`` -- ONE (B, H, W, 3)
    buffer per pipe: it is written and read on the launch stream only -- and the levels pre-process that.  The
    converter is then the only reader of the uploaded buffer, so ``ev_pre``, which lets the next upload into
    the slot start, is recorded right behind it.  A batch that is already on the device (one (B, H * 3 // 2, W)
    uint8 HIP tensor) is neither staged nor uploaded: the converter reads it on the current stream.  The
    hand-back routes of ``collect`` convert the batch to BGR (host frames on the host, a device batch on the
    device) and take the synchronous BGR path."""

    to_source_dev = None     # (ImagePipe: per slot the (S, B, 6) output grid -> source maps of its batch)

    pixel_format = 'bgr'
    bgr = None               # ('nv12': the converted batch, (B, H, W, 3) uint8 on the device)

    def __init__(self, det, B, H, W, scales, flip, depth, pixel_format='bgr'):
        dev = det.opt.device
        self._setup(det, B, scales, flip, depth)
        self.H, self.W, self.pixel_format = H, W, pixel_format
        self.frame_shape = (H * 3 // 2, W) if pixel_format == 'nv12' else (H, W, 3)
        self.levels = []
        for scale in self.scales:
            g, to_input, meta = det._pipe_level(H, W, scale)
            resize = (g.scaled_h, g.scaled_w) != (g.src_h, g.src_w)
            self.levels.append(types.SimpleNamespace(
                scale=scale, g=g, resize=resize, meta=meta,
                dst_to_src=(ctypes.c_double * 6)(*invert_affine(to_input).reshape(-1)),
                scaled=torch.empty((B, g.scaled_h, g.scaled_w, 3), dtype=torch.uint8, device=dev) if resize else None,
                batch=torch.empty((B * (2 if self.flip else 1), 3, g.inp_h, g.inp_w), device=dev,
                                  dtype=torch.float32)))
        first = self.levels[0]        # (the single-scale pipe's own names)
        self.scale, self.g, self.meta, self.batch = first.scale, first.g, first.meta, first.batch
        self.pinned_in = [torch.empty((B,) + self.frame_shape, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.np_in = [t.numpy() for t in self.pinned_in]
        self.dev_in = [torch.empty((B,) + self.frame_shape, dtype=torch.uint8, device=dev) for _ in range(depth)]
        if pixel_format == 'nv12':
            self.bgr = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        self._setup_tail()

    def _setup(self, det, B, scales, flip, depth):
        """What does not depend on the frames' geometry: streams, events, digests, staging threads, side input."""
        opt, dev = det.opt, det.opt.device
        self.det, self.B, self.depth = det, B, depth
        self.scales, self.flip = tuple(scales), bool(flip)
        # merge_outputs does more than pass one scale through: soft-NMS, and a cut of S * K rows
        self.merge = len(self.scales) > 1 or bool(getattr(opt, "nms", False))
        self.mean = (ctypes.c_float * 3)(*[float(v) for v in det.mean.reshape(-1)])
        self.std = (ctypes.c_float * 3)(*[float(v) for v in det.std.reshape(-1)])
        self.copy_stream = torch.cuda.Stream()
        self.ev_h2d = [torch.cuda.Event() for _ in range(depth)]
        self.ev_pre = [torch.cuda.Event() for _ in range(depth)]
        self.ev_done = [torch.cuda.Event() for _ in range(depth)]
        self.used = [False] * depth
        # one range digest per test scale: every scale's plan is looked at
        self.digest_host = [torch.zeros((len(self.scales), 2), dtype=torch.int32).pin_memory() for _ in range(depth)]
        self.has_digest = [[False] * len(self.scales) for _ in range(depth)]
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=min(4, B))
        side = det._pipe_side_shape
        self.side_pinned = self.side_dev = None
        self.side_host = [None] * depth      # the batch's side array as given (host tail, f32s re-run)
        if side is not None:
            self.side_pinned = [torch.empty((B,) + tuple(side), dtype=torch.float32).pin_memory() for _ in range(depth)]
            self.side_dev = [torch.empty((B,) + tuple(side), dtype=torch.float32, device=dev) for _ in range(depth)]

    def _setup_tail(self):
        self.tail = self.det._device_tail(self)
        self.dets_host = None if self.tail is not None else [[None] * len(self.scales) for _ in range(self.depth)]

    def _stage(self, slot, frames):
        dst = self.np_in[slot]
        n = len(frames)
        step = -(-n // self.pool._max_workers)

        def copy(lo):
            for i in range(lo, min(lo + step, n)):
                np.copyto(dst[i], frames[i])
        list(self.pool.map(copy, range(0, n, step)))

    def _upload(self, slot):
        """On the copy stream: the staged batch to the device."""
        self.dev_in[slot].copy_(self.pinned_in[slot], non_blocking=True)

    def _pre_process(self, slot, level, stream):
        """On the launch stream: the uploaded batch of ``slot`` -> the batch of test scale ``level``."""
        lv = self.levels[level]
        lib, g, src = native.lib(), lv.g, self.dev_in[slot] if self.bgr is None else self.bgr
        if lv.resize:
            for j in range(self.B):
                native.check(lib.cn_resize_bilinear_u8(native.ptr(src[j]), g.src_h, g.src_w, g.src_w * 3,
                                                       g.scaled_h, g.scaled_w, native.ptr(lv.scaled[j]), stream),
                             "cn_resize_bilinear_u8")
            src = lv.scaled
        self.det._pipe_pre_process(self, lv, src, stream)

    def _metas(self, slot, level, n):
        """The metas of the first ``n`` images of the batch in ``slot`` at test scale ``level`` (host tail)."""
        return [self.levels[level].meta] * n

    def _run_sync(self, frames, **kw):
        """The batch once more, synchronously, host tail: both hand-back routes of ``collect``.  NV12 frames
        are converted first: a device-resident batch on the device, host frames on the host."""
        if self.pixel_format == 'nv12':
            if torch.is_tensor(frames):
                return self.det._run_uploaded_sync(self.det._nv12_to_bgr_device(frames), self.scales, **kw)
            frames = [nv12_to_bgr(f) for f in frames]
        return self.det._run_frames_sync(frames, self.scales, **kw)

    def submit(self, i, frames, side=None):
        det = self.det
        slot = i % self.depth
        resident = torch.is_tensor(frames)       # (NV12 only: the batch is on the device already)
        if self.used[slot]:
            self.ev_h2d[slot].synchronize()      # the pinned buffer's previous upload has left it
        if not resident:
            self._stage(slot, frames)
        if self.side_pinned is not None:
            self.side_host[slot] = side
            self.side_pinned[slot].numpy()[:len(frames)] = side
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(self.copy_stream):
            if not resident:
                if self.used[slot]:
                    self.copy_stream.wait_event(self.ev_pre[slot])   # the device copy's previous reader is done
                self._upload(slot)
            if self.side_pinned is not None:
                if self.used[slot]:
                    self.copy_stream.wait_event(self.ev_done[slot])   # its reader is the tail, not the pre-process
                self.side_dev[slot].copy_(self.side_pinned[slot], non_blocking=True)
            self.ev_h2d[slot].record(self.copy_stream)
        self.used[slot] = True
        cur.wait_event(self.ev_h2d[slot])
        stream = native.stream_ptr()
        if self.bgr is not None:
            det._nv12_to_bgr_device(frames if resident else self.dev_in[slot], self.bgr, stream)
            self.ev_pre[slot].record()           # the converter is the uploaded buffer's only reader
        for li, lv in enumerate(self.levels):
            self._pre_process(slot, li, stream)
            if li == len(self.levels) - 1 and self.bgr is None:
                self.ev_pre[slot].record()
            rects = self._rects(slot, li)
            if rects is None:
                dets = det._run_scale(lv.batch, self.flip)
                plan = det.model.plan_for(lv.batch.shape[0], lv.batch.shape[2], lv.batch.shape[3], lv.batch.device)
            else:
                dets = det._run_scale(lv.batch, self.flip, rects=rects)
                plan = det.model.__dict__["_ran"]        # (the ragged plan, or the ordinary one for a full canvas)
            rs = getattr(plan.b, "range_sum", None) if plan.b.range is not None else None
            self.has_digest[slot][li] = rs is not None
            if rs is not None:
                self.digest_host[slot][li].copy_(rs, non_blocking=True)
            if self.tail is not None:
                self.tail.run(slot, li, dets)
            else:
                dh = self.dets_host[slot]
                dh[li] = torch.empty(dets.shape, dtype=dets.dtype).pin_memory() if dh[li] is None else dh[li]
                dh[li].copy_(dets, non_blocking=True)
        if self.tail is not None:
            self.tail.finish(slot)
        self.ev_done[slot].record()

    def collect(self, i, frames, arrays=False):
        """Results of batch i (waits for it; later batches keep the device busy).  ``arrays``: see
        ``run_frames``."""
        from .engine import F16_MAX_BITS
        det = self.det
        slot = i % self.depth
        kw = det._arrays_kw(arrays)          # options of the host tail: both fallback routes and a pipe without a tail
        if self.side_pinned is not None:
            kw = dict(kw, side=self.side_host[slot])
        self.ev_done[slot].synchronize()
        det.__dict__["_unchecked"] = 0       # (the batch's range digests are looked at right here)
        digest = self.digest_host[slot].tolist()
        if any(has and (int(d[0]) & 0xffffffff) > F16_MAX_BITS for has, d in zip(self.has_digest[slot], digest)):
            # an f32s value was clamped somewhere up to this batch: results invalid.  Drain the
            # device, let the module re-calibrate, and run this batch again synchronously.
            torch.cuda.synchronize()
            det.range_ok(None)
            return self._run_sync(frames, **kw)
        n = len(frames)
        if self.tail is not None:
            self.tail.arrays = bool(arrays)
            results = self.tail.results(slot, n)
            if results is not None:
                return results
            # the batch does not fit the task's device tail (exdet: a frame with more positive rows than
            # the merge kernel holds): drain the device and run this batch again synchronously, host tail
            torch.cuda.synchronize()
            det.tail_fallbacks += 1
            return self._run_sync(frames, **kw)
        return self._host_tail(slot, slice(0, n), kw)

    def _rects(self, slot, level):
        """The canvas rectangles of the batch in ``slot`` at test scale ``level`` (``ImagePipe`` under
        --keep_res), or None: every image fills the batch tensor."""
        return None

    def _host_tail(self, slot, sel, kw):
        """The host tail on the images ``sel`` (a slice) of the raw detections copied out for ``slot``."""
        det = self.det
        if not self.merge:
            return det.results_batch(self.dets_host[slot][0].numpy()[sel], self._metas(slot, 0, sel.stop)[sel],
                                     self.scale, **kw)
        return det._results_merged([(d.numpy()[sel], self._metas(slot, li, sel.stop)[sel], lv.scale)
                                    for li, (d, lv) in enumerate(zip(self.dets_host[slot], self.levels))], **kw)


class ImageTables(object):
    """Host bookkeeping of ``ImagePipe`` (no device needed): per image size the geometry of every test scale, and
    the tables of a batch.  The geometry of an image size -- ``input_geometry``, ``get_affine_transform``,
    ``invert_affine``, ``_meta`` through the task's ``_pipe_level``, what ``run(image)`` computes -- is kept per
    (H, W): a dataset has few distinct sizes, and these calls would otherwise outweigh the batch's time on the
    device."""
    GEOMETRY_CACHE = 8192

    def __init__(self, det, scales):
        self.det, self.scales, self._geometry = det, tuple(scales), {}

    def of(self, H, W):
        """What one (H, W) image needs at every test scale: ``rec`` (S, 2) descriptors without their offsets,
        ``to_source`` (S, 6), ``metas`` [S], ``scaled`` [S] (h, w), ``resize`` [S], ``inp`` [S] (h, w) the
        network input of the image."""
        e = self._geometry.get((H, W))
        if e is not None:
            return e
        if not (0 < H <= 32767 and 0 < W <= 32767):
            raise ValueError("run_images needs images of 1 .. 32767 rows and columns, got %d x %d" % (H, W))
        S = len(self.scales)
        rec = np.zeros((S, 2), native.IMAGE_DESC)
        e = types.SimpleNamespace(rec=rec, to_source=np.zeros((S, 6), np.float64), metas=[], scaled=[], resize=[],
                                  inp=[], nbytes=H * W * 3)
        for l, scale in enumerate(self.scales):
            g, to_input, meta = self.det._pipe_level(H, W, scale)
            if g.scaled_h <= 0 or g.scaled_w <= 0:
                raise ValueError("run_images: a %d x %d image has no pixels at test scale %s" % (H, W, scale))
            src, dst = rec[l, 0], rec[l, 1]
            src['H'], src['W'], src['pitch'] = H, W, 3 * W
            dst['H'], dst['W'], dst['pitch'] = g.scaled_h, g.scaled_w, 3 * g.scaled_w
            dst['dst_to_src'] = invert_affine(to_input).reshape(-1)
            # as cn_resize_bilinear_u8 forms them (Python floats are doubles)
            dst['scale'] = (1.0 / (float(g.scaled_w) / float(W)), 1.0 / (float(g.scaled_h) / float(H)))
            e.to_source[l] = np.asarray(get_affine_transform(meta['c'], meta['s'], 0,
                                                             (meta['out_width'], meta['out_height']), inv=1),
                                        np.float64).reshape(-1)
            e.metas.append(meta)
            e.scaled.append((g.scaled_h, g.scaled_w))
            e.resize.append((g.scaled_h, g.scaled_w) != (H, W))
            e.inp.append((g.inp_h, g.inp_w))
        if len(self._geometry) >= self.GEOMETRY_CACHE:
            self._geometry.clear()
        self._geometry[(H, W)] = e
        return e

    def fill(self, shapes, desc, to_source):
        """Fill the (S, 2, B) descriptor table and the (S, B, 6) map table for images of ``shapes`` [(H, W)]
        packed back to back -> (bytes of the packed images, their byte offsets, per level [metas], per level
        (resize, max scaled h, max scaled w, bytes of the packed scaled images))."""
        S, n = len(self.scales), len(shapes)
        es = [self.of(H, W) for H, W in shapes]
        for j, e in enumerate(es):
            desc[:, :, j] = e.rec
            to_source[:, j] = e.to_source
        sizes = np.array([e.nbytes for e in es], np.uint64)
        offsets = np.cumsum(sizes) - sizes
        desc['offset'][:, :, :n] = offsets
        plan = []
        for l in range(S):
            if not any(e.resize[l] for e in es):
                plan.append((False, 0, 0, 0))
                continue
            sz = np.array([e.scaled[l][0] * e.scaled[l][1] * 3 for e in es], np.uint64)
            desc['offset'][l, 1, :n] = np.cumsum(sz) - sz
            plan.append((True, max(e.scaled[l][0] for e in es), max(e.scaled[l][1] for e in es), int(sz.sum())))
        return int(sizes.sum()), offsets, [[e.metas[l] for e in es] for l in range(S)], plan

    def canvas(self, shapes, pinned=None):
        """--keep_res, where the network input follows the image: per test scale the canvas (h, w) that holds
        the inputs of images of ``shapes`` -- the maxima of their own input sizes, or with ``pinned`` =
        (h, w) (``check_canvas`` has seen it) that canvas, taken through ``input_geometry`` at the scale as
        the largest image it holds is."""
        es = [self.of(H, W) for H, W in shapes]
        if pinned is None:
            return [(max(e.inp[l][0] for e in es), max(e.inp[l][1] for e in es)) for l in range(len(self.scales))]
        out = []
        for scale in self.scales:
            g = self.det.input_geometry(pinned[0] - 1, pinned[1] - 1, scale)
            out.append((g.inp_h, g.inp_w))
        return out

    def check_canvas(self, shapes, canvas):
        """``run_images(canvas=)``: (h, w), both multiples of pad + 1 and at least the network input of every
        image of ``shapes`` at scale 1; ``ValueError`` otherwise.  Returns (h, w) as integers."""
        step = int(self.det.opt.pad) + 1
        try:
            h, w = (int(v) for v in canvas)
        except (TypeError, ValueError):
            raise ValueError("canvas must be (h, w), got %r" % (canvas,))
        if h <= 0 or w <= 0 or h % step or w % step or (h, w) != tuple(canvas):
            raise ValueError("canvas must be positive multiples of pad + 1 = %d, got %r" % (step, tuple(canvas)))
        for H, W in shapes:
            g = self.det.input_geometry(H, W, 1.0)
            if g.inp_h > h or g.inp_w > w:
                raise ValueError("canvas %d x %d is smaller than the %d x %d network input of a %d x %d image"
                                 % (h, w, g.inp_h, g.inp_w, H, W))
        return h, w

    def fill_rects(self, shapes, canvases, flip, rects):
        """Fill the (S, k * B, 4) int32 rectangle table, k = 2 with ``flip``: image i at the origin of the
        scale's canvas, (0, 0, inp_w, inp_h); with ``flip`` entries 2i and 2i + 1 -- that rectangle and its
        mirror image in the canvas, (Wc - inp_w, 0, Wc, inp_h), where ``flip_concat`` puts the mirrored image.
        Entries past the batch's images stay empty (their slices are cleared)."""
        rects[...] = 0
        k = 2 if flip else 1
        for j, (H, W) in enumerate(shapes):
            e = self.of(H, W)
            for l, (hc, wc) in enumerate(canvases):
                h, w = e.inp[l]
                if h > hc or w > wc:
                    raise ValueError("canvas %d x %d does not hold the %d x %d input of a %d x %d image at test "
                                     "scale %s" % (hc, wc, h, w, H, W, self.scales[l]))
                rects[l, k * j] = (0, 0, w, h)
                if flip:
                    rects[l, k * j + 1] = (wc - w, 0, wc, h)


class ImagePipe(FramePipe):
    """``FramePipe`` for batches of B images of ANY sizes (``run_images`` / ``run_images_stream``), in the
    fixed-resolution mode: every image is warped into the same (input_h, input_w) tensor, so the network, the
    decode and the tail see the batches ``FramePipe`` gives them; only the map in and the map out differ per
    image.  Per slot: one pinned uint8 buffer with the images packed back to back and its device copy (byte
    capacities: the first batch sizes them, a larger batch grows them geometrically once the slot's previous
    upload and its readers are done); a pinned (S, 2, B) table of ``cn_image_desc`` -- per test scale the
    source descriptors and the descriptors the warp reads (the scaled images where the level resizes, else
    the sources again, with the image's dst -> src matrix) -- and a pinned (S, B, 6) float64 table of the
    output grid -> source maps, each with its device copy.  All three go up on the copy stream under
    ``FramePipe``'s events.  Per test scale: ``cn_resize_bilinear_u8_ragged`` where at least one image of the
    batch is resized (the others are copied by it), the task's ``_pipe_pre_process_images`` into ``lv.batch``
    (``cn_warp_normalize_u8_f32_ragged``; ddd, whose levels never resize: ``cn_warp_table_u8_f32_ragged``),
    then ``FramePipe``'s own steps, the tail reading the slot's maps (``DeviceTail.source_map``).  A task's
    side array (ddd: the images' matrices) rides as under ``FramePipe``.  The host side of the tables is
    ``ImageTables``.

    ``canvas=True``, the --keep_res form: the network input follows the image, so the images of a
    batch give inputs of several sizes.  Per batch and test scale they share a CANVAS, the maxima of their
    input heights and widths (``pinned``: one canvas for every batch, ``run_images(canvas=)``); the warp writes
    image i's own padded input at the canvas origin of slice i (with flip-test the mirror image of the whole
    canvas into the next slice, so the mirrored image sits at its right edge), and the network runs a ragged
    plan (``PlannedModule.forward(x, rects=...)``) whose masks keep every image apart from what surrounds it.
    ``lv.batch`` is then the tensor of the batch's canvas, out of a small per-level dictionary keyed by
    canvas; a pinned (S, k * B, 4) int32 rectangle table per slot and its device copy ride with the
    descriptors; a pipe without a device tail runs the host tail image by image (every image has its own
    output size)."""

    CANVAS_BATCHES = 4       # batch tensors kept per test scale of a canvas pipe, least recently used first out

    def __init__(self, det, B, scales, flip, depth, canvas=False, pinned=None):
        opt, dev = det.opt, det.opt.device
        self._setup(det, B, scales, flip, depth)
        S, k = len(self.scales), 2 if self.flip else 1
        self.canvas, self.pinned_canvas = bool(canvas), pinned
        meta = {'out_height': opt.input_h // opt.down_ratio, 'out_width': opt.input_w // opt.down_ratio}
        # lv.meta: what all images share (no 'c' / 's'); lv.scaled: the level's packed resized images
        self.levels = [types.SimpleNamespace(
            scale=scale, g=None, meta=None if canvas else meta, scaled=None, batches={},
            batch=None if canvas else torch.empty((B * k, 3, opt.input_h, opt.input_w), device=dev,
                                                  dtype=torch.float32))
            for scale in self.scales]
        self.scale, self.batch = self.scales[0], self.levels[0].batch
        if canvas:
            self.rects_pinned = [torch.zeros((S, k * B, 4), dtype=torch.int32).pin_memory() for _ in range(depth)]
            self.rects_dev = [torch.zeros((S, k * B, 4), dtype=torch.int32, device=dev) for _ in range(depth)]
            self.canvases = [None] * depth       # per slot, per level (h, w)
        self.capacity = [0] * depth
        self.pinned_in, self.np_in, self.dev_in = [None] * depth, [None] * depth, [None] * depth
        self.desc_pinned = [torch.zeros((S * 2 * B * native.IMAGE_DESC.itemsize,), dtype=torch.uint8).pin_memory()
                            for _ in range(depth)]
        self.desc_host = [t.numpy().view(native.IMAGE_DESC).reshape(S, 2, B) for t in self.desc_pinned]
        self.desc_dev = [torch.empty_like(t, device=dev) for t in self.desc_pinned]
        self.to_source_pinned = [torch.zeros((S, B, 6), dtype=torch.float64).pin_memory() for _ in range(depth)]
        self.to_source_dev = [torch.empty((S, B, 6), dtype=torch.float64, device=dev) for _ in range(depth)]
        self.metas = [None] * depth          # per slot [level][image]
        self.plan = [None] * depth           # per slot, per level (resize, max scaled_h, max scaled_w)
        self.nbytes = [0] * depth
        self.tables = ImageTables(det, self.scales)
        self._setup_tail()

    def _grow(self, slot, nbytes):
        """The slot's staging buffers for ``nbytes`` (the caller has waited for ``ev_h2d``)."""
        if self.used[slot]:
            self.ev_pre[slot].synchronize()      # the device copy's last reader, before it is let go
        cap = max(nbytes, 2 * self.capacity[slot])
        self.pinned_in[slot] = torch.empty((cap,), dtype=torch.uint8).pin_memory()
        self.np_in[slot] = self.pinned_in[slot].numpy()
        with torch.cuda.stream(self.copy_stream):    # written on the copy stream: its allocator's block
            self.dev_in[slot] = torch.empty((cap,), dtype=torch.uint8, device=self.det.opt.device)
        self.capacity[slot] = cap

    def _stage(self, slot, frames):
        shapes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        nbytes, offsets, self.metas[slot], self.plan[slot] = self.tables.fill(shapes, self.desc_host[slot],
                                                                         self.to_source_pinned[slot].numpy())
        if nbytes > self.capacity[slot]:
            self._grow(slot, nbytes)
        self.nbytes[slot] = nbytes
        if self.canvas:
            self.canvases[slot] = self.tables.canvas(shapes, self.pinned_canvas)
            self.tables.fill_rects(shapes, self.canvases[slot], self.flip, self.rects_pinned[slot].numpy())
        for lv, (resize, _, _, scaled_bytes) in zip(self.levels, self.plan[slot]):
            # read and written on the launch stream only: its allocator orders a new buffer behind the old one's use
            if resize and (lv.scaled is None or lv.scaled.numel() < scaled_bytes):
                lv.scaled = torch.empty((max(scaled_bytes, 2 * (0 if lv.scaled is None else lv.scaled.numel())),),
                                        dtype=torch.uint8, device=self.det.opt.device)
        dst, n = self.np_in[slot], len(frames)
        step = -(-n // self.pool._max_workers)

        def copy(lo):
            for i in range(lo, min(lo + step, n)):
                (H, W), off = shapes[i], int(offsets[i])
                np.copyto(dst[off:off + H * W * 3].reshape(H, W, 3), frames[i])
        list(self.pool.map(copy, range(0, n, step)))

    def _upload(self, slot):
        n = self.nbytes[slot]
        self.dev_in[slot][:n].copy_(self.pinned_in[slot][:n], non_blocking=True)
        self.desc_dev[slot].copy_(self.desc_pinned[slot], non_blocking=True)
        if self.used[slot]:
            self.copy_stream.wait_event(self.ev_done[slot])      # the maps' reader is the tail, not the pre-process
        self.to_source_dev[slot].copy_(self.to_source_pinned[slot], non_blocking=True)
        if self.canvas:                      # (read by the forwards of every level: behind ``ev_done`` too)
            self.rects_dev[slot].copy_(self.rects_pinned[slot], non_blocking=True)

    def _canvas_batch(self, slot, level):
        """``lv.batch`` for the canvas of the batch in ``slot``: written and read on the launch stream only."""
        lv, (h, w) = self.levels[level], self.canvases[slot][level]
        t = lv.batches.pop((h, w), None)
        if t is None:
            while len(lv.batches) >= self.CANVAS_BATCHES:
                lv.batches.pop(next(iter(lv.batches)))
            t = torch.empty((self.B * (2 if self.flip else 1), 3, h, w), device=self.det.opt.device,
                            dtype=torch.float32)
        lv.batches[(h, w)] = t
        lv.batch = t
        if level == 0:
            self.batch = t

    def _rects(self, slot, level):
        if not self.canvas:
            return None
        from .engine import CanvasRects
        return CanvasRects(self.rects_pinned[slot][level].numpy(), self.rects_dev[slot][level], not self.flip)

    def _host_tail(self, slot, sel, kw):
        if not self.canvas:
            return super(ImagePipe, self)._host_tail(slot, sel, kw)
        out = []
        for i in range(sel.start, sel.stop):     # every image has its own output size: a batch of one each
            out += super(ImagePipe, self)._host_tail(slot, slice(i, i + 1), kw)
        return out

    def _pre_process(self, slot, level, stream):
        lib, B, lv = native.lib(), self.B, self.levels[level]
        if self.canvas:
            self._canvas_batch(slot, level)
        item = native.IMAGE_DESC.itemsize
        descs = self.desc_dev[slot].data_ptr() + level * 2 * B * item
        src = self.dev_in[slot]
        resize, max_h, max_w, _ = self.plan[slot][level]
        if resize:
            native.check(lib.cn_resize_bilinear_u8_ragged(native.ptr(src), ctypes.c_void_p(descs), native.ptr(lv.scaled),
                                                          ctypes.c_void_p(descs + B * item), B, max_h, max_w, stream),
                         "cn_resize_bilinear_u8_ragged")
            src = lv.scaled
        self.det._pipe_pre_process_images(self, lv, src, ctypes.c_void_p(descs + B * item), stream)

    def _metas(self, slot, level, n):
        return self.metas[slot][level][:n]

    def _run_sync(self, frames, **kw):
        if self.canvas:
            return self.det._run_images_sync_keep_res(frames, self.scales, **kw)
        return self.det._run_images_sync(frames, self.scales, **kw)


class TilePipe(FramePipe):
    """``FramePipe`` for frames much larger than the network input (``run_tiles`` / ``run_tiles_stream``, ctdet and
    multi_pose): the B frames of (H, W) are cut into T overlapping (input_h, input_w) tiles each at native
    resolution (``tiles.tile_grid``), tile t of frame b is image b * T + t of the TILE BATCH, and the pipe's
    levels are the chunks of ``C = min(tile_batch, B * T)`` tiles of that batch, not test scales: every chunk
    runs the ONE plan of batch C, a short last chunk padded to C in a batch tensor of its own whose surplus
    slices are zero from the start and whose surplus rows nobody reads.  Static on the device: one
    ``cn_image_desc`` per tile, all of a frame's pointing into that frame with the tile's own matrix, so a
    chunk's pre-process is one ``cn_warp_normalize_u8_f32_ragged`` launch on its slice of the table (with ctdet's
    ``levels`` the table is ``tiles.pyramid_grid``'s: ``cn_tile_box_desc``, ``cn_tile_box_normalize_u8_f32``, and a
    (T, 2) gate table beside the cores for ``cn_ctdet_tiles_merge_gated_f32``: DESIGN.md 3.6d); the
    (B * T, 6) output grid -> frame maps; the (T, 4) cores.  The tail (``TilesTail``) post-processes each chunk
    into its slice of the (B * T, K, 5) rows and merges the frames' tiles behind the last chunk
    (``cn_ctdet_tiles_merge_f32``); multi_pose: ``PoseTilesTail``, 39-column rows, ``cn_multi_pose_tiles_merge_f32``.
    The pipe is task-neutral: it calls ``det._tiles_tail``, ``det._tiles_host_tail`` and ``det._run_tiles_sync`` and
    hands them ``options``, the task's arguments beyond ``max_per_frame``.  Range digests, staging, the copy stream,
    NV12 and both hand-back routes are ``FramePipe``'s; the synchronous path is ``det._run_tiles_sync``."""

    def __init__(self, det, B, H, W, overlap, margin, tile_batch, max_per_frame, depth, pixel_format='bgr',
                 options=None):
        from .tiles import tile_maps
        # the task's own, beyond max_per_frame (multi_pose: min_score; ctdet: levels, size_gate, gate_slack)
        self.options = dict(options or {})
        self.pyramid = self.options.get('levels')          # the listed levels of a tile pyramid, or None
        opt, dev = det.opt, det.opt.device
        if not (0 < H <= 32767 and 0 < W <= 32767):
            raise ValueError("run_tiles needs frames of 1 .. 32767 rows and columns, got %d x %d" % (H, W))
        th, tw = int(opt.input_h), int(opt.input_w)
        self.grid = grid = det._tiles_grid(H, W, overlap, margin, self.options)
        self.overlap, self.margin, self.tile_batch = overlap, margin, int(tile_batch)
        self.max_per_frame = int(max_per_frame)
        self.T, self.N = grid.T, B * grid.T
        self.C = C = min(self.tile_batch, self.N)
        chunks = [(lo, min(lo + C, self.N)) for lo in range(0, self.N, C)]
        self._setup(det, B, (1.0,) * len(chunks), False, depth)      # one digest per level, i.e. per chunk
        self.H, self.W, self.pixel_format = H, W, pixel_format
        self.frame_shape = (H * 3 // 2, W) if pixel_format == 'nv12' else (H, W, 3)
        self.gates_dev = None
        if self.pyramid is None:
            metas, dst_to_src, to_source = tile_maps(grid, opt.down_ratio)
            desc = np.zeros((self.N,), native.IMAGE_DESC)
        else:            # cn_tile_box_desc per tile (its level and origin), one size gate per tile
            metas, to_source = grid.metas, grid.to_source
            desc = np.zeros((self.N,), native.TILE_BOX_DESC)
            self.gates_dev = torch.from_numpy(np.ascontiguousarray(grid.gates)).to(dev)
        self.tile_metas = metas * B                                  # image b * T + t
        for b in range(B):
            d = desc[b * grid.T:(b + 1) * grid.T]
            d['offset'], d['H'], d['W'], d['pitch'] = b * H * W * 3, H, W, 3 * W
            if self.pyramid is None:
                d['dst_to_src'] = dst_to_src
            else:
                d['level'] = grid.level
                d['y0'], d['x0'] = [o[0] for o in grid.origins], [o[1] for o in grid.origins]
        self.desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
        # (not per slot as ``ImagePipe``'s: the maps of a tile pipe never change; the tail addresses its chunk)
        self.to_source_dev = torch.from_numpy(np.ascontiguousarray(np.tile(to_source, (B, 1)))).to(dev)
        self.cores_dev = torch.from_numpy(np.ascontiguousarray(grid.cores)).to(dev)
        shared = torch.empty((C, 3, th, tw), device=dev, dtype=torch.float32)
        self.levels = []
        for lo, hi in chunks:
            short = hi - lo < C
            self.levels.append(types.SimpleNamespace(
                scale=1.0, g=None, meta=None, lo=lo, hi=hi, n=hi - lo,
                batch=torch.zeros((C, 3, th, tw), device=dev, dtype=torch.float32) if short else shared))
        self.scale, self.batch = 1.0, self.levels[0].batch
        self.pinned_in = [torch.empty((B,) + self.frame_shape, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.np_in = [t.numpy() for t in self.pinned_in]
        self.dev_in = [torch.empty((B,) + self.frame_shape, dtype=torch.uint8, device=dev) for _ in range(depth)]
        if pixel_format == 'nv12':
            self.bgr = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        self._setup_tail()

    def _setup_tail(self):
        self.tail = self.det._tiles_tail(self)
        self.dets_host = None if self.tail is not None else [[None] * len(self.levels) for _ in range(self.depth)]

    def _pre_process(self, slot, level, stream):
        """On the launch stream: the tiles of chunk ``level`` out of the uploaded frames, one launch."""
        lv = self.levels[level]
        src = self.dev_in[slot] if self.bgr is None else self.bgr
        if self.pyramid is not None:     # (a chunk may span levels: the level is the tile's)
            descs = ctypes.c_void_p(self.desc_dev.data_ptr() + lv.lo * native.TILE_BOX_DESC.itemsize)
            native.check(native.lib().cn_tile_box_normalize_u8_f32(
                native.ptr(src), descs, lv.n, int(lv.batch.shape[2]), int(lv.batch.shape[3]), self.mean, self.std,
                native.ptr(lv.batch), stream), "cn_tile_box_normalize_u8_f32")
            return
        descs = ctypes.c_void_p(self.desc_dev.data_ptr() + lv.lo * native.IMAGE_DESC.itemsize)
        native.check(native.lib().cn_warp_normalize_u8_f32_ragged(
            native.ptr(src), descs, lv.n, int(lv.batch.shape[2]), int(lv.batch.shape[3]), self.mean, self.std, 0,
            native.ptr(lv.batch), stream), "cn_warp_normalize_u8_f32_ragged")

    def _run_sync(self, frames, **kw):
        if self.pixel_format == 'nv12':
            frames = [nv12_to_bgr(f) for f in frames]
        return self.det._run_tiles_sync(frames, self.overlap, self.margin, self.tile_batch, self.max_per_frame,
                                        **dict(self.options, **kw))

    def _host_tail(self, slot, sel, kw):
        """A pipe without a device tail: the host tile merge on the raw detections copied out per chunk."""
        dets = np.concatenate([d.numpy()[:lv.n] for d, lv in zip(self.dets_host[slot], self.levels)], axis=0)
        return self.det._tiles_host_tail(dets, self.grid, self.B, self.max_per_frame, **dict(self.options, **kw))
