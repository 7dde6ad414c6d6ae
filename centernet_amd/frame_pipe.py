"""The frame pipe of ``run_frames`` / ``run_frames_stream`` (``FramePipe``) and the base class of a task's
device tail (``DeviceTail``): what runs behind the decode of every test scale, on the launch stream, so
that the host only slices pinned rows.  The task classes (``detectors/*.py``) supply a ``DeviceTail``
subclass each -- the admission test, the kernel calls and the result shape -- through one hook,
``BaseDetector._device_tail(pipe)``."""
import concurrent.futures
import ctypes
import types

import numpy as np
import torch

from . import native
from .image import get_affine_transform, invert_affine


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
        # output grid -> source pixels of every test scale, float64 (2, 3) row-major, on the device
        self.to_source = []
        for lv in pipe.levels:
            m = lv.meta
            t = get_affine_transform(m['c'], m['s'], 0, (m['out_width'], m['out_height']), inv=1)
            self.to_source.append(torch.from_numpy(np.ascontiguousarray(t, np.float64).reshape(-1)).to(self.device))

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
    input map and meta of one test scale) and ``_pipe_pre_process`` (the batched pre-process launch).
    A task with per-frame side inputs (ddd: one 3 x 4 calibration matrix per frame) sets
    ``_pipe_side_shape``: the pipe then keeps ``depth`` pinned (B, *shape) float32 buffers and their device
    copies, ``submit`` takes the batch's side array, uploads it on the copy stream with the frames, and the
    tail reads ``pipe.side_dev[slot]`` / ``pipe.side_host[slot]``."""

    def __init__(self, det, B, H, W, scales, flip, depth):
        opt, dev = det.opt, det.opt.device
        self.det, self.B, self.H, self.W, self.depth = det, B, H, W, depth
        self.scales, self.flip = tuple(scales), bool(flip)
        # merge_outputs does more than pass one scale through: soft-NMS, and a cut of S * K rows
        self.merge = len(self.scales) > 1 or bool(getattr(opt, "nms", False))
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
        self.mean = (ctypes.c_float * 3)(*[float(v) for v in det.mean.reshape(-1)])
        self.std = (ctypes.c_float * 3)(*[float(v) for v in det.std.reshape(-1)])
        self.pinned_in = [torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.np_in = [t.numpy() for t in self.pinned_in]
        self.dev_in = [torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(depth)]
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
        self.tail = det._device_tail(self)
        self.dets_host = None if self.tail is not None else [[None] * len(self.scales) for _ in range(depth)]

    def _stage(self, slot, frames):
        dst = self.np_in[slot]
        n = len(frames)
        step = -(-n // self.pool._max_workers)

        def copy(lo):
            for i in range(lo, min(lo + step, n)):
                np.copyto(dst[i], frames[i])
        list(self.pool.map(copy, range(0, n, step)))

    def submit(self, i, frames, side=None):
        det, lib, B = self.det, native.lib(), self.B
        slot = i % self.depth
        if self.used[slot]:
            self.ev_h2d[slot].synchronize()      # the pinned buffer's previous upload has left it
        self._stage(slot, frames)
        if self.side_pinned is not None:
            self.side_host[slot] = side
            self.side_pinned[slot].numpy()[:len(frames)] = side
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(self.copy_stream):
            if self.used[slot]:
                self.copy_stream.wait_event(self.ev_pre[slot])   # the device copy's previous reader is done
            self.dev_in[slot].copy_(self.pinned_in[slot], non_blocking=True)
            if self.side_pinned is not None:
                if self.used[slot]:
                    self.copy_stream.wait_event(self.ev_done[slot])   # its reader is the tail, not the pre-process
                self.side_dev[slot].copy_(self.side_pinned[slot], non_blocking=True)
            self.ev_h2d[slot].record(self.copy_stream)
        self.used[slot] = True
        cur.wait_event(self.ev_h2d[slot])
        stream = native.stream_ptr()
        for li, lv in enumerate(self.levels):
            g, src = lv.g, self.dev_in[slot]
            if lv.resize:
                for j in range(B):
                    native.check(lib.cn_resize_bilinear_u8(native.ptr(src[j]), g.src_h, g.src_w, g.src_w * 3,
                                                           g.scaled_h, g.scaled_w, native.ptr(lv.scaled[j]), stream),
                                 "cn_resize_bilinear_u8")
                src = lv.scaled
            det._pipe_pre_process(self, lv, src, stream)
            if li == len(self.levels) - 1:
                self.ev_pre[slot].record()
            dets = det._run_scale(lv.batch, self.flip)
            plan = det.model.plan_for(lv.batch.shape[0], g.inp_h, g.inp_w, lv.batch.device)
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
            return det._run_frames_sync(frames, self.scales, **kw)
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
            return det._run_frames_sync(frames, self.scales, **kw)
        if not self.merge:
            return det.results_batch(self.dets_host[slot][0].numpy()[:n], [self.meta] * n, self.scale, **kw)
        return det._results_merged([(d.numpy()[:n], [lv.meta] * n, lv.scale)
                                    for d, lv in zip(self.dets_host[slot], self.levels)], **kw)
