"""multi_pose task (public behaviour of src/lib/detectors/multi_pose.py:24-81): centre
heat-map + box size + 17 joint offsets, optional joint heat-maps / sub-pixel offsets, decoded
by the fused ``cn_multi_pose_decode_f32`` kernels (``run_batch``: top-K on ``hm``, the ``wh`` / ``hps`` /
``reg`` heads at the K cells only, ``cn_multi_pose_heads_at_cells_f32``, then the joint match on the dense
``hm_hp`` / ``hp_offset``, ``cn_multi_pose_match_f32``).  New surface: ``run_batch``, ``run_frames`` and ``run_tiles``
(frames much larger than the network input, tiled and merged on the device)."""
import math
import time

import numpy as np
import torch

from .. import native
from ..decode import multi_pose_decode, multi_pose_decode_at_cells
from ..frame_pipe import DeviceTail
from ..post_process import multi_pose_post_process, multi_pose_tiles_results
from ..utils import flip_average, flip_average_batch
from .base_detector import BaseDetector
from .tiles_mixin import TilesMixin

ROW = 39  # [x1, y1, x2, y2, score, 17 x (x, y)]


def deferred_pose_heads(opt):
    """The heads ``run_batch`` leaves to the decode: ``multi_pose_decode`` only gathers ``wh``, ``hps`` (and
    ``reg``) at the K decoded centres (decode.py:506-519), so their dense maps are not computed.  ``hm``,
    ``hm_hp`` and ``hp_offset`` stay dense.  Not with flip-test (the averaged maps are needed) or K > 128; the
    network side (fp32 compute mode, fusable 3x3 + 1x1 heads) is the plan builder's decision."""
    if opt.flip_test or opt.K > 128 or 'wh' not in opt.heads or 'hps' not in opt.heads:
        return ()
    if 'reg' in opt.heads:
        return ('wh', 'hps', 'reg') if opt.reg_offset else ()
    return ('wh', 'hps')


class MultiPoseDetector(TilesMixin, BaseDetector):
    def __init__(self, opt):
        super(MultiPoseDetector, self).__init__(opt)
        self.flip_idx = opt.flip_idx

    def _deferred_heads(self):
        return deferred_pose_heads(self.opt)

    _list_results = True

    def _head_maps(self, out):
        """Post-sigmoid centre map and the optional branches, as the decode expects them."""
        hm = out['hm'].sigmoid_()
        hm_hp = None
        if self.opt.hm_hp:
            hm_hp = out['hm_hp'] if self.opt.mse_loss else out['hm_hp'].sigmoid_()
        reg = out['reg'] if self.opt.reg_offset else None
        hp_offset = out['hp_offset'] if self.opt.reg_hp_offset else None
        return hm, out['wh'], out['hps'], reg, hm_hp, hp_offset

    def _average_flip(self, hm, wh, hps, reg, hm_hp, hp_offset):
        """Flip-test (multi_pose.py:44-55): image 1 of the batch is the mirrored frame; maps are
        averaged after un-mirroring, offsets of the un-mirrored frame are kept."""
        hm = flip_average(hm)
        wh = flip_average(wh)
        hps = flip_average(hps, self.flip_idx, offsets=True)
        if hm_hp is not None:
            hm_hp = flip_average(hm_hp, self.flip_idx)
        reg = None if reg is None else reg[0:1]
        hp_offset = None if hp_offset is None else hp_offset[0:1]
        return hm, wh, hps, reg, hm_hp, hp_offset

    def process(self, images, return_time=False):
        with torch.no_grad():
            torch.cuda.synchronize()
            # consumed before the next run; f32s range words checked here (see CtdetDetector)
            output = self.model(images, borrow=True, check=True)[-1]
            maps = self._head_maps(output)
            torch.cuda.synchronize()
            forward_time = time.time()
            if self.opt.flip_test:
                maps = self._average_flip(*maps)
                output['hm'], output['wh'], output['hps'] = maps[0], maps[1], maps[2]
            hm, wh, hps, reg, hm_hp, hp_offset = maps
            dets = multi_pose_decode(hm, wh, hps, reg=reg, hm_hp=hm_hp, hp_offset=hp_offset,
                                     K=self.opt.K)
        return (output, dets, forward_time) if return_time else (output, dets)

    def _decode_batch(self, o):
        """``run_batch``'s decode -> raw (B,K,40) detections; sigmoids fused into the decode kernels."""
        if self.opt.mse_loss and self.opt.hm_hp:
            raise NotImplementedError("run_batch: mse_loss joint heat-maps are not logits")
        hm_hp = o['hm_hp'] if self.opt.hm_hp else None
        hp_offset = o['hp_offset'] if self.opt.reg_hp_offset else None
        late = o.get('_deferred')
        if late is not None:
            return multi_pose_decode_at_cells(o['hm'], late, hm_hp=hm_hp, hp_offset=hp_offset,
                                              K=self.opt.K, apply_sigmoid=True)
        return multi_pose_decode(o['hm'], o['wh'], o['hps'], reg=o['reg'] if self.opt.reg_offset else None,
                                 hm_hp=hm_hp, hp_offset=hp_offset, K=self.opt.K, apply_sigmoid=True)

    _canvas_task = True

    def _run_scale(self, images, flip, rects=None):
        """One test scale of the frame pipeline: ``run_batch``, or with ``flip`` the (2B, 3, H, W)
        frame / mirror pairs -> network -> batched flip average (sigmoids in the flip kernel, joints
        exchanged, offsets of the un-mirrored frame, as ``process``) -> decode: (B, K, 40).  ``rects``: a canvas
        batch, as ``CtdetDetector._run_scale``."""
        if not flip:
            return self.run_batch(images, rects=rects)
        self._note_unchecked_forward()
        self._sync_deferral()        # flip-test defers nothing: plan_for(...) is then this dense plan
        opt = self.opt
        with torch.no_grad():
            o = self.model(images, borrow=True, **({} if rects is None else {"rects": rects}))[-1]
            hm = flip_average_batch(o['hm'], sigmoid=True)
            wh = flip_average_batch(o['wh'])
            hps = flip_average_batch(o['hps'], self.flip_idx, offsets=True)
            hm_hp = flip_average_batch(o['hm_hp'], self.flip_idx, sigmoid=not opt.mse_loss) if opt.hm_hp else None
            reg = flip_average_batch(o['reg'], first=True) if opt.reg_offset else None
            hp_offset = flip_average_batch(o['hp_offset'], first=True) if opt.reg_hp_offset else None
            return multi_pose_decode(hm, wh, hps, reg=reg, hm_hp=hm_hp, hp_offset=hp_offset, K=opt.K)

    def _post_batch(self, dets, metas, scale):
        """``post_process`` of every image of a (B, K, 40) host array: per image ``{1: (K, 39)}``."""
        per = multi_pose_post_process(dets.copy(), [m['c'] for m in metas], [m['s'] for m in metas],
                                      metas[0]['out_height'], metas[0]['out_width'])
        out = []
        for d in per:
            rows = np.array(d[1], dtype=np.float32).reshape(-1, ROW)
            rows[:, :4] /= scale
            rows[:, 5:] /= scale
            out.append({1: rows})
        return out

    def results_batch(self, dets, metas, scale, arrays=False):
        """Host tail of ``run_frames``: (B, K, 40) host array -> per image ``{1: [[x1, y1, x2,
        y2, score, 17 x (x, y)], ...]}``, i.e. merge_outputs([post_process(...)]) for one scale
        without NMS (multi_pose.py:62-81).  ``arrays``: the same rows as a (K, 39) float32 array."""
        return [{1: d[1] if arrays else d[1].tolist()} for d in self._post_batch(dets, metas, scale)]

    def _device_tail(self, pipe):
        return MultiPoseTail(pipe) if MultiPoseTail.admits(pipe) else None

    def post_process(self, dets, meta, scale=1):
        """Output-grid units -> image coordinates of the unscaled frame (multi_pose.py:62-72)."""
        host = dets.detach().cpu().numpy()
        host = host.reshape(1, -1, host.shape[2])
        per_class = multi_pose_post_process(host.copy(), [meta['c']], [meta['s']],
                                            meta['out_height'], meta['out_width'])[0]
        for cls in range(1, self.num_classes + 1):
            rows = np.array(per_class[cls], dtype=np.float32).reshape(-1, ROW)
            rows[:, :4] /= scale
            rows[:, 5:] /= scale
            per_class[cls] = rows
        return per_class

    def merge_outputs(self, detections, arrays=False):
        """Concatenate the test scales; soft-NMS when asked or when there are several
        (multi_pose.py:74-81).  The person class is the only one.  ``arrays`` (the frame pipeline's
        opt-in): the (n, 39) float32 array instead of its list form."""
        people = np.concatenate([d[1] for d in detections], axis=0).astype(np.float32)
        if self.opt.nms or len(self.opt.test_scales) > 1:
            from ..soft_nms import soft_nms_39
            soft_nms_39(people, Nt=0.5, method=2)
        return {1: people if arrays else people.tolist()}


    # ------------------------------------------------------------------ run_tiles: large frames, tiled
    @staticmethod
    def _tiles_min_score(min_score):
        """``min_score`` of ``run_tiles``: None, or a finite number -> None / float."""
        if min_score is None:
            return None
        if isinstance(min_score, (bool, str, bytes)) or not isinstance(min_score, (int, float, np.integer, np.floating)) \
                or not math.isfinite(min_score):
            raise ValueError("run_tiles: min_score must be a finite number or None, got %r" % (min_score,))
        return float(min_score)

    def _tiles_tail(self, pipe):
        return PoseTilesTail(pipe) if PoseTilesTail.admits(pipe) else None

    def _tiles_host_tail(self, dets, grid, B, max_per_frame, min_score=None, arrays=False):
        """Host tail of ``run_tiles``: (B * T, K, 40) host raw detections of the tile batch -> per frame ``{1:
        rows}`` in frame pixels: ``_post_batch`` with the tile metas, then ``post_process.multi_pose_tiles_results``
        (core filter, ``min_score``, ``merge_outputs``' soft-NMS with tiles for scales, the ``max_per_frame`` cut)."""
        from ..tiles import tile_maps
        metas = tile_maps(grid, self.opt.down_ratio)[0]
        posts = self._post_batch(np.asarray(dets), metas * B, 1.0)
        out = []
        for b in range(B):
            rows = multi_pose_tiles_results([p[1] for p in posts[b * grid.T:(b + 1) * grid.T]], grid.cores,
                                            self.opt.nms, max_per_frame, min_score)[1]
            out.append({1: rows if arrays else rows.tolist()})
        return out

    def run_tiles(self, frames, overlap=None, margin=None, tile_batch=32, max_per_frame=None, pixel_format='bgr',
                  arrays=False, *, min_score=None):
        """``CtdetDetector.run_tiles`` for people in large frames: a list of (H, W, 3) uint8 BGR frames of one
        size -> per frame ``{1: rows}`` in frame pixels, rows [x1, y1, x2, y2, score, 17 x (x, y)] as nested
        lists, or with ``arrays=True`` one (n, 39) float32 array (the ``run_frames`` convention).  Tiling,
        ``overlap``, ``margin``, ``tile_batch``, ``pixel_format`` and the refusals are the ctdet entry's.  The merge
        (``cn_multi_pose_tiles_merge_f32``; ``post_process.multi_pose_tiles_results`` is its specification): a
        tile keeps the people whose box centre lies in its core and, with ``min_score`` (keyword only: a finite
        number, ``ValueError`` otherwise), whose score is at least that; when the frame has more than one tile
        or with ``--nms``, Gaussian soft-NMS over the frame as ``merge_outputs`` runs it over test scales; then
        the ``max_per_frame`` (default ``max_per_image``) best rows, ties included.  A frame with more than
        ``native.POSE_TILES_MAX_ROWS`` survivors sends its batch through the host tail (``tail_fallbacks``):
        ``min_score`` is what keeps a 4K frame's candidates below that.  With one tile per frame and
        ``max_per_frame >= K`` the result is ``run_frames``', bit for bit."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        return self._tiles_run(frames, args, pixel_format, arrays, min_score=self._tiles_min_score(min_score))

    def run_tiles_stream(self, batches, depth=3, overlap=None, margin=None, tile_batch=32, max_per_frame=None,
                         pixel_format='bgr', arrays=False, *, min_score=None):
        """``run_tiles`` over an iterable of batches (lists of frames, all batches of one length and frame
        size), pipelined as ``run_frames_stream``.  Yields the per-frame results batch by batch, in order."""
        args = self._tiles_args(overlap, margin, tile_batch, max_per_frame)
        yield from self._tiles_stream(batches, depth, args, pixel_format, arrays,
                                      min_score=self._tiles_min_score(min_score))


class PoseTilesTail(DeviceTail):
    """The multi_pose tail of ``TilePipe``: per chunk cn_multi_pose_post_process_f32 with one inverse map per tile
    into the chunk's slice of the (B * T, K, 39) tile rows; behind the last chunk cn_multi_pose_tiles_merge_f32:
    final 39-column rows in frame pixels, their count and one status word per frame."""

    @classmethod
    def admits(cls, pipe):
        """Not with more detections per tile or rows per frame than the kernels take."""
        K = pipe.det.opt.K
        return K <= 128 and pipe.T * K <= native.TILES_MAX_ROWS

    def __init__(self, pipe):
        super(PoseTilesTail, self).__init__(pipe)    # (``pipe.to_source_dev`` is set: no per-level maps)
        K, B, T = self.det.opt.K, pipe.B, pipe.T
        self.output('rows', (B, T * K, ROW), torch.float32)
        self.output('counts', (B,), torch.int32)
        self.output('status', (B,), torch.int32)
        self.tile_rows = torch.empty((B * T, K, ROW), device=self.device, dtype=torch.float32)
        self.ws_bytes = int(native.lib().cn_multi_pose_tiles_merge_workspace_bytes(B, T, K))
        self.ws = torch.empty((max(self.ws_bytes, 16),), device=self.device, dtype=torch.uint8)
        min_score = pipe.options.get('min_score')
        self.min_score = float('nan') if min_score is None else float(min_score)     # (NaN: no score test)

    def run(self, slot, level, dets):
        """Chunk ``level``: the raw detections of its tiles -> frame pixels, into its slice."""
        pipe, lv = self.pipe, self.pipe.levels[level]
        dets = dets.contiguous()
        native.check(native.lib().cn_multi_pose_post_process_f32(
            native.ptr(dets), lv.n, self.det.opt.K, native.ptr(pipe.to_source_dev[lv.lo:]), 1, 1.0,
            native.ptr(self.tile_rows[lv.lo:]), native.stream_ptr()), "cn_multi_pose_post_process_f32")

    def finish(self, slot):
        pipe, opt = self.pipe, self.det.opt
        native.check(native.lib().cn_multi_pose_tiles_merge_f32(
            native.ptr(self.tile_rows), pipe.B, pipe.T, opt.K, native.ptr(pipe.cores_dev), int(bool(opt.nms)),
            pipe.max_per_frame, self.min_score, native.ptr(self.out['rows']), native.ptr(self.out['counts']),
            native.ptr(self.out['status']), native.ptr(self.ws), self.ws_bytes, native.stream_ptr()),
            "cn_multi_pose_tiles_merge_f32")
        super(PoseTilesTail, self).finish(slot)

    def results(self, slot, n):
        """Per frame ``{1: rows}``, or None when a frame's status is set: more survivors than the merge holds,
        the batch goes back to the host tail.  Only the counted rows leave the pinned buffer."""
        if self.host('status', slot).numpy().any():
            return None
        rows, counts = self.host('rows', slot).numpy(), self.host('counts', slot).numpy().tolist()
        if self.arrays:
            return [{1: rows[i, :counts[i]].copy()} for i in range(n)]
        return [{1: rows[i, :counts[i]].tolist()} for i in range(n)]


class MultiPoseTail(DeviceTail):
    """cn_multi_pose_post_process_f32 per test scale and, when the pipe merges, cn_multi_pose_merge_f32
    (``merge_outputs`` on the device): final 39-column rows in source pixels."""

    @classmethod
    def admits(cls, pipe):
        """Not with more detections than the kernels take."""
        K = pipe.det.opt.K
        return not (K > 128 or (pipe.merge and len(pipe.scales) * K > native.MERGE_MAX_ROWS))

    def __init__(self, pipe):
        super(MultiPoseTail, self).__init__(pipe)
        K, B, S = self.det.opt.K, pipe.B, len(pipe.scales)
        rows = self.output('rows', (B, S * K if pipe.merge else K, ROW), torch.float32)
        # one slice per test scale; a pipe without a merge has one scale, and its slice is the result
        self.scale_rows = rows[None]
        if pipe.merge:
            self.scale_rows = torch.empty((S, B, K, ROW), device=self.device, dtype=torch.float32)

    def run(self, slot, level, dets):
        """Raw detections -> source pixels / scale, into slice ``level``."""
        pipe = self.pipe
        dets = dets.contiguous()
        native.check(native.lib().cn_multi_pose_post_process_f32(
            native.ptr(dets), pipe.B, self.det.opt.K, *self.source_map(slot, level),
            float(pipe.levels[level].scale), native.ptr(self.scale_rows[level]), native.stream_ptr()),
            "cn_multi_pose_post_process_f32")

    def finish(self, slot):
        pipe, det = self.pipe, self.det
        if pipe.merge:
            native.check(native.lib().cn_multi_pose_merge_f32(
                native.ptr(self.scale_rows), len(pipe.scales), pipe.B, det.opt.K, int(bool(det.opt.nms)),
                native.ptr(self.out['rows']), native.stream_ptr()), "cn_multi_pose_merge_f32")
        super(MultiPoseTail, self).finish(slot)

    def results(self, slot, n):
        """Per image ``{1: rows}``: the rows are final; the host copies them out of the pinned buffer as nested
        lists, or with ``arrays`` as one (S * K, 39) array each."""
        rows = self.host('rows', slot).numpy()[:n]
        if self.arrays:
            rows = rows.copy()
            return [{1: rows[i]} for i in range(n)]
        return [{1: r} for r in rows.tolist()]
