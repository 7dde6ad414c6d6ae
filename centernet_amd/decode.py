"""Heat-map decode entry points (mirror of src/lib/models/decode.py), backed by the
fused HIP kernels in csrc/cn_decode.hip (the top-K forms and their one route),
csrc/cn_decode_large.hip (``ctdet_decode`` and ``_topk`` with 128 < K <= 1024) and
csrc/cn_decode_tasks.hip (pose matching, ddd, exct, agnex).

Same callables, same argument meaning, tensors in / tensor out:
    ctdet_decode(heat, wh, reg=None, cat_spec_wh=False, K=100)      decode.py:464-495
    multi_pose_decode(heat, wh, kps, reg, hm_hp, hp_offset, K)      decode.py:497-571
    ddd_decode(heat, rot, depth, dim, wh, reg, K)                   decode.py:426-462
    ctdet_decode_at_cells / multi_pose_decode_at_cells / ddd_decode_at_cells
                                                                    the same rows from a deferred-heads plan
    _nms / _topk / _topk_channel                                    decode.py:9-15, 92-119
``heat`` is post-sigmoid as in the reference; pass ``apply_sigmoid=True`` with logits
to fuse ``hm.sigmoid_()`` (detectors/ctdet.py:31) into the same pass over the heat-map.
"""
import torch

from . import native

_ws_cache = {}


def _workspace(nbytes, device):
    key = str(device)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 256), device=device, dtype=torch.uint8)
        _ws_cache[key] = ws
    return ws


_own_ws = {}
_verify_state = __import__("os").environ.get("CN_DECODE_VERIFY_STATE") == "1"


def _own_workspace(entry, nbytes, device, shape):
    """A workspace that only `entry` with this shape on this stream ever touches, zeroed once: the
    one-launch image-level decode keeps three state words per image in it, needs them zero on entry
    and leaves them zero on exit (include/centernet_amd.h, CN_DECODE_STATE_CLEAN) -- so the call is
    ONE kernel launch, without the fill the library otherwise puts in front."""
    key = (str(device), entry, torch.cuda.current_stream(device).cuda_stream) + tuple(shape)
    ws = _own_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        if len(_own_ws) >= 32:
            _own_ws.clear()
        ws = torch.zeros(max(int(nbytes), 256), device=device, dtype=torch.uint8)
        _own_ws[key] = ws
    return ws


def _owned_call(entry, cname, lib, shape, flags, device, call):
    """``call(flags, ws) -> return code`` of the library entry ``cname`` on the owned workspace of ``entry``
    for this (B, C, H, W, K), with ``DECODE_STATE_CLEAN`` added to ``flags``.  A failed call may have left the
    image state words dirty: the owned workspaces are dropped, never reused.  ``CN_DECODE_VERIFY_STATE=1``
    (debug): synchronise and look at the state words the kernel promises to leave at zero
    (``cn_decode_state_region``)."""
    ws = _own_workspace(entry, lib.cn_ctdet_decode_workspace_bytes(*shape), device, shape)
    rc = call(flags | native.DECODE_STATE_CLEAN, ws)
    if rc:
        _own_ws.clear()
    native.check(rc, cname)
    if _verify_state:
        import ctypes
        off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        native.check(lib.cn_decode_state_region(*shape, ctypes.byref(off), ctypes.byref(nb)),
                     "cn_decode_state_region")
        words = ws[off.value:off.value + nb.value].view(torch.int32)
        if nb.value and int(words.abs().max().item()) != 0:
            _own_ws.clear()
            raise native.NativeError("%s left its workspace state words dirty" % cname)


def _prep(*ts):
    out = []
    for t in ts:
        if t is None:
            out.append(None)
            continue
        if not t.is_cuda:
            raise native.NativeError("decode needs HIP tensors (got %s); there is no CPU path" % t.device)
        native.require_f32(t)
        out.append(t.contiguous())
    return out


def _expect(name, t, B, C, H, W, device):
    """The decoders read their maps through raw pointers: a map of the wrong size would be a
    silent out-of-bounds device read, where the reference's torch ops raise."""
    if t is None:
        return
    if t.dim() != 4 or tuple(t.shape) != (B, C, H, W):
        raise RuntimeError("%s must have shape %s, got %s" % (name, (B, C, H, W), tuple(t.shape)))
    if t.device != device:
        raise RuntimeError("%s is on %s, the heat-map on %s" % (name, t.device, device))


def _large_k(K):
    """Which image-level top-K a call with this K (already known to fit the map) takes: False = the forms of
    ``cn_ctdet_decode_f32`` / ``cn_topk_f32`` (K <= 128, exactly as ever), True = the large-K form of
    csrc/cn_decode_large.hip (128 < K <= 1024); more raises."""
    if K > native.DECODE_LARGE_MAX_K:
        raise RuntimeError("the image-level top-K takes K <= %d, got K = %d" % (native.DECODE_LARGE_MAX_K, K))
    return K > native.DECODE_MAX_K


def ctdet_decode(heat, wh, reg=None, cat_spec_wh=False, K=100, apply_sigmoid=False,
                 return_inds=False, _debug_flags=0):
    heat, wh, reg = _prep(heat, wh, reg)
    lib = native.lib()
    if heat.dim() != 4:
        raise RuntimeError("heat must be (B, C, H, W)")
    B, C, H, W = heat.shape
    _expect("wh", wh, B, 2 * C if cat_spec_wh else 2, H, W, heat.device)
    _expect("reg", reg, B, 2, H, W, heat.device)
    if K > H * W:
        raise RuntimeError("selected index k out of range")  # torch.topk's error
    large = _large_k(K)
    dets = torch.empty((B, K, 6), device=heat.device, dtype=torch.float32)
    inds = torch.empty((B, K), device=heat.device, dtype=torch.int32)
    flags = int(bool(apply_sigmoid)) | int(_debug_flags)

    def call(flags, ws):
        entry = lib.cn_ctdet_decode_large_f32 if large else lib.cn_ctdet_decode_f32
        return entry(native.ptr(heat), native.ptr(wh), native.ptr(reg), B, C, H, W, K,
                     int(bool(cat_spec_wh)), flags,
                     native.ptr(dets), native.ptr(inds), native.ptr(ws), ws.numel(),
                     native.stream_ptr())
    if large:           # (no state words to keep clean, but the candidate keys cross its two launches: per stream)
        ws = _own_workspace("ctdet_large", lib.cn_ctdet_decode_large_workspace_bytes(B, C, H, W, K), heat.device,
                            (B, C, H, W, K))
        native.check(call(flags, ws), "cn_ctdet_decode_large_f32")
    elif _debug_flags:  # (tests / A-B: a shared workspace, the library fills the state words)
        ws = _workspace(lib.cn_ctdet_decode_workspace_bytes(B, C, H, W, K), heat.device)
        native.check(call(flags, ws), "cn_ctdet_decode_f32")
    else:
        _owned_call("ctdet", "cn_ctdet_decode_f32", lib, (B, C, H, W, K), flags, heat.device, call)
    return (dets, inds.long()) if return_inds else dets


def _topk_f32(lib, heat, B, C, H, W, K, flags, ws, stream, large=False):
    """``cn_topk_f32`` (``large``: ``cn_topk_large_f32``) into fresh (B, K) buffers -> (scores, inds, clses,
    return code)."""
    scores = torch.empty((B, K), device=heat.device, dtype=torch.float32)
    inds = torch.empty((B, K), device=heat.device, dtype=torch.int32)
    clses = torch.empty((B, K), device=heat.device, dtype=torch.int32)
    entry = lib.cn_topk_large_f32 if large else lib.cn_topk_f32
    rc = entry(native.ptr(heat), B, C, H, W, K, flags, native.ptr(scores), native.ptr(inds),
               native.ptr(clses), native.ptr(ws), ws.numel(), stream)
    return scores, inds, clses, rc


def _cells_topk(heat, late, K, apply_sigmoid, maps=()):
    """What the ``*_decode_at_cells`` functions share in front of their heads call, behind their own check of
    the head set: the heat-map and the feature map of ``late`` (an ``engine.DeferredHeads``) must fit each
    other, further dense ``maps`` ((name, tensor or None, channels), ...) the heat-map, and K the map; then the
    image-level top-K with the peak test, ONE launch on an owned workspace (``_own_workspace``).
    Returns (heat, B, C, H, W, scores, inds, clses, stream)."""
    (heat,) = _prep(heat)
    lib = native.lib()
    if heat.dim() != 4:
        raise RuntimeError("heat must be (B, C, H, W)")
    B, C, H, W = heat.shape
    f, dev = late.feat, heat.device
    if (f.B, f.H, f.W) != (B, H, W) or f.nchw or f.fmt not in ("f32s", "f32") or f.t.device != dev:
        raise RuntimeError("the deferred heads' feature map must be an NHWC fp32 / f32s (%d, %d, %d, .) "
                           "activation on the heat-map's device" % (B, H, W))
    for name, t, channels in maps:
        _expect(name, t, B, channels, H, W, dev)
    if K > H * W:
        raise RuntimeError("selected index k out of range")
    st = native.stream_ptr()
    out = []

    def call(flags, ws):
        out[:] = _topk_f32(lib, heat, B, C, H, W, K, flags, ws, st)
        return out.pop()
    _owned_call("topk", "cn_topk_f32", lib, (B, C, H, W, K), int(bool(apply_sigmoid)), dev, call)
    scores, inds, clses = out
    return heat, B, C, H, W, scores, inds, clses, st


def _feat_args(f):
    """The feature ``Act`` as the ``*_heads_at_cells_f32`` entries take it: (pointer, B, H, W, C, pitch,
    dtype, 2^exponent)."""
    s = f.fmt == "f32s"
    return (f.ptr(), f.B, f.H, f.W, f.C, f.pitch, native.DTYPE_F32S if s else native.DTYPE_F32,
            float(2.0 ** f.exp) if s else 1.0)


def _cells_result(dets, inds, vals, return_inds, return_vals):
    """``dets``, or the tuple (dets[, inds as int64][, head values]) the caller asked for."""
    out = (dets,)
    if return_inds:
        out += (inds.long(),)
    if return_vals:
        out += (vals,)
    return out if len(out) > 1 else dets


def ctdet_decode_at_cells(heat, late, K=100, apply_sigmoid=False, return_inds=False, return_vals=False):
    """``ctdet_decode`` without dense ``wh`` / ``reg`` maps: ``late`` is the ``engine.DeferredHeads`` of a
    deferred-heads plan (heads ``('wh',)`` or ``('wh', 'reg')``).  Two launches on the current stream: the
    image-level top-K of ``heat`` (``cn_topk_f32`` with the peak test: the scores, cells and classes of
    ``ctdet_decode``, bit for bit) and ``cn_ctdet_heads_at_cells_f32``, which evaluates the heads at
    those cells in plain fp32 and assembles the (B, K, 6) rows.  ``return_vals``: also the raw head
    values (B, K, 2 * heads)."""
    if late.names not in (("wh",), ("wh", "reg")):
        raise RuntimeError("ctdet_decode_at_cells takes the heads ('wh',) or ('wh', 'reg'), got %r" % (late.names,))
    heat, B, C, H, W, scores, inds, clses, st = _cells_topk(heat, late, K, apply_sigmoid)
    nh = len(late.names)
    dets = torch.empty((B, K, 6), device=heat.device, dtype=torch.float32)
    vals = torch.empty((B, K, 2 * nh), device=heat.device, dtype=torch.float32) if return_vals else None
    rc = native.lib().cn_ctdet_heads_at_cells_f32(
        *_feat_args(late.feat), native.ptr(scores), native.ptr(inds), native.ptr(clses), K,
        native.ptr(late.w1), native.ptr(late.b1), late.hidden, nh, native.ptr(late.w2), native.ptr(late.b2),
        native.ptr(dets), native.ptr(vals), st)
    native.check(rc, "cn_ctdet_heads_at_cells_f32")
    return _cells_result(dets, inds, vals, return_inds, return_vals)


def multi_pose_decode_at_cells(heat, late, hm_hp=None, hp_offset=None, K=100, apply_sigmoid=False,
                               return_inds=False, return_vals=False):
    """``multi_pose_decode`` without dense ``wh`` / ``hps`` / ``reg`` maps: ``late`` is the
    ``engine.DeferredHeads`` of a deferred-heads plan (heads ``('wh', 'hps')`` or ``('wh', 'hps', 'reg')``).
    Three calls on the current stream: the image-level top-K of ``heat`` (``cn_topk_f32``),
    ``cn_multi_pose_heads_at_cells_f32``, which evaluates the heads at those cells in plain fp32 and writes
    the stage-A rows (B, K, 5 + 2J + 1), and -- with ``hm_hp`` -- ``cn_multi_pose_match_f32``, the joint
    candidates and the match of ``multi_pose_decode`` on the dense ``hm_hp`` / ``hp_offset``.
    ``apply_sigmoid``: ``heat`` and ``hm_hp`` hold logits.  ``return_vals``: also the raw head values
    (B, K, 2 + 2J [+ 2]) in head order."""
    if late.names not in (("wh", "hps"), ("wh", "hps", "reg")):
        raise RuntimeError("multi_pose_decode_at_cells takes the heads ('wh', 'hps') or ('wh', 'hps', 'reg'), "
                           "got %r" % (late.names,))
    couts = tuple(late.couts)
    if couts[0] != 2 or couts[1] % 2 or not 2 <= couts[1] <= 34 or couts[2:] not in ((), (2,)):
        raise RuntimeError("multi_pose_decode_at_cells: head outputs %r are not (2, 2J[, 2])" % (couts,))
    J = couts[1] // 2
    hm_hp, hp_offset = _prep(hm_hp, hp_offset)
    heat, B, C, H, W, scores, inds, clses, st = _cells_topk(
        heat, late, K, apply_sigmoid, maps=(("hm_hp", hm_hp, J), ("hp_offset", hp_offset, 2)))
    lib, dev = native.lib(), heat.device
    dets = torch.empty((B, K, 5 + 2 * J + 1), device=dev, dtype=torch.float32)
    vals = torch.empty((B, K, sum(couts)), device=dev, dtype=torch.float32) if return_vals else None
    rc = lib.cn_multi_pose_heads_at_cells_f32(
        *_feat_args(late.feat), native.ptr(scores), native.ptr(inds), native.ptr(clses), K,
        native.ptr(late.w1), native.ptr(late.b1), late.hidden, len(late.names), J, native.ptr(late.w2),
        native.ptr(late.b2), native.ptr(dets), native.ptr(vals), st)
    native.check(rc, "cn_multi_pose_heads_at_cells_f32")
    if hm_hp is not None:
        mws = _workspace(lib.cn_multi_pose_decode_workspace_bytes(B, 1, H, W, J, K), dev)
        rc = lib.cn_multi_pose_match_f32(native.ptr(hm_hp), native.ptr(hp_offset), B, J, H, W, K,
                                         int(bool(apply_sigmoid)), native.ptr(dets), native.ptr(mws),
                                         mws.numel(), st)
        native.check(rc, "cn_multi_pose_match_f32")
    return _cells_result(dets, inds, vals, return_inds, return_vals)


def _topk_channel(scores, K=40, apply_sigmoid=False, nms=False):
    """decode.py:92-101: per-channel top-K -> (scores, inds, ys, xs), each (B, C, K).  With
    ``nms=True`` the 3x3 peak test of ``_nms`` is fused in front (how the reference chains
    them, decode.py:528-533); ``nms=False`` is the plain function on any float map."""
    (scores,) = _prep(scores)
    lib = native.lib()
    B, C, H, W = scores.shape
    if K > H * W:
        raise RuntimeError("selected index k out of range")
    flags = int(bool(apply_sigmoid)) | (0 if nms else native.DECODE_NO_PEAK_TEST)
    s = torch.empty((B, C, K), device=scores.device, dtype=torch.float32)
    i = torch.empty((B, C, K), device=scores.device, dtype=torch.int32)
    nbytes = lib.cn_ctdet_decode_workspace_bytes(B, C, H, W, K)
    ws = _workspace(nbytes, scores.device)
    rc = lib.cn_nms_topk_channel_f32(native.ptr(scores), B, C, H, W, K, flags,
                                     native.ptr(s), native.ptr(i), native.ptr(ws), ws.numel(),
                                     native.stream_ptr())
    native.check(rc, "cn_nms_topk_channel_f32")
    i = i.long()
    ys = (i // W).float()
    xs = (i % W).float()
    return s, i, ys, xs


def multi_pose_decode(heat, wh, kps, reg=None, hm_hp=None, hp_offset=None, K=100,
                      apply_sigmoid=False):
    heat, wh, kps, reg, hm_hp, hp_offset = _prep(heat, wh, kps, reg, hm_hp, hp_offset)
    lib = native.lib()
    if heat.dim() != 4 or kps.dim() != 4 or kps.shape[1] % 2:
        raise RuntimeError("heat must be (B, C, H, W) and kps (B, 2J, H, W)")
    B, C, H, W = heat.shape
    J = kps.shape[1] // 2
    _expect("wh", wh, B, 2, H, W, heat.device)
    _expect("kps", kps, B, 2 * J, H, W, heat.device)
    _expect("reg", reg, B, 2, H, W, heat.device)
    _expect("hm_hp", hm_hp, B, J, H, W, heat.device)
    _expect("hp_offset", hp_offset, B, 2, H, W, heat.device)
    if K > H * W:
        raise RuntimeError("selected index k out of range")
    dets = torch.empty((B, K, 4 + 1 + 2 * J + 1), device=heat.device, dtype=torch.float32)
    nbytes = lib.cn_multi_pose_decode_workspace_bytes(B, C, H, W, J, K)
    ws = _workspace(nbytes, heat.device)
    rc = lib.cn_multi_pose_decode_f32(native.ptr(heat), native.ptr(wh), native.ptr(kps),
                                      native.ptr(reg), native.ptr(hm_hp), native.ptr(hp_offset),
                                      B, C, H, W, J, K, int(bool(apply_sigmoid)), native.ptr(dets),
                                      native.ptr(ws), ws.numel(), native.stream_ptr())
    native.check(rc, "cn_multi_pose_decode_f32")
    return dets


def _topk(scores, K=40, apply_sigmoid=False, nms=False):
    """decode.py:103-119: (scores, inds, clses, ys, xs), each (B, K); ``nms=True`` fuses the
    3x3 peak test of ``_nms`` in front (how the reference chains them), ``nms=False`` is the
    plain function."""
    (scores,) = _prep(scores)
    lib = native.lib()
    B, C, H, W = scores.shape
    if K > H * W:
        raise RuntimeError("selected index k out of range")
    flags = int(bool(apply_sigmoid)) | (0 if nms else native.DECODE_NO_PEAK_TEST)
    large = _large_k(K)
    if large:           # (the candidate keys cross the form's two launches: a workspace per stream)
        ws = _own_workspace("topk_large", lib.cn_ctdet_decode_large_workspace_bytes(B, C, H, W, K), scores.device,
                            (B, C, H, W, K))
    else:
        ws = _workspace(lib.cn_ctdet_decode_workspace_bytes(B, C, H, W, K), scores.device)
    s, i, c, rc = _topk_f32(lib, scores, B, C, H, W, K, flags, ws, native.stream_ptr(), large)
    native.check(rc, "cn_topk_large_f32" if large else "cn_topk_f32")
    i = i.long()
    return s, i, c.int(), (i // W).float(), (i % W).float()


def _transpose_and_gather_feat(feat, ind):
    """models/utils.py:21-26: (B,C,H,W), (B,K) -> (B,K,C), without the full-tensor transpose."""
    (feat,) = _prep(feat)
    lib = native.lib()
    B, C, H, W = feat.shape
    if ind.dim() != 2 or ind.shape[0] != B or ind.device != feat.device:
        raise RuntimeError("ind must be (B, K) on the device of feat")
    K = ind.shape[1]
    if ind.numel() and (int(ind.min()) < 0 or int(ind.max()) >= H * W):   # torch.gather raises
        raise RuntimeError("index out of range for a %dx%d map" % (H, W))
    ind32 = ind.to(torch.int32).contiguous()
    out = torch.empty((B, K, C), device=feat.device, dtype=torch.float32)
    rc = lib.cn_gather_feat_f32(native.ptr(feat), native.ptr(ind32), native.ptr(out), B, C, H, W, K,
                                native.stream_ptr())
    native.check(rc, "cn_gather_feat_f32")
    return out


def ddd_decode(heat, rot, depth, dim, wh=None, reg=None, K=40, apply_sigmoid=False, raw_depth=False):
    """decode.py:426-462 -> (B, K, 16) or (B, K, 18) with wh.  ``raw_depth``: ``depth`` is the head's raw
    map; the K gathered values are transformed (1 / (sigmoid + 1e-6) - 1, detectors/ddd.py:60) in the decode."""
    heat, rot, depth, dim, wh, reg = _prep(heat, rot, depth, dim, wh, reg)
    lib = native.lib()
    B, C, H, W = heat.shape
    if K > H * W:
        raise RuntimeError("selected index k out of range")
    _expect("rot", rot, B, 8, H, W, heat.device)
    _expect("depth", depth, B, 1, H, W, heat.device)
    _expect("dim", dim, B, 3, H, W, heat.device)
    _expect("wh", wh, B, 2, H, W, heat.device)
    _expect("reg", reg, B, 2, H, W, heat.device)
    dets = torch.empty((B, K, 18 if wh is not None else 16), device=heat.device, dtype=torch.float32)
    ws = _workspace(lib.cn_ddd_decode_workspace_bytes(B, C, H, W, K), heat.device)
    rc = lib.cn_ddd_decode_f32(native.ptr(heat), native.ptr(rot), native.ptr(depth), native.ptr(dim),
                               native.ptr(wh), native.ptr(reg), B, C, H, W, K,
                               int(bool(apply_sigmoid)) | (native.DECODE_DDD_RAW_DEPTH if raw_depth else 0),
                               native.ptr(dets), native.ptr(ws), ws.numel(), native.stream_ptr())
    native.check(rc, "cn_ddd_decode_f32")
    return dets


_DDD_HEADS = (("dep", 1), ("rot", 8), ("dim", 3), ("wh", 2), ("reg", 2))


def ddd_decode_at_cells(heat, late, K=40, apply_sigmoid=False, raw_depth=False, return_inds=False,
                        return_vals=False):
    """``ddd_decode`` without dense ``dep`` / ``rot`` / ``dim`` / ``wh`` / ``reg`` maps: ``late`` is the
    ``engine.DeferredHeads`` of a deferred-heads plan with the heads ``('dep', 'rot', 'dim')`` + optional
    ``'wh'`` + optional ``'reg'``, packed per group.  Two launches on the current stream: the image-level top-K
    of ``heat`` (``cn_topk_f32``: the scores, cells and classes of ``ddd_decode``, bit for bit) and
    ``cn_ddd_heads_at_cells_f32``, which evaluates the heads at those cells in plain fp32 and writes the
    (B, K, 18) rows -- (B, K, 16) without ``wh``.  ``raw_depth``: column 11 is 1 / (sigmoid(dep) + 1e-6) - 1 as
    ``ddd_decode(raw_depth=True)`` computes it, else the head's value.  ``return_vals``: also the raw head
    values (B, K, 12 [+ 2] [+ 2]) in head order."""
    names, couts = tuple(late.names), tuple(late.couts)
    has_wh, has_reg = "wh" in names, "reg" in names
    want = [hc for hc in _DDD_HEADS if hc[0] not in ("wh", "reg") or (has_wh if hc[0] == "wh" else has_reg)]
    if names != tuple(n for n, _ in want) or couts != tuple(c for _, c in want):
        raise RuntimeError("ddd_decode_at_cells takes the heads ('dep', 'rot', 'dim'[, 'wh'][, 'reg']) with "
                           "(1, 8, 3[, 2][, 2]) outputs, packed per group; got %r with %r" % (names, couts))
    heat, B, C, H, W, scores, inds, clses, st = _cells_topk(heat, late, K, apply_sigmoid)
    dets = torch.empty((B, K, 18 if has_wh else 16), device=heat.device, dtype=torch.float32)
    vals = torch.empty((B, K, sum(couts)), device=heat.device, dtype=torch.float32) if return_vals else None
    rc = native.lib().cn_ddd_heads_at_cells_f32(
        *_feat_args(late.feat), native.ptr(scores), native.ptr(inds), native.ptr(clses), K,
        late.hidden, len(late.groups), late.group_table(), int(has_wh), int(has_reg),
        native.DECODE_DDD_RAW_DEPTH if raw_depth else 0, native.ptr(dets), native.ptr(vals), st)
    native.check(rc, "cn_ddd_heads_at_cells_f32")
    return _cells_result(dets, inds, vals, return_inds, return_vals)


def agnex_ct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr=None, l_regr=None, b_regr=None,
                    r_regr=None, K=40, scores_thresh=0.1, center_thresh=0.1, aggr_weight=0.0,
                    num_dets=1000, stream=None):
    """decode.py:121-271 -> (B, num_dets, 14): the class-agnostic ``exct_decode`` -- single-channel edge
    maps, the centre map over the classes; groupings are scored against the centre map's per-cell maximum
    and take its arg-max at the box centre as their class (``cn_agnex_ct_decode_f32``; ``stream`` as in
    ``exct_decode``: ``cn_agnex_ct_decode_stream_f32``)."""
    return exct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr, K=K,
                       scores_thresh=scores_thresh, center_thresh=center_thresh, aggr_weight=aggr_weight,
                       num_dets=num_dets, stream=stream, _agnostic=True)


def exct_decode(t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr=None, l_regr=None, b_regr=None,
                r_regr=None, K=40, scores_thresh=0.1, center_thresh=0.1, aggr_weight=0.0,
                num_dets=1000, stream=None, _agnostic=False):
    """decode.py:273-424 -> (B, num_dets, 14).  Heat-maps post-sigmoid (values <= 1).
    ``aggr_weight > 0``: the edge aggregation of decode.py:17-90,136-140 runs in front
    (``cn_exct_aggregate_f32``: rows of t / b, columns of l / r).
    ``stream``: which form groups the K^4 candidates -- False the stored one (``cn_exct_decode_f32``: every
    score written to memory, K <= 64), True the streaming one (``cn_exct_decode_stream_f32``: scores recomputed
    while selecting, K <= 128), None the stored one up to K = 64 and the streaming one above.  Same rows, bit
    for bit, wherever both run."""
    if K > native.EXCT_STREAM_MAX_K:
        raise RuntimeError("exct_decode takes K <= %d (K^4 candidate indices), got K = %d"
                           % (native.EXCT_STREAM_MAX_K, K))
    if stream is None:
        stream = K > native.EXCT_STORED_MAX_K
    form = "_stream" if stream else ""
    t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr = _prep(
        t_heat, l_heat, b_heat, r_heat, ct_heat, t_regr, l_regr, b_regr, r_regr)
    lib = native.lib()
    B, C, H, W = t_heat.shape
    if _agnostic and C != 1:
        raise RuntimeError("agnex_ct_decode takes single-channel edge maps, got %d channels" % C)
    if aggr_weight > 0:
        for name, t in (("l_heat", l_heat), ("b_heat", b_heat), ("r_heat", r_heat)):
            _expect(name, t, B, C, H, W, t_heat.device)
        agg = []
        for t, horizontal in ((t_heat, 1), (l_heat, 0), (b_heat, 1), (r_heat, 0)):
            o = torch.empty_like(t)
            native.check(lib.cn_exct_aggregate_f32(native.ptr(t), native.ptr(o), B, C, H, W, horizontal,
                                                   float(aggr_weight), native.stream_ptr()),
                         "cn_exct_aggregate_f32")
            agg.append(o)
        t_heat, l_heat, b_heat, r_heat = agg
    for name, t in (("l_heat", l_heat), ("b_heat", b_heat), ("r_heat", r_heat)):
        _expect(name, t, B, C, H, W, t_heat.device)
    if _agnostic:
        if ct_heat.dim() != 4 or ct_heat.shape[0] != B or tuple(ct_heat.shape[2:]) != (H, W) or \
                ct_heat.device != t_heat.device:
            raise RuntimeError("ct_heat must be (B, classes, H, W) on the device of the edge maps")
    else:
        _expect("ct_heat", ct_heat, B, C, H, W, t_heat.device)
    for name, t in (("t_regr", t_regr), ("l_regr", l_regr), ("b_regr", b_regr), ("r_regr", r_regr)):
        _expect(name, t, B, 2, H, W, t_heat.device)
    if K > H * W or num_dets > K ** 4:
        raise RuntimeError("selected index k out of range")
    dets = torch.empty((B, num_dets, 14), device=t_heat.device, dtype=torch.float32)
    # aggregated edge maps exceed 1: clamp behind the peak test (decode.py:302-305)
    flags = native.EXCT_CLAMP_ONE if aggr_weight > 0 else 0
    name = ("cn_agnex_ct_decode" if _agnostic else "cn_exct_decode") + form
    Cc = int(ct_heat.shape[1])              # (== C unless class-agnostic)
    ws = _workspace(getattr(lib, name + "_workspace_bytes")(B, Cc, H, W, K), t_heat.device)
    rc = getattr(lib, name + "_f32")(native.ptr(t_heat), native.ptr(l_heat), native.ptr(b_heat),
                                     native.ptr(r_heat), native.ptr(ct_heat), native.ptr(t_regr),
                                     native.ptr(l_regr), native.ptr(b_regr), native.ptr(r_regr), B, Cc, H, W, K,
                                     scores_thresh, center_thresh, num_dets, flags, native.ptr(dets),
                                     native.ptr(ws), ws.numel(), native.stream_ptr())
    native.check(rc, name + "_f32")
    return dets
