"""Canvas batches under --keep_res on the device: the two mask entries against numpy bit for bit, the isolation
of the images of a ragged plan from what surrounds them (exact), the parity of its head maps with the torch
oracle of every image's own forward, and the canvas pipe of run_images / run_images_stream against its host
tail, the single-image path and run_frames."""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from centernet_amd import engine, native, synth
from oracle import net_oracle
from oracle.parity import compare_topk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANVAS = (128, 160)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# 4. cn_mask_rects_f32 / cn_mask_rects_nchw_f32 against numpy, bit for bit
# ------------------------------------------------------------------------------------------------
# left-aligned, full, empty, right-aligned down to ONE kept cell at shift 5, and one with all four margins (at
# shift 5 a single workgroup's rows lie above, inside and below it)
RECTS = np.array([[0, 0, 96, 64], [0, 0, 160, 128], [0, 0, 0, 0], [128, 96, 160, 128], [32, 32, 128, 96]], np.int32)


def _prefilled(shape, seed):
    """NaN and 60000 in a seeded pattern: a cell the kernel should have cleared and did not shows"""
    rng = np.random.RandomState(seed)
    return np.where(rng.rand(*shape) < 0.5, np.float32("nan"), np.float32(60000.0)).astype(np.float32)


def _kept(rects, shift, H, W):
    keep = np.zeros((len(rects), H, W), bool)
    for b, (x0, y0, x1, y1) in enumerate(rects):
        keep[b, min(y0 >> shift, H):min(y1 >> shift, H), min(x0 >> shift, W):min(x1 >> shift, W)] = True
    return keep


@pytest.mark.parametrize("shift", [0, 2, 5])
@pytest.mark.parametrize("C,pitch,c_off", [(27, 32, 0), (64, 64, 0), (32, 96, 32), (16, 16, 0)])
def test_nhwc_mask_equals_numpy(dev, shift, C, pitch, c_off):
    lib = native.lib()
    B, H, W = len(RECTS), CANVAS[0] >> shift, CANVAS[1] >> shift
    host = _prefilled((B, H, W, pitch), 7 * shift + C)
    t, rects = torch.from_numpy(host).to(dev), torch.from_numpy(RECTS).to(dev)
    native.check(lib.cn_mask_rects_f32(native.ptr(t), B, H, W, pitch, c_off, C, native.ptr(rects), shift,
                                       native.stream_ptr()), "cn_mask_rects_f32")
    width = min(-(-C // 32) * 32, pitch - c_off)            # whole 32-channel groups, cut at the pitch
    want = host.copy()
    want[:, :, :, c_off:c_off + width][~_kept(RECTS, shift, H, W)] = 0.0
    got = t.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    if shift == 5:
        assert (H, W) == (4, 5) and _kept(RECTS, shift, H, W)[3].sum() == 1      # the 1 x 1 kept cell
    if pitch == 96:                                          # the neighbouring groups of a concat slice
        assert np.array_equal(_bits(got[..., :32]), _bits(host[..., :32]))
        assert np.array_equal(_bits(got[..., 64:]), _bits(host[..., 64:]))


@pytest.mark.parametrize("shift,C", [(5, 3), (2, 2), (0, 1)])
def test_nchw_mask_equals_numpy(dev, shift, C):
    lib = native.lib()
    B, H, W = len(RECTS), CANVAS[0] >> shift, CANVAS[1] >> shift
    fill = np.float32(-1.0e4)
    host = _prefilled((B, C, H, W), 31 + shift)
    t, rects = torch.from_numpy(host).to(dev), torch.from_numpy(RECTS).to(dev)
    native.check(lib.cn_mask_rects_nchw_f32(native.ptr(t), B, C, H, W, native.ptr(rects), shift, float(fill),
                                            native.stream_ptr()), "cn_mask_rects_nchw_f32")
    want = host.copy()
    want[np.broadcast_to(~_kept(RECTS, shift, H, W)[:, None], want.shape)] = fill
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(want))
    assert shift != 5 or W == 5


def test_mask_entries_refuse_bad_arguments(dev):
    lib = native.lib()
    OK, SHAPE, NULL, ALIGN = native.CN_OK, -1, -5, -6
    t = torch.zeros((2, 4, 5, 64), device=dev)
    rects = torch.tensor([[0, 0, 160, 128], [0, 0, 32, 32]], dtype=torch.int32, device=dev)
    st = native.stream_ptr()

    def nhwc(t=t, r=rects, B=2, H=4, W=5, pitch=64, c_off=0, C=64, shift=5):
        return lib.cn_mask_rects_f32(native.ptr(t), B, H, W, pitch, c_off, C, native.ptr(r), shift, st)
    assert nhwc() == OK
    assert nhwc(t=None) == NULL and nhwc(r=None) == NULL
    assert nhwc(B=0) == SHAPE and nhwc(H=0) == SHAPE and nhwc(W=-1) == SHAPE and nhwc(C=0) == SHAPE
    assert nhwc(pitch=0) == SHAPE and nhwc(c_off=-4) == SHAPE and nhwc(c_off=32, C=64) == SHAPE
    assert nhwc(shift=-1) == SHAPE and nhwc(shift=31) == SHAPE and nhwc(B=65536) == SHAPE
    assert nhwc(pitch=30, C=27) == ALIGN and nhwc(c_off=2, C=32) == ALIGN
    misaligned = ctypes.c_void_p(t.data_ptr() + 4)
    assert lib.cn_mask_rects_f32(misaligned, 2, 4, 4, 64, 0, 64, native.ptr(rects), 5, st) == ALIGN
    n = torch.zeros((2, 3, 4, 5), device=dev)

    def nchw(t=n, r=rects, B=2, C=3, H=4, W=5, shift=5):
        return lib.cn_mask_rects_nchw_f32(native.ptr(t), B, C, H, W, native.ptr(r), shift, -1.0, st)
    assert nchw() == OK
    assert nchw(t=None) == NULL and nchw(r=None) == NULL
    assert nchw(B=0) == SHAPE and nchw(C=0) == SHAPE and nchw(H=0) == SHAPE and nchw(W=0) == SHAPE
    assert nchw(shift=-1) == SHAPE and nchw(B=65536) == SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 5. / 6. the ragged plan: isolation (exact) and parity with the oracle of every image's own forward
# ------------------------------------------------------------------------------------------------
CT_HEADS = {"hm": 80, "wh": 2, "reg": 2}
POSE_HEADS = {"hm": 1, "wh": 2, "hps": 34, "reg": 2, "hm_hp": 17, "hp_offset": 2}
NETS = {"resdcn_18": ("resdcn_18", CT_HEADS), "dla_34": ("dla_34", CT_HEADS), "dla_34_pose": ("dla_34", POSE_HEADS),
        "hourglass": ("hourglass", CT_HEADS)}
# (h, w) of the images of a batch: B = 3 in the 128 x 160 canvas; hourglass (pad + 1 = 128) B = 2 in 256 x 256
SIZES = [(64, 96), (128, 160), (32, 32)]
HG_SIZES = [(128, 256), (256, 128)]
_models, _oracle = {}, {}


def _model(case, dev):
    if case not in _models:
        from centernet_amd.model import create_model
        arch, heads = NETS[case]
        m = create_model(arch, dict(heads), 256 if arch.startswith("dla") else 64)
        synth.fill_state_dict_(m, 317)
        m.max_plans = 32
        _models[case] = m.to(dev).eval()
    return _models[case]


def _geometry(case):
    return (HG_SIZES, (256, 256)) if case == "hourglass" else (SIZES, CANVAS)


def _image(case, i, mirrored, seed=None):
    """Image ``i`` of the batch of ``case`` (``seed``: other contents at its size), or its mirror image"""
    sizes, _ = _geometry(case)
    x = synth.images(1, sizes[i][0], sizes[i][1], seed=20 + (i if seed is None else seed))
    return x.flip(-1).contiguous() if mirrored else x


def _rects(case, right):
    sizes, (hc, wc) = _geometry(case)
    return np.array([[wc - w if right else 0, 0, wc if right else w, h] for h, w in sizes], np.int32)


def _canvas_batch(case, right, fill, order=None):
    """The images of ``case`` in their rectangles (mirrored and right-aligned with ``right``), ``fill`` around"""
    sizes, (hc, wc) = _geometry(case)
    x = torch.full((len(sizes), 3, hc, wc), float(fill))
    for i, (x0, y0, x1, y1) in enumerate(_rects(case, right)):
        x[i, :, y0:y1, x0:x1] = _image(case, i, right, None if order is None else order[i])[0]
    return x


def _forward(m, x, rects, dev):
    with torch.no_grad():
        out = m(x.to(dev), rects=rects, check=False)[-1]
    return {k: v.cpu().numpy() for k, v in out.items()}


def _inside(a, rect):
    x0, y0, x1, y1 = (int(v) >> 2 for v in rect)
    return a[:, y0:y1, x0:x1]


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("case", ["resdcn_18", "dla_34", "dla_34_pose"])
def test_images_of_a_canvas_are_isolated(dev, case, right):
    m, rects = _model(case, dev), _rects(case, right)
    base = _forward(m, _canvas_batch(case, right, 0.0), rects, dev)
    assert (m.plan_for(3, 128, 160, dev, deferred=False, ragged=True, origin=not right).b.origin) is (not right)
    for fill in (float("nan"), 60000.0):
        got = _forward(m, _canvas_batch(case, right, fill), rects, dev)
        for name, ref in base.items():
            for b in range(3):
                assert np.array_equal(_bits(_inside(got[name][b], rects[b])), _bits(_inside(ref[b], rects[b]))), \
                    (name, b, fill)
    # the other two images with each other's contents (at their own sizes): image 0 does not move by a bit
    got = _forward(m, _canvas_batch(case, right, 0.0, order=[0, 2, 1]), rects, dev)
    for name, ref in base.items():
        assert np.array_equal(_bits(_inside(got[name][0], rects[0])), _bits(_inside(ref[0], rects[0]))), name
        assert not np.array_equal(_bits(got[name][1]), _bits(ref[1]))
    for name in engine.HEAT_MAPS:
        if name in base:
            keep = np.zeros(base[name].shape, bool)
            for b in range(3):
                _inside(keep[b], rects[b])[...] = True
            assert (base[name][~keep] == np.float32(engine.HM_FILL)).all() and keep.sum() < keep.size
            assert not (base[name][keep] == np.float32(engine.HM_FILL)).any()


def _report(rec):
    """The measured maxima into profiles/keep_res_canvas_parity.jsonl: one line per (case, alignment), the
    line of an earlier run replaced."""
    path = os.path.join(ROOT, "profiles", "keep_res_canvas_parity.jsonl")
    try:
        lines = [json.loads(l) for l in open(path)] if os.path.exists(path) else []
        lines = [l for l in lines if (l["case"], l["right_aligned"]) != (rec["case"], rec["right_aligned"])]
        with open(path, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines + [rec]))
    except (OSError, ValueError, KeyError):
        pass


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("case", ["resdcn_18", "dla_34", "dla_34_pose", "hourglass"])
def test_canvas_forward_matches_the_oracle_of_every_image(dev, case, right):
    """In-rectangle head maps against ``net_oracle.forward`` of each image's own input (the mirrored image for
    the right-aligned rectangles, where flip-test puts it), at 1e-4 of the map's scale -- tests/test_gpu_net.py's
    bar; the single-image forward of the device is measured against the same oracle and reported with it."""
    m, rects = _model(case, dev), _rects(case, right)
    arch, heads = NETS[case]
    sizes, _ = _geometry(case)
    got = _forward(m, _canvas_batch(case, right, 0.0), rects, dev)
    worst, alone = {}, {}
    for b in range(len(sizes)):
        key = (case, b, right)
        if key not in _oracle:
            ref = net_oracle.forward(arch, m.state_dict(), _image(case, b, right), list(heads))
            _oracle[key] = {k: v.numpy()[0] for k, v in ref.items()}
        with torch.no_grad():
            one = m(_image(case, b, right).to(dev), check=False)[-1]
        for name, ref in _oracle[key].items():
            scale = max(1.0, float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))))
            e = float(np.abs(_inside(got[name][b], rects[b]) - ref).max() / scale)
            worst[name] = max(worst.get(name, 0.0), e)
            alone[name] = max(alone.get(name, 0.0), float(np.abs(one[name][0].cpu().numpy() - ref).max() / scale))
    print("%s right=%s: canvas %r, single image %r" % (case, right, worst, alone))
    _report({"case": case, "right_aligned": right, "canvas_vs_oracle": worst, "single_image_vs_oracle": alone})
    assert max(worst.values()) < 1e-4, worst


# ------------------------------------------------------------------------------------------------
# 7. the canvas pipe
# ------------------------------------------------------------------------------------------------
MIXED = [(40, 70), (64, 64), (33, 100), (95, 31)]          # canvas 96 x 128
LARGER = [(40, 70), (100, 140), (64, 64), (95, 31)]        # canvas 128 x 160
CONFIGS = {"single": (False, (1.0,), False), "flip": (True, (1.0,), False), "flip_scales_nms": (True, (0.75, 1.0), True)}


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _images(seed, shapes=MIXED):
    return [_img(h, w, seed + i) for i, (h, w) in enumerate(shapes)]


def _build(task, args):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task, "--keep_res"] + list(args))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    det.model.max_plans = 64
    return det


@pytest.fixture(scope="module")
def ctdet(dev):
    return _build("ctdet", ["--arch", "resdcn_18"])


@pytest.fixture(scope="module")
def multi_pose(dev):
    # K = 6: the 8 x 16 centre map of the smallest image at scale 0.75 has about 14 peaks, and a top-K that runs
    # out of peaks fills up with zero scores in an order no two map sizes share
    return _build("multi_pose", ["--arch", "dla_34", "--K", "6"])


def _configure(det, config):
    flip, scales, nms = CONFIGS[config]
    det.opt.flip_test, det.opt.nms = bool(flip), bool(nms)
    det.opt.test_scales = det.scales = list(scales)
    det.tail_fallbacks = 0
    return det


def _same(a, b, what=""):
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        assert sorted(ra) == sorted(rb)
        for j in ra:
            x, y = np.asarray(ra[j], np.float32), np.asarray(rb[j], np.float32)
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i, j)


def _host_tail(det, per_scale, i):
    """The host tail of image ``i`` alone on the raw detections ``per_scale`` = [(dets, metas, scale)]"""
    one = [(d[i:i + 1], [metas[i]], scale) for d, metas, scale in per_scale]
    if len(one) == 1 and not det.opt.nms:
        return det.results_batch(*one[0])[0]
    return det._results_merged(one)[0]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("task", ["ctdet", "multi_pose"])
def test_canvas_pipe(dev, request, task, config):
    """(a) the device tail == the host tail on the pipe's own raw detections, bit for bit; (b) the raw detections
    of every image against ``_run_scale`` of that image alone through ``compare_topk``: scores within 1e-4, class
    identical, boxes (and joints) within 1e-4 of the grid scale -- which holds the cell too, a neighbouring cell
    being 1e4 tolerances away -- and at most 5 % of an image's K rows left out as near-ties."""
    det = _configure(request.getfixturevalue(task), config)
    images, n, k = _images(300), len(MIXED), 2 if det.opt.flip_test else 1
    pipe = det._canvas_pipe_for(images, 1, None, "run_images")
    assert pipe.canvas and pipe.tail is not None
    pipe.submit(0, images)
    got = pipe.collect(0, images)
    assert det.tail_fallbacks == 0
    per_scale = []
    for li, lv in enumerate(pipe.levels):
        rects = pipe._rects(0, li)
        assert rects[2] is (not det.opt.flip_test)
        dets = det._run_scale(lv.batch, pipe.flip, rects=rects).detach().cpu().numpy()
        per_scale.append((dets, pipe._metas(0, li, n), lv.scale))
        assert tuple(lv.batch.shape[2:]) == pipe.canvases[0][li]
        for i, im in enumerate(images):
            one, meta = det.pre_process_device(im, lv.scale)
            h, w = one.shape[2:]
            assert torch.equal(lv.batch[k * i, :, :h, :w].view(torch.int32), one[0].view(torch.int32)), (li, i)
            alone = det._run_scale(one, pipe.flip).detach().cpu().numpy()
            D = dets.shape[2]
            r = compare_topk(dets[i:i + 1], alone, box_cols=tuple(range(4)) + tuple(range(5, D - 1)),
                             got_ids=dets[i:i + 1, :, D - 1:].astype(np.int64),
                             ref_ids=alone[:, :, D - 1:].astype(np.int64))
            print("%s %s scale %s image %d: %r" % (task, config, lv.scale, i, r))
            assert r["paired"] >= 0.95, r
    assert det.range_ok()
    _same(got, [_host_tail(det, per_scale, i) for i in range(n)], "host tail on the same detections")
    _same(det.run_images(images), got, "run_images")


def test_stream_over_two_canvases_equals_run_images(dev, ctdet):
    det = _configure(ctdet, "flip")
    batches = [_images(310), _images(320, LARGER), _images(330), _images(340, LARGER[::-1])]
    alone = [det.run_images(b) for b in batches]
    streamed = list(det.run_images_stream(iter(batches), depth=2))
    assert len(streamed) == len(batches)
    for s, a in zip(streamed, alone):
        _same(s, a)
    pipe = det._canvas_pipe_for(batches[0], 2, None, "run_images_stream")
    assert sorted(pipe.levels[0].batches) == [(96, 128), (128, 160)]


def test_pinned_canvas_is_one_plan(dev, ctdet):
    det = _configure(ctdet, "single")
    small, large = _images(350), _images(360, LARGER)
    _same(det.run_images(large, canvas=CANVAS), det.run_images(large), "own maxima == the pinned canvas")
    det.model.drop_plans()
    det.run_images(small, canvas=CANVAS)
    det.run_images(large, canvas=CANVAS)
    ragged = [key for key in det.model.__dict__["_plans"] if "ragged" in key]
    assert len(ragged) == 1 and ragged[0][1:3] == CANVAS, ragged
    det.run_images(small)                                    # its own canvas: another plan
    assert len([key for key in det.model.__dict__["_plans"] if "ragged" in key]) == 2
    with pytest.raises(ValueError, match="canvas"):
        det.run_images(large, canvas=(96, 128))


@pytest.mark.parametrize("task", ["ctdet", "multi_pose"])
def test_one_size_batch_equals_run_frames(dev, request, task):
    det = _configure(request.getfixturevalue(task), "flip")
    frames = _images(370, [(64, 96)] * 3)
    _same(det.run_images(frames), det.run_frames(frames))
    _same(list(det.run_images_stream(iter([frames, _images(380, MIXED[:3]), frames])))[2], det.run_frames(frames))
