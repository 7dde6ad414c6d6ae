"""Canvas batches under --keep_res in fp16 compute mode (``half_compute()``): ``cn_mask_rects_f16`` against numpy
bit for bit, the masks of every op of the four half plans, the isolation of the images of a ragged half plan
(exact), the parity of its head maps with the torch oracle of every image's own forward (the half-network bar),
and the canvas pipe of ``--fp16 --keep_res`` detectors, on every network family that has a half plan.  Inputs, rectangles and seeds are those of
tests/test_gpu_canvas.py, taken from that module."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from centernet_amd import engine, native, synth
from oracle import net_oracle
from oracle.parity import compare_topk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_f32_tests():
    spec = importlib.util.spec_from_file_location("_canvas_f32_tests", os.path.join(ROOT, "tests", "test_gpu_canvas.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


f32 = _load_f32_tests()          # RECTS, CANVAS, the network cases and the pipe's images: one definition
RECTS, CANVAS = f32.RECTS, f32.CANVAS


def _bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ------------------------------------------------------------------------------------------------
# 1. cn_mask_rects_f16 against numpy, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 2, 5])
@pytest.mark.parametrize("C,pitch,c_off", [(16, 16, 0), (16, 48, 16), (8, 24, 8), (27, 32, 0), (64, 64, 0),
                                           (32, 96, 32)])
def test_half_nhwc_mask_equals_numpy(dev, shift, C, pitch, c_off):
    lib = native.lib()
    B, H, W = len(RECTS), CANVAS[0] >> shift, CANVAS[1] >> shift
    host = f32._prefilled((B, H, W, pitch), 7 * shift + C).astype(np.float16)      # NaN and 60000 are halves
    assert set(np.unique(_bits16(host))) == {0x7E00, 0x7B53}
    t, rects = torch.from_numpy(host).to(dev), torch.from_numpy(RECTS).to(dev)
    native.check(lib.cn_mask_rects_f16(native.ptr(t), B, H, W, pitch, c_off, C, native.ptr(rects), shift,
                                       native.stream_ptr()), "cn_mask_rects_f16")
    width = min(-(-C // 8) * 8, pitch - c_off)              # whole 8-channel groups, cut at the pitch
    want = host.copy()
    want[:, :, :, c_off:c_off + width][~f32._kept(RECTS, shift, H, W)] = 0.0
    got = t.cpu().numpy()
    assert np.array_equal(_bits16(got), _bits16(want))
    cleared = _bits16(got[:, :, :, c_off:c_off + width][~f32._kept(RECTS, shift, H, W)])
    assert cleared.size and (cleared == 0).all()            # +0.0
    if shift == 5:
        assert (H, W) == (4, 5) and f32._kept(RECTS, shift, H, W)[3].sum() == 1      # the 1 x 1 kept cell
    # the neighbouring members of a concatenation slice: (16, 48, 16) is the case whole 32-channel groups would
    # get wrong (channels 32 .. 47 belong to the next member)
    assert np.array_equal(_bits16(got[..., :c_off]), _bits16(host[..., :c_off]))
    assert np.array_equal(_bits16(got[..., c_off + width:]), _bits16(host[..., c_off + width:]))
    assert (C, pitch, c_off) != (16, 48, 16) or width == 16


def test_half_mask_entry_refuses_bad_arguments(dev):
    lib = native.lib()
    OK, SHAPE, NULL, ALIGN = native.CN_OK, -1, -5, -6
    t = torch.zeros((2, 4, 5, 64), device=dev, dtype=torch.float16)
    rects = torch.tensor([[0, 0, 160, 128], [0, 0, 32, 32]], dtype=torch.int32, device=dev)
    st = native.stream_ptr()

    def nhwc(t=t, r=rects, B=2, H=4, W=5, pitch=64, c_off=0, C=64, shift=5):
        return lib.cn_mask_rects_f16(native.ptr(t), B, H, W, pitch, c_off, C, native.ptr(r), shift, st)
    assert nhwc() == OK
    assert nhwc(t=None) == NULL and nhwc(r=None) == NULL
    assert nhwc(B=0) == SHAPE and nhwc(H=0) == SHAPE and nhwc(W=-1) == SHAPE and nhwc(C=0) == SHAPE
    assert nhwc(pitch=0) == SHAPE and nhwc(c_off=-8) == SHAPE and nhwc(c_off=32, C=64) == SHAPE
    assert nhwc(shift=-1) == SHAPE and nhwc(shift=31) == SHAPE and nhwc(B=65536) == SHAPE
    assert nhwc(pitch=60, C=27) == ALIGN and nhwc(c_off=4, C=32) == ALIGN
    assert nhwc(pitch=32, C=27) == OK and nhwc(c_off=8, C=16) == OK
    misaligned = ctypes.c_void_p(t.data_ptr() + 2)
    assert lib.cn_mask_rects_f16(misaligned, 2, 4, 4, 64, 0, 64, native.ptr(rects), 5, st) == ALIGN
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. the ragged half plan: every op masked on the slice it wrote, and isolation (exact)
# ------------------------------------------------------------------------------------------------
_models, _oracle, _spread = {}, {}, {}


def _model(case, dev):
    if case not in _models:
        from centernet_amd.model import create_model
        arch, heads = f32.NETS[case]
        m = create_model(arch, dict(heads), 256 if arch.startswith("dla") else 64)
        synth.fill_state_dict_(m, 317)
        m.max_plans = 32
        _models[case] = m.to(dev).eval().half_compute()
    return _models[case]


def _inside_mask(a, rects, shape_hw):
    """(B, H, W) bool: the cells of activation ``a`` that lie inside the images' rectangles"""
    shift = (shape_hw[0] // a.H).bit_length() - 1
    return torch.from_numpy(f32._kept(rects, shift, a.H, a.W))


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("case", ["resdcn_18", "dla_34", "dla_34_pose", "hourglass"])
def test_every_op_of_a_half_canvas_plan_is_masked(dev, case, right):
    """The walk over the launch list of each half plan: every op that wrote an NHWC activation (the /om offset
    maps aside) is followed by one mask launch; a half activation is described by whole 8-channel groups, so
    its mask clears exactly the slice the op wrote; the members of an in-place concatenation do not overlap;
    and after a forward every such tensor -- ALL channels of its buffer, so a member nobody masked shows --
    is exactly zero outside the rectangles and holds something inside them."""
    m, rects = _model(case, dev), f32._rects(case, right)
    sizes, canvas = f32._geometry(case)
    f32._forward(m, f32._canvas_batch(case, right, 60000.0), rects, dev)
    plan = m.plan_for(len(sizes), canvas[0], canvas[1], dev, deferred=False, ragged=True, origin=not right)
    b = plan.b
    assert b.dtype == torch.float16 and b.ragged and b.origin is (not right)
    trace, seen, kinds = b.trace, {}, set()
    assert trace[0][0] == "mask" and len(trace) == len(b.ops) == len(b.meta)
    for i, (kind, a) in enumerate(trace):
        if a is None or a.nchw:
            continue
        if (a.lid or "").endswith("/om"):
            assert a.fmt == "f32" and a.t.dtype == torch.float32 and trace[i + 1][0] != "mask", (i, kind)
            continue
        kinds.add(kind)
        assert trace[i + 1][0] == "mask" and b.meta[i + 1]["kind"] == "mask", (i, kind)
        assert a.fmt == "f16" and a.t.dtype == torch.float16, (i, kind, a.fmt)
        assert tuple(a.t.shape) == (a.B, a.H, a.W, a.pitch), (i, kind)
        assert a.C % 8 == 0 and a.c_off % 8 == 0 and a.pitch % 8 == 0 and a.c_off + a.C <= a.pitch, \
            (i, kind, a.C, a.c_off, a.pitch)
        for (o, c, k) in seen.setdefault(a.t.data_ptr(), []):
            assert a.c_off >= o + c or o >= a.c_off + a.C, ("two ops wrote overlapping slices", kind, k)
        seen[a.t.data_ptr()].append((a.c_off, a.C, kind))
        keep = _inside_mask(a, rects, canvas).to(dev)
        t = a.t.view(torch.int16)
        assert not bool(t[~keep].any()), ("non-zero bits outside the rectangles", i, kind, a.C, a.c_off, a.pitch)
        assert bool(a.t[..., a.c_off:a.c_off + a.C][keep].float().abs().sum() > 0), (i, kind)
    # every member of every buffer was written by some op of the trace
    for ptr, spans in seen.items():
        pitch = next(a.pitch for _, a in trace if a is not None and not a.nchw and a.t.data_ptr() == ptr)
        assert sum(c for _, c, _ in spans) == pitch, (spans, pitch)
    want = {"resdcn_18": {"conv", "maxpool", "dcn", "deconv"}, "hourglass": {"conv", "upsample"},
            "dla_34": {"conv", "maxpool", "dcn", "dwdeconv"}}[f32.NETS[case][0]]
    assert want <= kinds, (want, kinds)
    n_mask = sum(1 for k, _ in trace if k == "mask")
    print("%s right=%s: %d launches, %d of them masks, op kinds %s" % (case, right, len(trace), n_mask, sorted(kinds)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("case", ["resdcn_18", "dla_34", "dla_34_pose", "hourglass"])
def test_images_of_a_half_canvas_are_isolated(dev, case, right):
    m, rects = _model(case, dev), f32._rects(case, right)
    sizes, canvas = f32._geometry(case)
    n = len(sizes)
    base = f32._forward(m, f32._canvas_batch(case, right, 0.0), rects, dev)
    plan = m.plan_for(n, canvas[0], canvas[1], dev, deferred=False, ragged=True, origin=not right)
    assert plan.b.origin is (not right) and plan.b.dtype == torch.float16
    for fill in (float("nan"), 60000.0):
        got = f32._forward(m, f32._canvas_batch(case, right, fill), rects, dev)
        for name, ref in base.items():
            for b in range(n):
                assert np.array_equal(_bits(f32._inside(got[name][b], rects[b])),
                                      _bits(f32._inside(ref[b], rects[b]))), (name, b, fill)
    # the other images with other contents (at their own sizes): image 0 does not move by a bit
    order = [0, 2, 1] if n == 3 else [0, 5]
    got = f32._forward(m, f32._canvas_batch(case, right, 0.0, order=order), rects, dev)
    for name, ref in base.items():
        assert np.array_equal(_bits(f32._inside(got[name][0], rects[0])), _bits(f32._inside(ref[0], rects[0]))), name
        assert not np.array_equal(_bits(got[name][1]), _bits(ref[1]))
        assert np.isfinite(f32._inside(ref[0], rects[0])).all()
    for name in engine.HEAT_MAPS:
        if name in base:
            keep = np.zeros(base[name].shape, bool)
            for b in range(n):
                f32._inside(keep[b], rects[b])[...] = True
            assert (base[name][~keep] == np.float32(engine.HM_FILL)).all() and keep.sum() < keep.size
            assert not (base[name][keep] == np.float32(engine.HM_FILL)).any()


# ------------------------------------------------------------------------------------------------
# 3. parity with the oracle of every image's own forward, at the half-network bar
# ------------------------------------------------------------------------------------------------
PARITY = os.path.join(ROOT, "profiles", "keep_res_canvas_half_parity.jsonl")


def _report(rec):
    """One line per (case, alignment) into profiles/keep_res_canvas_half_parity.jsonl, the line of an earlier run
    replaced (the format of keep_res_canvas_parity.jsonl)."""
    try:
        lines = [json.loads(l) for l in open(PARITY)] if os.path.exists(PARITY) else []
        lines = [l for l in lines if (l["case"], l["right_aligned"]) != (rec["case"], rec["right_aligned"])]
        with open(PARITY, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines + [rec]))
    except (OSError, ValueError, KeyError):
        pass


def _scaled(got, ref):
    """|got - ref| in units of the reference map's rms scale (at least 1): the measure of the half-network bar"""
    scale = max(1.0, float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))))
    return np.abs(got - ref) / scale


def _batch_spread(case, dev):
    """What tests/test_gpu_half_dla_net.py::test_half_dla_batch_independence reports, for this case's network at
    this case's canvas size: image 0 of a B = 2 ordinary half forward against its B = 1 forward -- the routes
    (kernel form, K split) follow the grid size, so the two differ by rounding.  (max, p99) over the heads.
    Ordinary plans only: nothing of the canvas code runs here."""
    if case not in _spread:
        m = _model(case, dev)
        _, (hc, wc) = f32._geometry(case)
        x = synth.images(2, hc, wc, seed=4).to(dev)
        with torch.no_grad():
            two = {k: v[0].cpu().numpy() for k, v in m(x, check=False)[-1].items()}
            one = {k: v[0].cpu().numpy() for k, v in m(x[:1].contiguous(), check=False)[-1].items()}
        e = {k: _scaled(two[k], one[k]) for k in one}
        _spread[case] = (max(float(v.max()) for v in e.values()),
                         max(float(np.quantile(v, 0.99)) for v in e.values()),
                         {k: int((two[k] != one[k]).sum()) for k in one})
    return _spread[case]


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("case", ["resdcn_18", "dla_34", "dla_34_pose", "hourglass"])
def test_half_canvas_forward_matches_the_oracle_of_every_image(dev, case, right):
    """In-rectangle head maps of the half canvas forward against ``net_oracle.forward`` of each image's own input,
    at the bar of tests/test_gpu_half_resnet.py and tests/test_gpu_half_dla_net.py: per head max < 2e-2 and
    p99 < 5e-3 of the map's rms scale.  The half single-image forward is measured against the same oracle, and
    the canvas may be worse than it by no more than the B = 1 / B = 2 spread of the ordinary half plans of the
    same build (``_batch_spread``: a canvas plan runs other routes than a single-image plan, as a B = 2 plan
    does): the margin is measured on code that is not under test."""
    m, rects = _model(case, dev), f32._rects(case, right)
    arch, heads = f32.NETS[case]
    sizes, _ = f32._geometry(case)
    got = f32._forward(m, f32._canvas_batch(case, right, 0.0), rects, dev)
    cmax, cp99, amax, ap99 = {}, {}, {}, {}
    for b in range(len(sizes)):
        key = (case, b, right)
        if key not in _oracle:
            ref = net_oracle.forward(arch, m.state_dict(), f32._image(case, b, right), list(heads))
            _oracle[key] = {k: v.numpy()[0] for k, v in ref.items()}
        with torch.no_grad():
            one = m(f32._image(case, b, right).to(dev), check=False)[-1]
        for name, ref in _oracle[key].items():
            ec = _scaled(f32._inside(got[name][b], rects[b]), ref)
            ea = _scaled(one[name][0].cpu().numpy(), ref)
            for d, v in ((cmax, ec.max()), (cp99, np.quantile(ec, 0.99)), (amax, ea.max()), (ap99, np.quantile(ea, 0.99))):
                d[name] = max(d.get(name, 0.0), float(v))
    smax, sp99, differ = _batch_spread(case, dev)
    print("%s right=%s: canvas max %r p99 %r; single image max %r p99 %r; B=1/B=2 spread max %.3e p99 %.3e "
          "(values that differ: %r)" % (case, right, cmax, cp99, amax, ap99, smax, sp99, differ))
    _report({"case": case, "right_aligned": right, "canvas_vs_oracle": cmax, "canvas_vs_oracle_p99": cp99,
             "single_image_vs_oracle": amax, "single_image_vs_oracle_p99": ap99,
             "batch_spread_max": smax, "batch_spread_p99": sp99, "batch_spread_values_differing": differ})
    for name in cmax:
        assert cmax[name] < 2e-2 and cp99[name] < 5e-3, (name, cmax[name], cp99[name])
        assert cmax[name] <= amax[name] + smax, (name, cmax[name], amax[name], smax)
        assert cp99[name] <= ap99[name] + sp99, (name, cp99[name], ap99[name], sp99)


# ------------------------------------------------------------------------------------------------
# 4. the canvas pipe of --fp16 --keep_res detectors
# ------------------------------------------------------------------------------------------------
MIXED, LARGER, CONFIGS = f32.MIXED, f32.LARGER, f32.CONFIGS
FP16_TOL = 2e-3       # the project's bar for fp16 pipes against run (test_fp16_frame_and_image_pipes_equal_run)


@pytest.fixture(scope="module")
def ctdet(dev):
    det = f32._build("ctdet", ["--arch", "resdcn_18", "--fp16"])
    assert det.model.compute_dtype == torch.float16
    return det


@pytest.fixture(scope="module")
def multi_pose(dev):
    det = f32._build("multi_pose", ["--arch", "dla_34", "--K", "6", "--fp16"])     # K = 6: see test_gpu_canvas.py
    assert det.model.compute_dtype == torch.float16
    return det


def _pipe_run(det, images):
    """One canvas batch through the pipe: (pipe, its results, [(raw rows, metas, scale)] per level)"""
    n = len(images)
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
        assert np.isfinite(dets).all()
        per_scale.append((dets, pipe._metas(0, li, n), lv.scale))
        assert tuple(lv.batch.shape[2:]) == pipe.canvases[0][li]
        plan = det.model.__dict__["_ran"]
        assert plan.b.ragged and plan.b.dtype == torch.float16 and plan.b.origin is (not det.opt.flip_test)
    return pipe, got, per_scale


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("task", ["ctdet", "multi_pose"])
def test_half_canvas_pipe_tails(dev, request, task, config):
    """(a) the device tail == the host tail on the pipe's own raw detections, bit for bit; (c) ``run_images``
    equals the pipe's results.  The plans that ran are ragged half plans."""
    det = f32._configure(request.getfixturevalue(task), config)
    images = f32._images(300)
    pipe, got, per_scale = _pipe_run(det, images)
    f32._same(got, [f32._host_tail(det, per_scale, i) for i in range(len(images))], "host tail on the same detections")
    f32._same(det.run_images(images), got, "run_images")
    assert all(len(r) for r in got)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("task", ["ctdet", "multi_pose"])
def test_half_canvas_pipe_rows_against_the_single_image(dev, request, task, config):
    """(b) the raw rows of every image against ``_run_scale`` of that image alone through ``compare_topk``: scores
    and boxes (and joints) within 2e-3 -- the bar of test_fp16_frame_and_image_pipes_equal_run --, class identical,
    and at least 95 % of an image's K rows paired, as tests/test_gpu_canvas.py::test_canvas_pipe asks in fp32 of
    the same images.  Every image is compared before anything is asserted; the fractions go to
    profiles/keep_res_canvas_half_parity.jsonl.

    MEASURED (MI355X): every row of every image pairs in place with eps = 0 in all six configurations -- the raw
    rows of the canvas are bit-equal to those of the image alone.  That needs the deformable layers of a ragged half
    plan to form their sampling positions relative to the image's own rectangle (cn_dcn_v2_forward_nhwc_f16_rects,
    tests/test_gpu_dcn_half_rects.py): flip-test puts the mirror image right-aligned, off the canvas origin, and
    with positions formed from the absolute column the bilinear fractions round differently there (hm logits up
    to 4.9e-4 apart, scores up to 6.5e-5), which decided near-ties of the reference's own scores the other way --
    two adjacent cells of one class at 0.23401 / 0.23403 (ctdet), the 6th and 7th of K = 6 peaks 2e-6 apart
    (multi_pose) -- and three of these cases failed on it."""
    det = f32._configure(request.getfixturevalue(task), config)
    images, k = f32._images(300), 2 if det.opt.flip_test else 1
    pipe, got, per_scale = _pipe_run(det, images)
    fractions, failures = [], []
    for (dets, metas, scale), lv in zip(per_scale, pipe.levels):
        for i, im in enumerate(images):
            one, meta = det.pre_process_device(im, lv.scale)
            h, w = one.shape[2:]
            assert torch.equal(lv.batch[k * i, :, :h, :w].view(torch.int32), one[0].view(torch.int32)), (scale, i)
            alone = det._run_scale(one, pipe.flip).detach().cpu().numpy()
            D = dets.shape[2]
            try:
                r = compare_topk(dets[i:i + 1], alone, box_cols=tuple(range(4)) + tuple(range(5, D - 1)),
                                 score_tol=FP16_TOL, box_tol=FP16_TOL,
                                 got_ids=dets[i:i + 1, :, D - 1:].astype(np.int64),
                                 ref_ids=alone[:, :, D - 1:].astype(np.int64))
            except AssertionError as e:
                r = {"compare_topk_raised": repr(e.args[0] if e.args else e)}
                failures.append((scale, i, r))
            else:
                if r["paired"] < 0.95:
                    failures.append((scale, i, r))
            print("%s %s fp16 scale %s image %d: %r" % (task, config, scale, i, r))
            fractions.append({"scale": scale, "image": i, **r})
    _report({"case": "pipe/%s/%s" % (task, config), "right_aligned": bool(det.opt.flip_test), "compare_topk": fractions})
    assert not failures, failures


def test_half_stream_over_two_canvases_equals_run_images(dev, ctdet):
    det = f32._configure(ctdet, "flip")
    batches = [f32._images(310), f32._images(320, LARGER), f32._images(330), f32._images(340, LARGER[::-1])]
    alone = [det.run_images(b) for b in batches]
    streamed = list(det.run_images_stream(iter(batches), depth=2))
    assert len(streamed) == len(batches)
    for s, a in zip(streamed, alone):
        f32._same(s, a)
    pipe = det._canvas_pipe_for(batches[0], 2, None, "run_images_stream")
    assert sorted(pipe.levels[0].batches) == [(96, 128), (128, 160)]


def test_half_pinned_canvas_is_one_ragged_half_plan(dev, ctdet):
    det = f32._configure(ctdet, "single")
    small, large = f32._images(350), f32._images(360, LARGER)
    f32._same(det.run_images(large, canvas=CANVAS), det.run_images(large), "own maxima == the pinned canvas")
    det.model.drop_plans()
    det.run_images(small, canvas=CANVAS)
    det.run_images(large, canvas=CANVAS)
    plans = det.model.__dict__["_plans"]
    ragged = [key for key in plans if "ragged" in key]
    assert len(ragged) == 1 and ragged[0][1:3] == CANVAS, ragged
    assert torch.float16 in ragged[0] and plans[ragged[0]].b.dtype == torch.float16
    det.run_images(small)                                    # its own canvas: another plan
    assert len([key for key in det.model.__dict__["_plans"] if "ragged" in key]) == 2


# every family with a half plan, both tasks: the families the pipe tests above do not run
FAMILIES = [("ctdet", "res_18"), ("ctdet", "hourglass"), ("ctdet", "dla_34"), ("multi_pose", "resdcn_18"),
            ("multi_pose", "hourglass")]
FAMILY_SHAPES = [(100, 140), (120, 100), (60, 200)]     # inputs of two or three sizes at pad 31 and at pad 127


def _top_score(res):
    return max(float(np.asarray(rows, np.float32)[:, 4].max()) for rows in res.values() if len(rows))


@pytest.mark.parametrize("task,arch", FAMILIES)
def test_half_canvas_batches_run_on_every_family(dev, task, arch):
    """--fp16 --keep_res with flip-test: ``run_images`` of a mixed-size batch runs a ragged half plan on the device
    tail, gives finite rows, ``run_images_stream`` gives the same bit for bit, and every image's best score is
    within 2e-3 of ``run(image)``'s (the best score does not depend on how near-ties are ranked)."""
    det = f32._configure(f32._build(task, ["--arch", arch, "--fp16", "--K", "20"]), "flip")
    assert det.model.compute_dtype == torch.float16
    images = f32._images(390, FAMILY_SHAPES)
    got = det.run_images(images)
    assert len(got) == len(images) and det.tail_fallbacks == 0
    plans = det.model.__dict__["_plans"]
    ragged = [key for key in plans if "ragged" in key]
    assert ragged and all(plans[key].b.dtype == torch.float16 for key in ragged), list(plans)
    for res in got:
        assert all(np.isfinite(np.asarray(rows, np.float32)).all() for rows in res.values())
    f32._same(list(det.run_images_stream(iter([images, images])))[1], got, "run_images_stream")
    for im, res in zip(images, got):
        alone = det.run(im)["results"]
        assert abs(_top_score(res) - _top_score(alone)) < 2e-3, (_top_score(res), _top_score(alone))
