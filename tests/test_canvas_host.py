"""Canvas batches under --keep_res, the host side (no GPU): the masking rule itself, checked on the torch
oracle, and the tables and refusals of ``run_images``.

The rule: an image's network input sits in a larger canvas; when every materialised tensor is
zero outside the image's rectangle, the convolutions' taps read the zeros that their own padding would have
supplied, and the head maps inside the rectangle are those of the image's own forward."""
import numpy as np
import pytest
import torch

from centernet_amd import synth
from oracle import net_oracle

HEADS = {"hm": 80, "wh": 2, "reg": 2}
CANVAS = (128, 160)
IMAGE = (64, 96)


def _masked_forward(monkeypatch, sd, canvas, x0, skip=()):
    """``net_oracle.forward`` of resdcn_18 on ``canvas`` with the input and every ``_t`` trace point (the
    materialised tensors) zeroed outside the IMAGE rectangle at column ``x0``; ``skip``: trace points left
    unmasked; ``skip=None``: no masks at all."""
    Hc, Wc = CANVAS
    h, w = IMAGE

    def mask(t):
        s = Hc // t.shape[2]
        assert t.shape[2] * s == Hc and t.shape[3] * s == Wc
        out = torch.zeros_like(t)
        out[:, :, :h // s, x0 // s:(x0 + w) // s] = t[:, :, :h // s, x0 // s:(x0 + w) // s]
        return out

    def traced(name, t):
        return t if (skip is None or name in skip) else mask(t)
    monkeypatch.setattr(net_oracle, "_t", traced)
    return net_oracle.forward("resdcn_18", sd, canvas if skip is None else mask(canvas), list(HEADS))


@pytest.fixture(scope="module")
def single():
    from centernet_amd.model import create_model
    m = create_model("resdcn_18", dict(HEADS), 64)
    synth.fill_state_dict_(m, 317)
    sd = m.state_dict()
    x = synth.images(1, IMAGE[0], IMAGE[1], seed=3)
    return sd, x, net_oracle.forward("resdcn_18", sd, x, list(HEADS))


def _errors(out, ref, x0):
    """Per head: max |difference| inside the rectangle over the map's scale (tests/test_gpu_net.py's measure)."""
    h, w = IMAGE[0] // 4, IMAGE[1] // 4
    errs = {}
    for name, r in ref.items():
        r = r.numpy()
        got = out[name].numpy()[:, :, :h, x0 // 4:x0 // 4 + w]
        scale = max(1.0, float(np.sqrt(np.mean(r.astype(np.float64) ** 2))))
        errs[name] = float(np.abs(got - r).max() / scale)
    return errs


def _canvas(x, x0):
    g = torch.Generator().manual_seed(11)
    canvas = torch.randn((1, 3) + CANVAS, generator=g) * 3.0       # garbage outside the rectangle
    canvas[:, :, :IMAGE[0], x0:x0 + IMAGE[1]] = x
    return canvas


@pytest.mark.parametrize("x0", [0, 64])
def test_masked_canvas_forward_is_the_images_own_forward(monkeypatch, single, x0):
    sd, x, ref = single
    errs = _errors(_masked_forward(monkeypatch, sd, _canvas(x, x0), x0), ref, x0)
    print("x0 = %d: %r" % (x0, errs))
    assert max(errs.values()) < 1e-4, errs


def test_left_aligned_rectangle_needs_no_mask_on_the_stem(monkeypatch, single):
    """What lets a plan of rectangles at the canvas origin keep the stem's max-pool inside the stem launch."""
    sd, x, ref = single
    errs = _errors(_masked_forward(monkeypatch, sd, _canvas(x, 0), 0, skip=("stem",)), ref, 0)
    print(errs)
    assert max(errs.values()) < 1e-4, errs


def test_negative_controls_exceed_the_bar(monkeypatch, single):
    """Without masks, and right-aligned with the stem left unmasked, the maps are wrong: the tests above
    cannot pass vacuously."""
    sd, x, ref = single
    none = _errors(_masked_forward(monkeypatch, sd, _canvas(x, 0), 0, skip=None), ref, 0)
    stem = _errors(_masked_forward(monkeypatch, sd, _canvas(x, 64), 64, skip=("stem",)), ref, 64)
    print("no masks: %r; right-aligned, stem unmasked: %r" % (none, stem))
    assert max(none.values()) > 1e-4, none
    assert max(stem.values()) > 1e-4, stem


# ------------------------------------------------------------------------------------------------
# the tables of a canvas batch, and the refusals
# ------------------------------------------------------------------------------------------------
SIZES = [(40, 70), (64, 64), (33, 100), (95, 31)]
SCALES = (1.0, 0.75)


def _detector(cls=None, task="ctdet", args=("--keep_res",)):
    from centernet_amd.detectors.base_detector import BaseDetector
    from centernet_amd.opts import opts
    cls = cls or BaseDetector
    det = cls.__new__(cls)
    det.opt = opts().init([task] + list(args))
    det.mean = np.array(det.opt.mean, dtype=np.float32).reshape(1, 1, 3)
    det.std = np.array(det.opt.std, dtype=np.float32).reshape(1, 1, 3)
    det.scales = list(SCALES)
    return det


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.parametrize("flip", [False, True])
def test_canvas_tables_equal_the_single_image_geometry(flip):
    from centernet_amd import native
    from centernet_amd.frame_pipe import ImageTables
    from centernet_amd.image import get_affine_transform, invert_affine
    det = _detector()
    assert det.opt.pad == 31 and not det.opt.fix_res
    assert det.input_geometry(64, 64, 1.0)[4:6] == (96, 96)      # a multiple of 32 still gets + 32
    tables, S, B, k = ImageTables(det, SCALES), len(SCALES), len(SIZES), 2 if flip else 1
    desc = np.zeros((S, 2, B), native.IMAGE_DESC)
    to_source = np.zeros((S, B, 6), np.float64)
    tables.fill(SIZES, desc, to_source)
    canvases = tables.canvas(SIZES)
    rects = np.full((S, k * B, 4), -1, np.int32)
    tables.fill_rects(SIZES, canvases, flip, rects)
    for l, scale in enumerate(SCALES):
        gs = [det.input_geometry(H, W, scale) for H, W in SIZES]
        hc, wc = canvases[l]
        assert (hc, wc) == (max(g.inp_h for g in gs), max(g.inp_w for g in gs))
        assert hc % 32 == 0 and wc % 32 == 0 and not (rects[l] % 32).any()
        for j, g in enumerate(gs):
            assert tuple(rects[l, k * j]) == (0, 0, g.inp_w, g.inp_h)
            if flip:
                assert tuple(rects[l, k * j + 1]) == (wc - g.inp_w, 0, wc, g.inp_h)
            # what run(image) computes: pre_process_device's matrix and post_process' inverse map
            to_input = get_affine_transform(g.center, g.extent, 0, [g.inp_w, g.inp_h])
            assert np.array_equal(_bits(desc[l, 1, j]['dst_to_src']), _bits(invert_affine(to_input).reshape(-1)))
            meta = det._meta(g)
            inv = get_affine_transform(meta['c'], meta['s'], 0, (meta['out_width'], meta['out_height']), inv=1)
            assert np.array_equal(_bits(to_source[l, j]), _bits(np.asarray(inv).reshape(-1)))
    # a pinned canvas goes through the images' own rule at every scale, and holds every image there
    pinned = tables.canvas(SIZES, (128, 160))
    assert pinned[0] == (128, 160)
    assert pinned[1] == tuple(det.input_geometry(127, 159, 0.75)[4:6])
    assert all(p[0] >= c[0] and p[1] >= c[1] for p, c in zip(pinned, canvases))
    tables.fill_rects(SIZES, pinned, flip, rects)
    assert tuple(rects[0, 0]) == (0, 0, 96, 64) and (not flip or tuple(rects[0, 1]) == (64, 0, 160, 64))


def test_canvas_argument_is_checked():
    from centernet_amd.frame_pipe import ImageTables
    tables = ImageTables(_detector(), SCALES)
    assert tables.check_canvas(SIZES, (128, 160)) == (128, 160)
    assert tables.check_canvas(SIZES, [160, 192]) == (160, 192)
    assert tables.canvas(SIZES)[0] == (96, 128) and tables.check_canvas(SIZES, (96, 128)) == (96, 128)
    for bad in ((64, 160), (96, 96), (130, 160), (128, 161), (0, 160), (128.5, 160), (128,), None, "ab"):
        with pytest.raises(ValueError):
            tables.check_canvas(SIZES, bad)
    with pytest.raises(ValueError):                  # a canvas the batch does not fit at a test scale
        tables.fill_rects(SIZES, [(96, 96), (96, 96)], False, np.zeros((2, 4, 4), np.int32))


def test_refusals():
    from centernet_amd.detectors.ctdet import CtdetDetector
    from centernet_amd.detectors.exdet import ExdetDetector
    from centernet_amd.detectors.multi_pose import MultiPoseDetector
    a, b = np.zeros((40, 70, 3), np.uint8), np.zeros((95, 31, 3), np.uint8)
    exdet = _detector(ExdetDetector, "exdet")
    assert not exdet._canvas_batches()
    with pytest.raises(ValueError, match="keep_res"):
        exdet.run_images([a, b])
    with pytest.raises(ValueError, match="keep_res"):
        list(exdet.run_images_stream(iter([[a, b]])))
    with pytest.raises(ValueError, match="keep_res"):          # today's refusal, canvas= or not
        exdet.run_images([a, b], canvas=(128, 160))
    with pytest.raises(ValueError, match="canvas"):
        exdet.run_images([a, a], canvas=(128, 160))
    for cls, task in ((CtdetDetector, "ctdet"), (MultiPoseDetector, "multi_pose")):
        det = _detector(cls, task)
        assert det._canvas_batches() and det._images_one_size([a, b], "run_images") is False
        for bad in ((64, 96), (130, 160)):           # too small, no multiple of pad + 1: before any pipe is built
            with pytest.raises(ValueError, match="canvas"):
                det.run_images([a, b], canvas=bad)
            with pytest.raises(ValueError, match="canvas"):
                list(det.run_images_stream(iter([[a, b]]), canvas=bad))
        fixed = _detector(cls, task, args=())
        assert not fixed._canvas_batches()
        with pytest.raises(ValueError, match="canvas"):
            fixed.run_images([a, b], canvas=(128, 160))


@pytest.mark.parametrize("flip", [False, True])
def test_origin_is_false_exactly_with_flip(flip):
    """A plan of rectangles at the canvas origin keeps the stem's max-pool inside the stem launch; the mirror
    images of flip-test sit at the canvas' right edge, and need the other plan."""
    from centernet_amd.engine import CanvasRects
    from centernet_amd.frame_pipe import ImagePipe, ImageTables
    pipe = ImagePipe.__new__(ImagePipe)
    pipe.canvas, pipe.flip = True, flip
    k = 2 if flip else 1
    pipe.rects_pinned, pipe.rects_dev = [torch.zeros((2, k * 4, 4), dtype=torch.int32)], [[None, None]]
    tables = ImageTables(_detector(), SCALES)
    tables.fill_rects(SIZES, tables.canvas(SIZES), flip, pipe.rects_pinned[0].numpy())
    for level in range(2):
        r = pipe._rects(0, level)
        assert isinstance(r, CanvasRects)
        host, dev, origin = r
        assert origin is (not flip)
        assert bool((host[:, :2] == 0).all()) is origin     # and it is what the rectangles themselves say
    pipe.canvas = False
    assert pipe._rects(0, 0) is None
