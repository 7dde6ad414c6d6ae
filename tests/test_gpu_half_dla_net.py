"""half_compute() on dla_34: against the committed fp32 goldens, in-place against copying concatenation, batch
independence, and --fp16 detectors (ctdet, multi_pose, ddd) against the f32s ones and across their pipes.  The
bars are the project's own for half networks (tests/test_gpu_half_resnet.py)."""
import contextlib
import sys

import numpy as np
import pytest
import torch

from centernet_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _model(heads, seed, dev):
    from centernet_amd.model import create_model
    m = create_model("dla_34", dict(heads), 256)
    synth.fill_state_dict_(m, seed)
    return m.to(dev).eval()


def _scaled_err(got, ref):
    """|got - ref| in units of the reference map's rms scale (at least 1): the measure of the golden bar."""
    scale = max(1.0, float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))))
    return np.abs(got - ref) / scale


@pytest.mark.parametrize("case", ["dla_34", "dla_34_pose"])
def test_half_dla_vs_fp32_golden(dev, gen, net_golden, case):
    """half_compute() against the fp32 goldens of the reference's own modules (1 x 128 x 128), at the bar of
    test_half_resnets_vs_fp32_golden: per head max < 2e-2 and p99 < 5e-3 of the map's rms scale.  The observed
    values are printed.  (At 128^2 level0 runs on conv16h_kernel; level1, Wo = 64, does not.)"""
    z, meta = net_golden
    heads = gen.POSE_HEADS if case.endswith("_pose") else gen.NET_HEADS
    m = _model(heads, gen.NET_SEED, dev)
    m.half_compute()
    B, H, W = gen.NET_INPUT
    x = synth.images(B, H, W, seed=0)
    with torch.no_grad():
        out = m(x.to(dev))[-1]
    fails = []
    for h in heads:
        ref = z["%s/%s" % (case, h)]
        got = out[h].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape
        e = _scaled_err(got, ref)
        print("%s fp16 head %s: max %.2e  p99 %.2e" % (case, h, e.max(), np.quantile(e, 0.99)))
        if not (e.max() < 2e-2 and np.quantile(e, 0.99) < 5e-3):
            fails.append((h, float(e.max()), float(np.quantile(e, 0.99))))
    assert not fails, fails


def test_half_dla_inplace_concat_equals_copying_concat(dev, gen, monkeypatch):
    """The same half forward with CN_CONCAT_INPLACE=0 (every member copied into its buffer) and with the default
    (tree1 / tree2 / the max-pool write their slices): bit-equal heads."""
    m = _model(gen.NET_HEADS, gen.NET_SEED, dev)
    m.half_compute()
    x = synth.images(1, 128, 128, seed=0).to(dev)
    with torch.no_grad():
        inplace = {k: v.clone() for k, v in m(x)[-1].items()}
        monkeypatch.setenv("CN_CONCAT_INPLACE", "0")
        m.drop_plans()
        copying = m(x)[-1]
        for k in gen.NET_HEADS:
            assert torch.equal(inplace[k], copying[k]), k


def test_half_dla_batch_independence(dev, gen):
    """Image 0 of a B = 2 half forward against the B = 1 forward: within the golden bar (the K split may depend on
    B, so bit equality is reported, not required)."""
    m = _model(gen.NET_HEADS, gen.NET_SEED, dev)
    m.half_compute()
    x = synth.images(2, 128, 128, seed=4).to(dev)
    with torch.no_grad():
        two = {k: v.clone() for k, v in m(x)[-1].items()}
        one = m(x[:1].contiguous())[-1]
    fails = []
    for k in gen.NET_HEADS:
        a, b = one[k][0].cpu().numpy(), two[k][0].cpu().numpy()
        e = _scaled_err(b, a)
        print("half dla_34 batch independence %s: %d of %d values differ, max %.2e p99 %.2e of the rms scale" % (
            k, int((a != b).sum()), a.size, e.max(), np.quantile(e, 0.99)))
        if not (np.isfinite(b).all() and e.max() < 2e-2 and np.quantile(e, 0.99) < 5e-3):
            fails.append((k, float(e.max())))
    assert not fails, fails


# ---- detectors ------------------------------------------------------------------------------------------
TASKS = {  # task: (size arguments, (h, w) of the network input, score column of the raw rows)
    "ctdet": (["--input_h", "128", "--input_w", "128"], (128, 128), 4),
    "multi_pose": (["--input_h", "128", "--input_w", "128"], (128, 128), 4),
    "ddd": (["--input_h", "128", "--input_w", "384", "--K", "40"], (128, 384), 2),
}


def _detector(task, extra):
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task, "--arch", "dla_34"] + TASKS[task][0] + list(extra))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


@pytest.mark.parametrize("task", list(TASKS))
def test_fp16_dla_detector_run_batch_against_f32s(dev, task):
    """A 2-image run_batch of dla_34 with --fp16 against the same detector in f32s: score delta below 2e-2 (the bar
    of test_fp16_detector_run_batch_against_f32s)."""
    (h, w), col = TASKS[task][1], TASKS[task][2]
    x = synth.images(2, h, w, seed=9).to(dev)
    det16, _ = _detector(task, ["--fp16"])
    assert det16.model.compute_dtype == torch.float16 and det16.model.deferred_names() == ()
    d16 = det16.run_batch(x).clone().cpu().numpy()
    ref = _detector(task, [])[0].run_batch(x).clone().cpu().numpy()
    assert d16.shape == ref.shape and np.isfinite(d16).all()
    e = np.abs(d16[..., col] - ref[..., col])
    print("dla_34 %s fp16 B=2 %dx%d: score delta max %.2e mean %.2e" % (task, h, w, e.max(), e.mean()))
    assert e.max() < 2e-2


@pytest.mark.parametrize("task", list(TASKS))
def test_fp16_dla_frame_and_image_pipes_equal_run(dev, task):
    """run, run_frames and run_images of a --fp16 dla_34 detector: the pipes give what run gives image by image, at
    the 2e-3 test_fp16_frame_and_image_pipes_equal_run holds the ResNets to."""
    det, opt = _detector(task, ["--fp16"])
    assert det.model.compute_dtype == torch.float16
    rng = np.random.RandomState(23)
    fh, fw = (100, 140) if task != "ddd" else (96, 300)
    frames = [rng.randint(0, 256, (fh, fw, 3)).astype(np.uint8) for _ in range(3)]
    images = frames[:2] + [rng.randint(0, 256, (fh - 10, fw - 20, 3)).astype(np.uint8)]
    calibs = [None] * 3
    if task == "ddd":                          # the task wants every frame's projection matrix
        opt.peak_thresh = 0.0                  # every row of the tail: no row sits on a cut
        calibs = [np.array([[700 + 20 * rng.rand(), 0, 150 + rng.rand(), 40 * rng.rand()],
                            [0, 700 + 20 * rng.rand(), 48 + rng.rand(), rng.rand()],
                            [0, 0, 1, 0.005 * rng.rand()]], np.float32) for _ in range(3)]
    side = (calibs,) if task == "ddd" else ()
    worst = 0.0
    for batch, got in ((frames, det.run_frames(frames, *side)), (images, det.run_images(images, *side))):
        assert len(got) == len(batch)
        for f, p, rb in zip(batch, calibs, got):
            rs = det.run(f, p)["results"]
            assert set(rb) == set(rs)
            for j in rs:
                a, b = np.asarray(rb[j], np.float32), np.asarray(rs[j], np.float32)
                assert a.shape == b.shape and np.isfinite(a).all(), (task, j, a.shape, b.shape)
                if a.size:
                    worst = max(worst, float(np.abs(a - b).max()))
                    assert np.abs(a - b).max() < 2e-3, (task, j, float(np.abs(a - b).max()))
    print("dla_34 %s fp16 pipes against run: max |diff| %.2e" % (task, worst))
