"""half_compute() on the ResNet networks: the deformable module in a half plan against the oracle, res_18 /
resdcn_18 / resdcn_101 against the committed fp32 goldens, a --fp16 detector against the f32s one, and batch
independence."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centernet_amd import synth
from oracle import net_oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as dh   # noqa: E402
from dcn_cases import TOL     # noqa: E402

pytestmark = pytest.mark.gpu
HEADS = {"hm": 80, "wh": 2, "reg": 2}


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _model(arch, heads, seed, dev):
    from centernet_amd.model import create_model
    m = create_model(arch, dict(heads), 64)
    synth.fill_state_dict_(m, seed)
    return m.to(dev).eval()


@pytest.mark.parametrize("shape", [(1, 64, 8, 16, 64), (2, 128, 9, 11, 40)], ids=["tileable", "ragged"])
def test_half_plan_dcn_module_against_the_oracle(dev, shape):
    """PlanBuilder(dtype=float16).dcn with the module's own offset convolution, against net_oracle.dcn on the same
    half-rounded operands (input, both weights; biases stay fp32).

    With om64 the float64 offset convolution, ref64 / cols the float64 deformable result on om64's offsets and
    sigmoid(om64) masks, E32 = max |net_oracle.dcn - ref64| and E32om = max |torch fp32 offset conv - om64|, the bar is
        |got - ref64| <= [2^-11 |ref64| + 2^-25 + 2^-11 (|w| . |cols|) + 4 E32]          (the A2 bar, scale = 1)
                         + 2e-5 (1 + |ref64|)                                             (in-kernel sigmoid, dcn_cases.TOL)
                         + 4.25 * (4 E32om) * max |x| * sum_k |w_k|                       (the offset conv's fp32-output bar, propagated)
    The last term: the kernel's offsets and mask logits are within 4 E32om of om64 (that convolution's A2 bar).  A
    bilinear sample moves by at most 2 max |x| per pixel of either offset and the mask by at most 1/4 per unit of its
    logit, so one column entry moves by at most (2 + 2 + 1/4) max |x| times that error; summed with |w| over K."""
    from centernet_amd.dcn_v2 import DCN
    from centernet_amd.engine import PlanBuilder, Act
    B, Cin, H, W, Cout = shape
    mod = DCN(Cin, Cout, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
    synth.fill_state_dict_(mod, 77)
    with torch.no_grad():
        mod.weight.copy_(mod.weight.half().float())
        # offsets of a pixel or two and mask logits of order one, as in a trained layer
        mod.conv_offset_mask.weight.copy_(torch.from_numpy(
            synth.normal(tuple(mod.conv_offset_mask.weight.shape), (2.0 / (Cin * 9)) ** 0.5, 78)).half().float())
        mod.conv_offset_mask.bias.copy_(torch.from_numpy(synth.normal((27,), 0.3, 79)))
    mod = mod.to(dev).eval()
    x = torch.from_numpy(synth.normal((B, Cin, H, W), 1.0, 80)).half().float()
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    want32 = net_oracle.dcn(x, {"d." + k: v for k, v in sd.items()}, "d").double()
    cw, cb = sd["conv_offset_mask.weight"], sd["conv_offset_mask.bias"]
    om64 = F.conv2d(x.double(), cw.double(), cb.double(), 1, 1)
    e32om = float((F.conv2d(x, cw, cb, 1, 1).double() - om64).abs().max())
    o1, o2, ml = torch.chunk(om64, 3, dim=1)
    one, zero = torch.ones(Cout), torch.zeros(Cout)
    ref, cols = dh.dcn_ref64(x, torch.cat((o1, o2), 1), torch.sigmoid(ml), sd["weight"], sd["bias"], one, zero, False)
    e32 = float((want32 - ref).abs().max())
    pb = PlanBuilder(dev, B, H, W, dtype=torch.float16)
    xa = Act(x.permute(0, 2, 3, 1).contiguous().to(dev, torch.float16), B, H, W, Cin, fmt="f16")
    y = pb.dcn(xa, mod)
    assert y.t.dtype == torch.float16 and y.fmt == "f16"
    y.t.fill_(float("nan"))
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    got = y.t.permute(0, 3, 1, 2).float().cpu()
    bar = ref.abs() * 2.0 ** -11 + 2.0 ** -25 + dh.sample_term(sd["weight"], cols, one).view(B, Cout, H, W) + 4 * e32
    bar = bar + TOL * (1 + ref.abs())
    wsum = sd["weight"].double().abs().reshape(Cout, -1).sum(1).view(1, Cout, 1, 1)
    bar = bar + 4.25 * (4 * e32om) * float(x.abs().max()) * wsum
    err = (got.double() - ref).abs()
    print("half plan dcn %s: E32 %.3e, E32om %.3e, max |err| %.3e, max err / bar %.3f" % (
        shape, e32, e32om, float(err.max()), float((err / bar).max())))
    assert not torch.isnan(got).any()
    assert not bool((err > bar).any()), int((err > bar).sum())


@pytest.mark.parametrize("case", ["res_18", "resdcn_18", "resdcn_101"])
def test_half_resnets_vs_fp32_golden(dev, gen, net_golden, case):
    """half_compute() against the fp32 goldens of the reference's own modules (1 x 128 x 128), at the bar the project
    set for its fp16 network test (test_hourglass_fp16_vs_fp32_oracle): per head max < 2e-2 and p99 < 5e-3 of the
    map's rms scale.  That bar was set on Hourglass; the observed values are printed."""
    z, meta = net_golden
    m = _model(case, gen.NET_HEADS, gen.NET_SEED, dev)
    m.half_compute()
    B, H, W = gen.NET_INPUT
    x = synth.images(B, H, W, seed=0)
    with torch.no_grad():
        out = m(x.to(dev))[-1]
    fails = []
    for h in gen.NET_HEADS:
        ref = z["%s/%s" % (case, h)]
        got = out[h].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape
        scale = max(1.0, float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))))
        e = np.abs(got - ref) / scale
        print("%s fp16 head %s: max %.2e  p99 %.2e" % (case, h, e.max(), np.quantile(e, 0.99)))
        if not (e.max() < 2e-2 and np.quantile(e, 0.99) < 5e-3):
            fails.append((h, float(e.max()), float(np.quantile(e, 0.99))))
    assert not fails, fails


def _detector(extra):
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet", "--arch", "resdcn_18", "--K", "40", "--input_res", "256"] + extra)
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


def test_fp16_detector_run_batch_against_f32s(dev):
    """A 4-image run_batch of resdcn_18 with --fp16 against the same detector in f32s: score delta below 2e-2 (the
    bar of test_end_to_end_hourglass_512_batch8), class agreement reported."""
    x = synth.images(4, 256, 256, seed=9).to(dev)
    det16 = _detector(["--fp16"])
    assert det16.model.compute_dtype == torch.float16 and det16.model.deferred_names() == ()
    d16 = det16.run_batch(x).clone().cpu().numpy()
    ref = _detector([]).run_batch(x).clone().cpu().numpy()
    assert d16.shape == ref.shape and np.isfinite(d16).all()
    e = np.abs(d16[..., 4] - ref[..., 4])
    same_cls = (d16[..., 5] == ref[..., 5]).mean()
    print("resdcn_18 fp16 B=4 256^2: score delta max %.2e mean %.2e, class agreement %.3f" % (e.max(), e.mean(), same_cls))
    assert e.max() < 2e-2


def test_half_batch_independence(dev):
    """Image 0 of a B = 2 half run equals the B = 1 run bit for bit."""
    m = _model("resdcn_18", HEADS, 317, dev)
    m.half_compute()
    x = synth.images(2, 128, 128, seed=4).to(dev)
    with torch.no_grad():
        two = {k: v.clone() for k, v in m(x)[-1].items()}
        one = m(x[:1].contiguous())[-1]
        for k in HEADS:
            diff = (one[k][0] != two[k][0])
            print("half batch independence %s: %d of %d values differ, max |diff| %.3e" % (
                k, int(diff.sum()), diff.numel(), float((one[k][0] - two[k][0]).abs().max())))
        for k in HEADS:
            assert torch.equal(one[k][0], two[k][0]), k


@pytest.mark.parametrize("task", ["ctdet", "multi_pose"])
def test_fp16_frame_and_image_pipes_equal_run(dev, task):
    """run, run_frames and run_images of a --fp16 detector (nothing deferred, heads fp32 NCHW): the pipes give what
    run gives image by image, at the tolerance the f32s pipes are held to (test_ctdet_run_frames_flip_equals_run)."""
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task, "--arch", "resdcn_18", "--input_h", "128", "--input_w", "128", "--fp16"])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    assert det.model.compute_dtype == torch.float16
    rng = np.random.RandomState(23)
    frames = [rng.randint(0, 256, (100, 140, 3)).astype(np.uint8) for _ in range(3)]
    images = frames[:2] + [rng.randint(0, 256, (90, 120, 3)).astype(np.uint8)]
    for batch, got in ((frames, det.run_frames(frames)), (images, det.run_images(images))):
        assert len(got) == len(batch)
        for f, rb in zip(batch, got):
            rs = det.run(f)["results"]
            assert set(rb) == set(rs)
            for j in rs:
                a, b = np.asarray(rb[j], np.float32), np.asarray(rs[j], np.float32)
                assert a.shape == b.shape and np.isfinite(a).all(), (task, j, a.shape, b.shape)
                if a.size:
                    assert np.abs(a - b).max() < 2e-3, (task, j, float(np.abs(a - b).max()))
