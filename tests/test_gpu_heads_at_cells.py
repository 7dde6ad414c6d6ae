"""The gather-only ctdet heads at the decoded cells (cn_ctdet_heads_at_cells_f32, the deferred-heads plan).
Tolerance: the project's bar, |diff| <= 2e-5 * (1 + |ref|) against torch fp64 (tests/test_gpu_conv.py)."""
import contextlib
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centernet_amd import synth

pytestmark = pytest.mark.gpu
TOL = 2e-5

B, H, W, C, K = 2, 8, 12, 64, 16
# (y, x) per image: the four corners, one cell on each edge, interior cells, one cell three times
CELLS = [
    [(0, 0), (0, 11), (7, 0), (7, 11), (0, 5), (7, 6), (3, 0), (4, 11),
     (1, 1), (3, 7), (3, 7), (3, 7), (6, 10), (2, 9), (5, 3), (4, 4)],
    [(7, 11), (0, 0), (0, 11), (7, 0), (0, 2), (7, 9), (5, 0), (2, 11),
     (6, 1), (1, 10), (2, 2), (2, 2), (2, 2), (4, 6), (3, 3), (5, 8)],
]


def _heads(hidden, names, seed=0, cin=C):
    pairs = {}
    for i, name in enumerate(names):
        c1 = torch.nn.Conv2d(cin, hidden, 3, padding=1, bias=True)
        c2 = torch.nn.Conv2d(hidden, 2, 1, bias=True)
        with torch.no_grad():
            c1.weight.copy_(torch.from_numpy(synth.normal(tuple(c1.weight.shape), (2.0 / (cin * 9)) ** 0.5, seed + 20 + i)))
            c1.bias.copy_(torch.from_numpy(synth.normal((hidden,), 0.2, seed + 30 + i)))
            c2.weight.copy_(torch.from_numpy(synth.normal(tuple(c2.weight.shape), 0.15, seed + 40 + i)))
            c2.bias.copy_(torch.from_numpy(synth.normal((2,), 0.5, seed + 50 + i)))
        pairs[name] = (c1, c2)
    return pairs


def _feature(dev, split, cin=C):
    """The feature map as the output of a PlanBuilder convolution: an f32s Act with a non-zero exponent
    (``split``; max |feature| ~ 8 gives e = -6), or the plain-fp32 Act of the fp32-MFMA mode.  Unit-variance
    input as in test_fused_heads: the bar is absolute near zero, an fp32-level bar for O(1) tensors (the
    bound for larger scales is stated in DESIGN.md 3.4b)."""
    from centernet_amd.engine import Act, PlanBuilder, exponent_for
    x = torch.from_numpy(synth.normal((B, cin, H, W), 1.0, 11))
    w = torch.from_numpy(synth.normal((cin, cin, 1, 1), (2.0 / cin) ** 0.5, 12))
    ref = F.conv2d(x, w)
    ef = exponent_for(float(ref.abs().max()))
    pb = PlanBuilder(dev, B, H, W, split=split, exps={"feat": ef})
    xa = Act(x.permute(0, 2, 3, 1).contiguous().to(dev), B, H, W, cin, exp=exponent_for(float(x.abs().max())))
    feat = pb.conv(xa, w, lid="feat")
    for op in pb.ops:
        op()
    torch.cuda.synchronize()
    if split:
        assert feat.fmt == "f32s" and feat.exp == ef and ef != 0
    else:
        assert feat.fmt == "f32"
    return feat, pb


def _dense_ref(feat, pairs):
    """name -> (B, 2, H, W) float64 on the host, from the feature values the kernels read."""
    x = feat.to_float().permute(0, 3, 1, 2).double().cpu()
    out = {}
    for name, (c1, c2) in pairs.items():
        h = F.relu(F.conv2d(x, c1.weight.detach().double(), c1.bias.detach().double(), padding=1))
        out[name] = F.conv2d(h, c2.weight.detach().double(), c2.bias.detach().double())
    return out


def _late(feat, pairs, dev):
    from centernet_amd.engine import DeferredHeads, pack_cell_heads
    names = list(pairs)
    packed = pack_cell_heads([pairs[n][0] for n in names], [pairs[n][1] for n in names], dev)
    return DeferredHeads(names, feat, pairs[names[0]][0].weight.shape[0], *packed)


@pytest.mark.parametrize("case", [
    (64, ("wh", "reg"), True),
    (256, ("wh", "reg"), True),         # the dla form
    (64, ("wh", "reg"), False),         # plain-fp32 feature map
    (64, ("wh",), True),                # reg absent
    # the other paths the entry admits: Cin in more than one chunk with a short last chunk (96 = 64 + 32,
    # 160 = 64 + 64 + 32), N = 256 on the one-slot 16-cell form, N = 384 on the two-slot form
    (128, ("wh", "reg"), True, 96),
    (192, ("wh", "reg"), True, 160),
], ids=["h64", "h256", "plain", "noreg", "h128_cin96", "h192_cin160"])
def test_heads_at_cells_against_fp64(dev, case):
    from centernet_amd import native
    hidden, names, split = case[:3]
    cin = case[3] if len(case) > 3 else C
    feat, _pb = _feature(dev, split, cin)
    pairs = _heads(hidden, names, cin=cin)
    late = _late(feat, pairs, dev)
    ref = _dense_ref(feat, pairs)
    inds = torch.tensor([[y * W + x for y, x in img] for img in CELLS], dtype=torch.int32, device=dev)
    scores = torch.linspace(0.9, 0.1, B * K, device=dev).reshape(B, K).contiguous()
    clses = (torch.arange(B * K, device=dev, dtype=torch.int32) % 5).reshape(B, K).contiguous()
    nh = len(names)
    dets = torch.empty((B, K, 6), device=dev)
    vals = torch.empty((B, K, 2 * nh), device=dev)
    native.check(native.lib().cn_ctdet_heads_at_cells_f32(
        feat.ptr(), B, H, W, cin, feat.pitch, native.DTYPE_F32S if split else native.DTYPE_F32,
        float(2.0 ** feat.exp) if split else 1.0, native.ptr(scores), native.ptr(inds), native.ptr(clses), K,
        native.ptr(late.w1), native.ptr(late.b1), hidden, nh, native.ptr(late.w2), native.ptr(late.b2),
        native.ptr(dets), native.ptr(vals), native.stream_ptr()), "cn_ctdet_heads_at_cells_f32")
    torch.cuda.synchronize()
    vals, dets = vals.cpu().double(), dets.cpu()
    worst = 0.0
    for b in range(B):
        for k, (y, x) in enumerate(CELLS[b]):
            want = torch.cat([ref[n][b, :, y, x] for n in names])
            err = ((vals[b, k] - want).abs() / (1 + want.abs())).max()
            worst = max(worst, float(err))
            # the row: same floats as the decode's arithmetic on these head values
            w_, h_ = vals[b, k, 0].float(), vals[b, k, 1].float()
            xs = torch.tensor(float(x)) + (vals[b, k, 2].float() if nh > 1 else 0.5)
            ys = torch.tensor(float(y)) + (vals[b, k, 3].float() if nh > 1 else 0.5)
            row = torch.stack([xs - w_ / 2, ys - h_ / 2, xs + w_ / 2, ys + h_ / 2])
            assert torch.equal(dets[b, k, :4], row), (b, k)
    print("heads at cells: max |diff| / (1 + |ref|) = %.3e" % worst)
    assert worst < TOL, worst
    assert torch.equal(dets[..., 4], scores.cpu()) and torch.equal(dets[..., 5], clses.cpu().float())
    # a repeated cell is simply computed again: the same bits
    assert torch.equal(vals[0, 9], vals[0, 10]) and torch.equal(vals[0, 9], vals[0, 11])


@pytest.mark.parametrize("with_reg", [True, False], ids=["reg", "noreg"])
def test_box_assembly_against_the_dense_decode(dev, with_reg):
    from centernet_amd.decode import ctdet_decode, ctdet_decode_at_cells
    feat, _pb = _feature(dev, True)
    pairs = _heads(64, ("wh", "reg") if with_reg else ("wh",), seed=3)
    late = _late(feat, pairs, dev)
    ref = _dense_ref(feat, pairs)
    heat = torch.from_numpy(synth.normal((B, 5, H, W), 1.5, 77)).to(dev)
    wh = ref["wh"].float().to(dev)
    reg = ref["reg"].float().to(dev) if with_reg else None
    want, want_inds = ctdet_decode(heat, wh, reg, K=K, apply_sigmoid=True, return_inds=True)
    got, got_inds = ctdet_decode_at_cells(heat, late, K=K, apply_sigmoid=True, return_inds=True)
    torch.cuda.synchronize()
    want, got = want.cpu(), got.cpu()
    assert torch.equal(got_inds.cpu(), want_inds.cpu())
    for col in (4, 5):      # scores, classes: bit-equal
        assert np.array_equal(got[..., col].contiguous().numpy().view(np.uint32),
                              want[..., col].contiguous().numpy().view(np.uint32))
    err = ((got[..., :4] - want[..., :4]).abs() / (1 + want[..., :4].abs())).max()
    print("box assembly: max |diff| / (1 + |value|) = %.3e" % float(err))
    assert float(err) < TOL, float(err)


def _detector(arch, extra=()):
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ctdet", "--arch", arch] + list(extra))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


def _deferred_against_dense(det, x, bit_equal_hm=True):
    """run_batch (deferred plan) against the dense plan + ``_decode`` of the same module on ``x``."""
    m = det.model
    assert m.deferred_names() == ("wh", "reg")
    Bx, _, Hx, Wx = x.shape
    dets = det.run_batch(x).clone()
    plan = m.plan_for(Bx, Hx, Wx, x.device)
    assert plan.deferred is not None and plan.deferred.names == ("wh", "reg")
    assert sorted(plan.outputs) == ["hm"]
    late_hm = m(x, deferred=True)[-1]["hm"]
    dense = m(x)[-1]
    dense_plan = m.plan_for(Bx, Hx, Wx, x.device, deferred=False)
    assert dense_plan is not plan and dense_plan.deferred is None and sorted(dense_plan.outputs) == ["hm", "reg", "wh"]
    assert len(plan.b.ops) == len(dense_plan.b.ops)            # one heads launch either way
    heads_op = [i for i, (kind, _) in enumerate(plan.b.trace) if kind == "heads"]
    assert len(heads_op) == 1
    assert plan.b.meta[heads_op[0]]["flops"] < dense_plan.b.meta[heads_op[0]]["flops"]
    if bit_equal_hm:
        assert torch.equal(late_hm, dense["hm"])
    want = det._decode(dense["hm"], dense["wh"], dense["reg"], True)
    torch.cuda.synchronize()
    assert det.range_ok()
    got, want = dets.cpu(), want.cpu()
    for col in (4, 5):
        assert np.array_equal(got[..., col].contiguous().numpy().view(np.uint32),
                              want[..., col].contiguous().numpy().view(np.uint32))
    err = ((got[..., :4] - want[..., :4]).abs() / (1 + want[..., :4].abs())).max()
    print("deferred vs dense plan: max box |diff| / (1 + |value|) = %.3e" % float(err))
    assert float(err) < TOL, float(err)


@pytest.mark.parametrize("shape", [(2, 128), (4, 512)], ids=["one_tile_per_workgroup", "persistent"])
def test_deferred_plan_against_dense_plan(dev, shape):
    """resdcn_18, f32s: (2, 3, 128, 128) runs the heads one tile per workgroup in both plans, (4, 3, 512, 512)
    on the persistent kernel in both (512 items with one head: above the 256-item threshold)."""
    n, res = shape
    det, opt = _detector("resdcn_18", ["--input_res", str(res)])
    assert det.model.uses_f32s()
    _deferred_against_dense(det, synth.images(n, res, res, seed=5).to(dev))


def test_deferred_plan_dla_34(dev):
    """The 256-wide heads end to end (both plans run them on the sliced one-tile-per-workgroup kernel)."""
    det, opt = _detector("dla_34", ["--input_res", "128"])
    _deferred_against_dense(det, synth.images(2, 128, 128, seed=6).to(dev))


@pytest.mark.parametrize("extra", [["--flip_test"], ["--cat_spec_wh"]], ids=["flip_test", "cat_spec_wh"])
def test_nothing_deferred_in_the_other_modes(dev, extra):
    det, opt = _detector("resdcn_18", ["--input_res", "128"] + extra)
    m = det.model
    assert m.deferred_names() == ()
    x = synth.images(2, 128, 128, seed=7).to(dev)
    got = det.run_batch(x).clone()
    plan = m.plan_for(2, 128, 128, x.device)
    assert plan.deferred is None and plan is m.plan_for(2, 128, 128, x.device, deferred=False)
    assert all(key[-1] == () for key in m.__dict__["_plans"])
    dense = m(x)[-1]                    # deferral never set: the module's plain forward
    want = det._decode(dense["hm"], dense["wh"], dense["reg"], True)
    torch.cuda.synchronize()
    assert det.range_ok() and torch.equal(got, want)


def test_half_compute_defers_nothing(dev):
    """fp16 compute (the hourglass configuration): the mode stays set on the module but the plan key carries no
    deferred names, and run_batch is the dense plan + the dense decode."""
    det, opt = _detector("hourglass", ["--input_res", "128"])
    m = det.model
    assert m.deferral() == ("wh", "reg") and m.deferred_names() == ("wh", "reg")
    m.half_compute()
    assert m.deferral() == ("wh", "reg") and m.deferred_names() == ()
    x = synth.images(1, 128, 128, seed=8).to(dev)
    got = det.run_batch(x).clone()
    plan = m.plan_for(1, 128, 128, x.device)
    assert plan.deferred is None and plan is m.plan_for(1, 128, 128, x.device, deferred=False)
    assert all(key[-1] == () for key in m.__dict__["_plans"])
    dense = m(x)[-1]
    want = det._decode(dense["hm"], dense["wh"], dense["reg"], True)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
