"""The gather-only multi_pose heads (wh, hps, reg) at the decoded centres: cn_multi_pose_heads_at_cells_f32,
cn_multi_pose_match_f32, decode.multi_pose_decode_at_cells and the deferred-heads plan of MultiPoseDetector.
Tolerance: the project's bar, |diff| <= 2e-5 * (1 + |ref|) against torch fp64 (tests/test_gpu_heads_at_cells.py,
DESIGN.md 3.4b); everything behind the head values is compared bit for bit."""
import contextlib
import functools
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
# four more: the second workgroup of an image then holds 4 of its 16 cells
MORE = [[(1, 6), (6, 5), (0, 8), (7, 2)], [(5, 5), (0, 9), (7, 4), (3, 10)]]


def _heads(hidden, couts, seed=0, cin=C):
    """name -> (3x3 conv + bias, 1x1 conv + bias) with ``couts`` = {name: outputs}."""
    pairs = {}
    for i, (name, cout) in enumerate(couts.items()):
        c1 = torch.nn.Conv2d(cin, hidden, 3, padding=1, bias=True)
        c2 = torch.nn.Conv2d(hidden, cout, 1, bias=True)
        with torch.no_grad():
            c1.weight.copy_(torch.from_numpy(synth.normal(tuple(c1.weight.shape), (2.0 / (cin * 9)) ** 0.5, seed + 20 + i)))
            c1.bias.copy_(torch.from_numpy(synth.normal((hidden,), 0.2, seed + 30 + i)))
            c2.weight.copy_(torch.from_numpy(synth.normal(tuple(c2.weight.shape), 0.15, seed + 40 + i)))
            c2.bias.copy_(torch.from_numpy(synth.normal((cout,), 0.5, seed + 50 + i)))
        pairs[name] = (c1, c2)
    return pairs


@functools.lru_cache(maxsize=None)
def _feature(dev, split, cin=C):
    """The feature map as the output of a PlanBuilder convolution (an f32s Act with a non-zero exponent, or the
    plain-fp32 Act of the fp32-MFMA mode), and its values in float64 NCHW on the host.  Built once per form and
    never written again."""
    from centernet_amd.engine import Act, PlanBuilder, exponent_for
    x = torch.from_numpy(synth.normal((B, cin, H, W), 1.0, 11))
    w = torch.from_numpy(synth.normal((cin, cin, 1, 1), (2.0 / cin) ** 0.5, 12))
    ef = exponent_for(float(F.conv2d(x, w).abs().max()))
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
    return feat, pb, feat.to_float().permute(0, 3, 1, 2).double().cpu()


def _dense_ref(x64, pairs):
    out = {}
    for name, (c1, c2) in pairs.items():
        h = F.relu(F.conv2d(x64, c1.weight.detach().double(), c1.bias.detach().double(), padding=1))
        out[name] = F.conv2d(h, c2.weight.detach().double(), c2.bias.detach().double())
    return out


def _late(feat, pairs, dev):
    from centernet_amd.engine import DeferredHeads, pack_cell_heads
    names = list(pairs)
    packed = pack_cell_heads([pairs[n][0] for n in names], [pairs[n][1] for n in names], dev)
    return DeferredHeads(names, feat, pairs[names[0]][0].weight.shape[0], *packed,
                         couts=[pairs[n][1].weight.shape[0] for n in names])


def _rows_from_vals(vals, inds, width, J, with_reg):
    """Stage-A columns 0..3 and 5..5+2J of multi_pose_decode in float32 numpy, one rounding per step, from the
    raw head values (B, K, 2 + 2J [+ 2]) and the cells."""
    f = np.float32
    xi, yi = (inds % width).astype(f), (inds // width).astype(f)
    w_, h_ = vals[..., 0], vals[..., 1]
    xs = xi + (vals[..., 2 + 2 * J] if with_reg else f(0.5))
    ys = yi + (vals[..., 3 + 2 * J] if with_reg else f(0.5))
    box = np.stack([xs - w_ / f(2), ys - h_ / f(2), xs + w_ / f(2), ys + h_ / f(2)], -1).astype(f)
    kps = vals[..., 2:2 + 2 * J].copy()
    kps[..., 0::2] += xi[..., None]
    kps[..., 1::2] += yi[..., None]
    return box, kps.astype(f)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", [
    dict(hidden=64, reg=True),                       # N = 192, f32s feature with a non-zero exponent
    dict(hidden=256, reg=True),                      # N = 768: past the old limit of 512, the three-slot form
    dict(hidden=256, reg=False),                     # N = 512, centre + 0.5
    dict(hidden=64, reg=True, split=False),          # plain-fp32 feature map
    dict(hidden=128, reg=True, cin=96),              # Cin = 64 + 32: the short last chunk
    dict(hidden=64, reg=True, J=3),                  # 6-output hps: rows of 12, nothing hard-wired to 17
    dict(hidden=64, reg=True, K=20),                 # second workgroup with ncell = 4 < 16
], ids=["h64", "h256_n768", "h256_noreg", "plain", "h128_cin96", "j3", "k20_partial_group"])
def test_pose_heads_at_cells_against_fp64(dev, case):
    from centernet_amd import native
    hidden, with_reg = case["hidden"], case["reg"]
    split, cin, J, k = case.get("split", True), case.get("cin", C), case.get("J", 17), case.get("K", K)
    feat, _pb, x64 = _feature(dev, split, cin)
    couts = {"wh": 2, "hps": 2 * J}
    if with_reg:
        couts["reg"] = 2
    names, nout, D = list(couts), sum(couts.values()), 5 + 2 * J + 1
    pairs = _heads(hidden, couts, cin=cin)
    late = _late(feat, pairs, dev)
    ref = _dense_ref(x64, pairs)
    cells = [CELLS[b] + (MORE[b] if k > K else []) for b in range(B)]
    assert all(len(c) == k for c in cells)
    inds = torch.tensor([[y * W + x for y, x in img] for img in cells], dtype=torch.int32, device=dev)
    scores = torch.linspace(0.9, 0.1, B * k, device=dev).reshape(B, k).contiguous()
    clses = (torch.arange(B * k, device=dev, dtype=torch.int32) % 5).reshape(B, k).contiguous()
    dets = torch.full((B, k, D), -7.0, device=dev)
    vals = torch.full((B, k, nout), -7.0, device=dev)
    native.check(native.lib().cn_multi_pose_heads_at_cells_f32(
        feat.ptr(), B, H, W, cin, feat.pitch, native.DTYPE_F32S if split else native.DTYPE_F32,
        float(2.0 ** feat.exp) if split else 1.0, native.ptr(scores), native.ptr(inds), native.ptr(clses), k,
        native.ptr(late.w1), native.ptr(late.b1), hidden, len(names), J, native.ptr(late.w2), native.ptr(late.b2),
        native.ptr(dets), native.ptr(vals), native.stream_ptr()), "cn_multi_pose_heads_at_cells_f32")
    torch.cuda.synchronize()
    vals, dets, inds_h = vals.cpu().numpy(), dets.cpu().numpy(), inds.cpu().numpy()
    worst = 0.0
    for b in range(B):
        for q, (y, x) in enumerate(cells[b]):
            want = torch.cat([ref[n][b, :, y, x] for n in names]).numpy()
            worst = max(worst, float((np.abs(vals[b, q].astype(np.float64) - want) / (1 + np.abs(want))).max()))
    print("pose heads at cells: max |diff| / (1 + |ref|) = %.3e" % worst)
    assert worst < TOL, worst
    # the rows: the decode's float32 arithmetic on these head values, bit for bit
    box, kps = _rows_from_vals(vals, inds_h, W, J, with_reg)
    assert np.array_equal(_bits(dets[..., :4]), _bits(box))
    assert np.array_equal(_bits(dets[..., 5:5 + 2 * J]), _bits(kps))
    assert np.array_equal(_bits(dets[..., 4]), _bits(scores.cpu().numpy()))
    assert np.array_equal(_bits(dets[..., D - 1]), _bits(clses.cpu().numpy().astype(np.float32)))
    # a repeated cell is simply computed again: the same bits
    assert np.array_equal(_bits(vals[0, 9]), _bits(vals[0, 10])) and np.array_equal(_bits(vals[0, 9]), _bits(vals[0, 11]))
    assert np.array_equal(_bits(dets[0, 9, :4]), _bits(dets[0, 11, :4]))


def test_pose_cell_outside_the_map_gives_a_nan_row(dev):
    from centernet_amd import native
    feat, _pb, _x = _feature(dev, True)
    J, D, nout = 17, 40, 38
    late = _late(feat, _heads(64, {"wh": 2, "hps": 34, "reg": 2}), dev)
    inds = torch.tensor([[5, -1, H * W, 17]] * B, dtype=torch.int32, device=dev)
    scores = torch.rand((B, 4), device=dev)
    clses = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    dets, vals = torch.zeros((B, 4, D), device=dev), torch.zeros((B, 4, nout), device=dev)
    native.check(native.lib().cn_multi_pose_heads_at_cells_f32(
        feat.ptr(), B, H, W, C, feat.pitch, native.DTYPE_F32S, float(2.0 ** feat.exp), native.ptr(scores),
        native.ptr(inds), native.ptr(clses), 4, native.ptr(late.w1), native.ptr(late.b1), 64, 3, J,
        native.ptr(late.w2), native.ptr(late.b2), native.ptr(dets), native.ptr(vals), native.stream_ptr()),
        "cn_multi_pose_heads_at_cells_f32")
    torch.cuda.synchronize()
    dets, vals = dets.cpu(), vals.cpu()
    assert torch.equal(dets[..., 4], scores.cpu()) and torch.equal(dets[..., 39], clses.cpu().float())
    coords = torch.cat([dets[..., :4], dets[..., 5:39]], -1)
    assert torch.isnan(coords[:, 1:3]).all() and torch.isnan(vals[:, 1:3]).all()
    assert torch.isfinite(coords[:, 0]).all() and torch.isfinite(coords[:, 3]).all()
    assert torch.isfinite(vals[:, 0]).all() and torch.isfinite(vals[:, 3]).all()


def _scatter(vals, inds, cols, height, width):
    """(B, K, n) head values at the cells ``inds`` (B, K) -> zero-filled dense (B, len(cols), H, W) map."""
    b, k = inds.shape
    m = torch.zeros((b, len(cols), height * width), device=vals.device, dtype=torch.float32)
    m.scatter_(2, inds[:, None, :].expand(b, len(cols), k), vals[..., cols].permute(0, 2, 1).contiguous())
    return m.reshape(b, len(cols), height, width)


def _dense_from_cells(heat, vals, inds, J, with_reg, hm_hp, hp_offset, k):
    """The existing dense decode on maps that hold the cells kernel's head values at the decoded cells."""
    from centernet_amd.decode import multi_pose_decode
    hh, ww = heat.shape[2:]
    for b in range(inds.shape[0]):
        assert len(set(inds[b].tolist())) == inds.shape[1]          # top-K cells of an image are distinct
    wh = _scatter(vals, inds, [0, 1], hh, ww)
    hps = _scatter(vals, inds, list(range(2, 2 + 2 * J)), hh, ww)
    reg = _scatter(vals, inds, [2 + 2 * J, 3 + 2 * J], hh, ww) if with_reg else None
    return multi_pose_decode(heat, wh, hps, reg=reg, hm_hp=hm_hp, hp_offset=hp_offset, K=k, apply_sigmoid=True)


@pytest.fixture(scope="module")
def decode_inputs(dev):
    """Random centre logits (with a lattice of raised cells, so that an image has more than K peaks and no
    top-K place is filled by a zero score), joint logits scaled so that candidate scores fall on both sides of
    the 0.1 threshold, joint offsets; one set of heads, with and without ``reg``."""
    heat = synth.normal((B, 1, H, W), 1.0, 71)
    heat[:, :, ::2, ::2] += 3.0 + np.abs(synth.normal((B, 1, H // 2, W // 2), 1.0, 72))
    hm_hp = synth.normal((B, 17, H, W), 2.5, 73) - 1.5
    hp_offset = synth.normal((B, 2, H, W), 0.3, 74)
    feat, _pb, _x = _feature(dev, True)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    lates = {}
    for r in (True, False):
        pairs = _heads(64, dict([("wh", 2), ("hps", 34)] + ([("reg", 2)] if r else [])), seed=3)
        with torch.no_grad():
            pairs["wh"][1].bias.copy_(torch.tensor([6.0, 5.0]))     # boxes of several cells: joints can match
        lates[r] = _late(feat, pairs, dev)
    return to(heat), to(hm_hp), to(hp_offset), lates


@pytest.mark.parametrize("form", ["full", "no_hp_offset", "stage_a", "noreg"])
def test_pose_decode_at_cells_bit_for_bit(dev, decode_inputs, form):
    from centernet_amd.decode import multi_pose_decode_at_cells
    heat, hm_hp, hp_offset, lates = decode_inputs
    with_reg = form != "noreg"
    late = lates[with_reg]
    hh = None if form == "stage_a" else hm_hp
    ho = None if form in ("stage_a", "no_hp_offset") else hp_offset
    got, inds, vals = multi_pose_decode_at_cells(heat, late, hm_hp=hh, hp_offset=ho, K=K, apply_sigmoid=True,
                                                 return_inds=True, return_vals=True)
    assert got.shape == (B, K, 40) and vals.shape == (B, K, 38 if with_reg else 36)
    want = _dense_from_cells(heat, vals, inds, 17, with_reg, hh, ho, K)
    torch.cuda.synchronize()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert (got[..., 4] > 0).all()
    assert np.array_equal(_bits(got), _bits(want))
    if hh is not None:
        # both outcomes of the match occur: joints snapped to a candidate and joints kept at the regression
        stage_a = multi_pose_decode_at_cells(heat, late, K=K, apply_sigmoid=True).cpu().numpy()
        moved = _bits(got[..., 5:39]) != _bits(stage_a[..., 5:39])
        joint_moved = moved.reshape(B, K, 17, 2).any(-1)
        print("joints snapped %d, kept %d" % (joint_moved.sum(), (~joint_moved).sum()))
        assert joint_moved.any() and (~joint_moved).any()
        # candidate scores on both sides of the threshold
        s = torch.sigmoid(hm_hp).cpu().numpy()
        assert (s > 0.1).any() and (s < 0.1).any()
        assert np.array_equal(_bits(got[..., :5]), _bits(stage_a[..., :5]))


def test_pose_decode_at_cells_refuses_other_heads(dev, decode_inputs):
    from centernet_amd.decode import multi_pose_decode_at_cells
    heat, _hm_hp, _off, _lates = decode_inputs
    feat, _pb, _x = _feature(dev, True)
    late = _late(feat, _heads(64, {"wh": 2, "reg": 2}), dev)
    with pytest.raises(RuntimeError, match="takes the heads"):
        multi_pose_decode_at_cells(heat, late, K=K)


# ---------------------------------------------------------------------------------------------- the detector
def _detector(arch, extra=()):
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["multi_pose", "--arch", arch] + list(extra))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


def _dense_decode(det, o):
    from centernet_amd.decode import multi_pose_decode
    opt = det.opt
    return multi_pose_decode(o["hm"], o["wh"], o["hps"], reg=o["reg"] if opt.reg_offset else None,
                             hm_hp=o["hm_hp"] if opt.hm_hp else None,
                             hp_offset=o["hp_offset"] if opt.reg_hp_offset else None, K=opt.K, apply_sigmoid=True)


# K = 40: three cell groups per image, the last one partial; 32 x 32 cells hold more than 40 peaks
@pytest.mark.parametrize("arch", ["resdcn_18", "dla_34"])
def test_deferred_pose_plan_against_dense_plan(dev, arch):
    from centernet_amd.decode import multi_pose_decode, multi_pose_decode_at_cells
    det, opt = _detector(arch, ["--input_res", "128", "--K", "40"])
    m = det.model
    assert m.uses_f32s() and m.deferred_names() == ("wh", "hps", "reg")
    x = synth.images(2, 128, 128, seed=5).to(dev)
    dets = det.run_batch(x).clone()
    plan = m.plan_for(2, 128, 128, x.device)
    assert plan.deferred is not None and plan.deferred.names == ("wh", "hps", "reg")
    assert plan.deferred.couts == (2, 34, 2)
    assert sorted(plan.outputs) == ["hm", "hm_hp", "hp_offset"]
    late_out = m(x, deferred=True)[-1]
    late = late_out["_deferred"]
    # stage A of the deferred plan, while its feature map is still the one of this forward
    a_got, inds, vals = multi_pose_decode_at_cells(late_out["hm"], late, K=opt.K, apply_sigmoid=True,
                                                   return_inds=True, return_vals=True)
    a_got, inds, vals = a_got.clone(), inds.clone(), vals.clone()
    dense = m(x)[-1]
    dense_plan = m.plan_for(2, 128, 128, x.device, deferred=False)
    assert dense_plan is not plan and dense_plan.deferred is None
    assert sorted(dense_plan.outputs) == ["hm", "hm_hp", "hp_offset", "hps", "reg", "wh"]
    assert len(plan.b.ops) == len(dense_plan.b.ops)            # one heads launch either way
    heads_op = [i for i, (kind, _) in enumerate(plan.b.trace) if kind == "heads"]
    assert len(heads_op) == 1
    assert [i for i, (kind, _) in enumerate(dense_plan.b.trace) if kind == "heads"] == heads_op
    assert plan.b.meta[heads_op[0]]["flops"] < dense_plan.b.meta[heads_op[0]]["flops"]
    # calibration is dense in both plans (one hidden exponent over all six heads): the same bits
    for name in ("hm", "hm_hp", "hp_offset"):
        assert torch.equal(late_out[name], dense[name]), name
    a_want = multi_pose_decode(dense["hm"], dense["wh"], dense["hps"], reg=dense["reg"], K=opt.K,
                               apply_sigmoid=True)
    want = _dense_from_cells(dense["hm"], vals, inds, 17, True, dense["hm_hp"], dense["hp_offset"], opt.K)
    torch.cuda.synchronize()
    assert det.range_ok()
    a_got, a_want = a_got.cpu().numpy(), a_want.cpu().numpy()
    for col in (4, 39):
        assert np.array_equal(_bits(a_got[..., col]), _bits(a_want[..., col]))
    err = (np.abs(a_got - a_want) / (1 + np.abs(a_want))).max()
    print("%s deferred vs dense plan, stage A: max |diff| / (1 + |value|) = %.3e" % (arch, float(err)))
    assert float(err) < TOL, float(err)
    assert np.array_equal(_bits(dets.cpu().numpy()), _bits(want.cpu().numpy()))


def test_nothing_deferred_with_flip_test(dev):
    det, opt = _detector("resdcn_18", ["--input_res", "128", "--flip_test"])
    m = det.model
    assert m.deferred_names() == ()
    x = synth.images(2, 128, 128, seed=7).to(dev)
    got = det.run_batch(x).clone()
    plan = m.plan_for(2, 128, 128, x.device)
    assert plan.deferred is None and plan is m.plan_for(2, 128, 128, x.device, deferred=False)
    assert all(key[-1] == () for key in m.__dict__["_plans"])
    want = _dense_decode(det, m(x)[-1])
    torch.cuda.synchronize()
    assert det.range_ok() and torch.equal(got, want)


def test_half_compute_defers_nothing(dev):
    det, opt = _detector("hourglass", ["--input_res", "128"])
    m = det.model
    assert m.deferral() == ("wh", "hps", "reg") and m.deferred_names() == ("wh", "hps", "reg")
    m.half_compute()
    assert m.deferral() == ("wh", "hps", "reg") and m.deferred_names() == ()
    x = synth.images(1, 128, 128, seed=8).to(dev)
    got = det.run_batch(x).clone()
    plan = m.plan_for(1, 128, 128, x.device)
    assert plan.deferred is None and plan is m.plan_for(1, 128, 128, x.device, deferred=False)
    assert all(key[-1] == () for key in m.__dict__["_plans"])
    want = _dense_decode(det, m(x)[-1])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
