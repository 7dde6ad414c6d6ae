"""The gather-only ddd heads (dep, rot, dim, wh, reg) at the decoded centres: cn_ddd_heads_at_cells_f32,
decode.ddd_decode_at_cells and the deferred-heads plan of DddDetector.
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
# four more: the second cell group of an image then holds 4 of its 16 cells
MORE = [[(1, 6), (6, 5), (0, 8), (7, 2)], [(5, 5), (0, 9), (7, 4), (3, 10)]]
COUTS = {"dep": 1, "rot": 8, "dim": 3, "wh": 2, "reg": 2}
COL = {"dep": 11, "rot": 3, "dim": 12, "wh": 15, "reg": 0}     # first column of a head in a row of ddd_decode


def _couts(wh=True, reg=True):
    return {n: c for n, c in COUTS.items() if (n != "wh" or wh) and (n != "reg" or reg)}


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


@functools.lru_cache(maxsize=None)
def _dense_ref(dev, split, cin, hidden, wh, reg):
    """fp64 dense heads on the feature map: computed once per head set and left unchanged."""
    _feat, _pb, x64 = _feature(dev, split, cin)
    out = {}
    for name, (c1, c2) in _heads(hidden, _couts(wh, reg), cin=cin).items():
        h = F.relu(F.conv2d(x64, c1.weight.detach().double(), c1.bias.detach().double(), padding=1))
        out[name] = F.conv2d(h, c2.weight.detach().double(), c2.bias.detach().double())
    return out


def _late(feat, pairs, dev, sizes=None):
    from centernet_amd.engine import DeferredHeads, cell_head_group_sizes, pack_cell_head_groups
    names = list(pairs)
    hidden = pairs[names[0]][0].weight.shape[0]
    if sizes is None:
        sizes = cell_head_group_sizes(len(names), hidden, wide=False)
    groups = pack_cell_head_groups([pairs[n][0] for n in names], [pairs[n][1] for n in names], dev, sizes)
    return DeferredHeads(names, feat, hidden, couts=[pairs[n][1].weight.shape[0] for n in names], groups=groups)


def _call(late, feat, split, cin, scores, inds, clses, k, dets, vals, flags=0):
    from centernet_amd import native
    native.check(native.lib().cn_ddd_heads_at_cells_f32(
        feat.ptr(), B, H, W, cin, feat.pitch, native.DTYPE_F32S if split else native.DTYPE_F32,
        float(2.0 ** feat.exp) if split else 1.0, native.ptr(scores), native.ptr(inds), native.ptr(clses), k,
        late.hidden, len(late.groups), late.group_table(), int("wh" in late.names), int("reg" in late.names), flags,
        native.ptr(dets), native.ptr(vals), native.stream_ptr()), "cn_ddd_heads_at_cells_f32")
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _voff(names):
    off, at = {}, 0
    for n in names:
        off[n] = at
        at += COUTS[n]
    return off


@pytest.mark.parametrize("case", [
    dict(hidden=64),                                  # N = 64 per group: the form ctdet alone instantiated so far
    dict(hidden=256),                                 # dla_34's width
    dict(hidden=128, cin=96),                         # Cin = 64 + 32: the short last chunk
    dict(hidden=64, split=False),                     # plain-fp32 feature map
    dict(hidden=64, wh=False),                        # rows of 16
    dict(hidden=64, reg=False),                       # centre + 0.5, written by group 0
    dict(hidden=64, K=20),                            # second cell group with ncell = 4 < 16
    dict(hidden=64, sizes=(5,)),                      # the other grouping: all five heads in one group
    dict(hidden=64, sizes=(3, 2)),                    # the widest groups the entry takes: N = 192 and 128
    dict(hidden=128, sizes=(3, 2)),                   # N = 384: the two-slot form
    dict(hidden=256, sizes=(3, 2)),                   # N = 768 and 512 on the three-slot form
], ids=["h64", "h256", "h128_cin96", "plain", "no_wh", "no_reg", "k20_partial_group", "h64_one_group_of_five",
        "h64_wide", "h128_wide", "h256_wide"])
def test_ddd_heads_at_cells_against_fp64(dev, case):
    from centernet_amd import native
    hidden, with_wh, with_reg = case["hidden"], case.get("wh", True), case.get("reg", True)
    split, cin, k, sizes = case.get("split", True), case.get("cin", C), case.get("K", K), case.get("sizes")
    if sizes is not None and max(sizes) > native.CELL_GROUP_MAX_HEADS:
        pytest.skip("not shipped: cn_ddd_heads_at_cells_f32 takes at most %d heads per group"
                    % native.CELL_GROUP_MAX_HEADS)
    feat, _pb, _x64 = _feature(dev, split, cin)
    couts = _couts(with_wh, with_reg)
    names, nout, D = list(couts), sum(couts.values()), 18 if with_wh else 16
    late = _late(feat, _heads(hidden, couts, cin=cin), dev, sizes)
    ref = _dense_ref(dev, split, cin, hidden, with_wh, with_reg)
    cells = [CELLS[b] + (MORE[b] if k > K else []) for b in range(B)]
    assert all(len(c) == k for c in cells)
    inds = torch.tensor([[y * W + x for y, x in img] for img in cells], dtype=torch.int32, device=dev)
    scores = torch.linspace(0.9, 0.1, B * k, device=dev).reshape(B, k).contiguous()
    clses = (torch.arange(B * k, device=dev, dtype=torch.int32) % 3).reshape(B, k).contiguous()
    dets = torch.full((B, k, D), -7.0, device=dev)
    vals = torch.full((B, k, nout), -7.0, device=dev)
    _call(late, feat, split, cin, scores, inds, clses, k, dets, vals)
    vals, dets, inds_h = vals.cpu().numpy(), dets.cpu().numpy(), inds.cpu().numpy()
    worst = 0.0
    for b in range(B):
        for q, (y, x) in enumerate(cells[b]):
            want = torch.cat([ref[n][b, :, y, x] for n in names]).numpy()
            worst = max(worst, float((np.abs(vals[b, q].astype(np.float64) - want) / (1 + np.abs(want))).max()))
    print("ddd heads at cells: max |diff| / (1 + |ref|) = %.3e" % worst)
    assert worst < TOL, worst
    # the rows: ddd_decode's float32 arithmetic on these head values, bit for bit
    f, off = np.float32, _voff(names)
    xi, yi = (inds_h % W).astype(f), (inds_h // W).astype(f)
    xs = xi + (vals[..., off["reg"]] if with_reg else f(0.5))          # a single add
    ys = yi + (vals[..., off["reg"] + 1] if with_reg else f(0.5))
    assert np.array_equal(_bits(dets[..., 0]), _bits(xs)) and np.array_equal(_bits(dets[..., 1]), _bits(ys))
    for n in names:
        if n != "reg":                                                  # copied; depth raw with the flag off
            assert np.array_equal(_bits(dets[..., COL[n]:COL[n] + COUTS[n]]),
                                  _bits(vals[..., off[n]:off[n] + COUTS[n]])), n
    assert np.array_equal(_bits(dets[..., 2]), _bits(scores.cpu().numpy()))
    assert np.array_equal(_bits(dets[..., D - 1]), _bits(clses.cpu().numpy().astype(np.float32)))
    # a repeated cell is simply computed again: the same bits
    assert np.array_equal(_bits(vals[0, 9]), _bits(vals[0, 10])) and np.array_equal(_bits(vals[0, 9]), _bits(vals[0, 11]))
    assert np.array_equal(_bits(dets[0, 9, [0, 1] + list(range(3, D - 1))]),
                          _bits(dets[0, 11, [0, 1] + list(range(3, D - 1))]))


@pytest.mark.parametrize("with_reg", [True, False], ids=["reg", "noreg"])
def test_ddd_cell_outside_the_map_gives_nan_columns(dev, with_reg):
    from centernet_amd import native
    feat, _pb, _x = _feature(dev, True)
    couts = _couts(True, with_reg)
    nout, D = sum(couts.values()), 18
    late = _late(feat, _heads(64, couts), dev)
    inds = torch.tensor([[5, -1, H * W, 17]] * B, dtype=torch.int32, device=dev)
    scores = torch.rand((B, 4), device=dev)
    clses = torch.ones((B, 4), dtype=torch.int32, device=dev)
    dets, vals = torch.zeros((B, 4, D), device=dev), torch.zeros((B, 4, nout), device=dev)
    _call(late, feat, True, C, scores, inds, clses, 4, dets, vals, flags=native.DECODE_DDD_RAW_DEPTH)
    dets, vals = dets.cpu(), vals.cpu()
    assert torch.equal(dets[..., 2], scores.cpu()) and torch.equal(dets[..., D - 1], clses.cpu().float())
    head_cols = torch.cat([dets[..., :2], dets[..., 3:D - 1]], -1)
    assert torch.isnan(head_cols[:, 1:3]).all() and torch.isnan(vals[:, 1:3]).all()
    assert torch.isfinite(head_cols[:, 0]).all() and torch.isfinite(head_cols[:, 3]).all()
    assert torch.isfinite(vals[:, 0]).all() and torch.isfinite(vals[:, 3]).all()


def _scatter(vals, inds, cols, height, width):
    """(B, K, n) head values at the cells ``inds`` (B, K) -> zero-filled dense (B, len(cols), H, W) map."""
    b, k = inds.shape
    m = torch.zeros((b, len(cols), height * width), device=vals.device, dtype=torch.float32)
    m.scatter_(2, inds[:, None, :].expand(b, len(cols), k), vals[..., cols].permute(0, 2, 1).contiguous())
    return m.reshape(b, len(cols), height, width)


def _dense_from_cells(heat, vals, inds, names, k, raw_depth, distinct=True):
    """The existing dense decode on maps that hold the cells kernel's head values at the decoded cells.
    ``distinct=False``: a cell may win in two classes (a network's own heat-map); it then carries the same head
    values both times, bit for bit, so the scattered maps are still well defined."""
    from centernet_amd.decode import ddd_decode
    hh, ww = heat.shape[2:]
    for b in range(inds.shape[0]):
        if distinct:
            assert len(set(inds[b].tolist())) == inds.shape[1]      # the K cells of an image are distinct
    off = _voff(names)
    m = {n: _scatter(vals, inds, list(range(off[n], off[n] + COUTS[n])), hh, ww) for n in names}
    return ddd_decode(heat, m["rot"], m["dep"], m["dim"], wh=m.get("wh"), reg=m.get("reg"), K=k,
                      apply_sigmoid=True, raw_depth=raw_depth)


@pytest.fixture(scope="module")
def decode_inputs(dev):
    """Centre logits of three classes: a quiet background and a lattice of raised cells, each raised in one class
    only, so that an image has more than K peaks, no top-K place is filled by a zero score and no cell is
    taken twice; one set of heads per form."""
    heat = 0.3 * synth.normal((B, 3, H, W), 1.0, 71)
    bump = 3.0 + np.abs(synth.normal((B, H // 2, W // 2), 1.0, 72))
    for y in range(0, H, 2):
        for x in range(0, W, 2):
            heat[:, (y // 2 + x // 2) % 3, y, x] += bump[:, y // 2, x // 2]
    feat, _pb, _x = _feature(dev, True)
    lates = {}
    for form, (wh, reg) in (("full", (True, True)), ("noreg", (True, False)), ("nowh", (False, True))):
        lates[form] = _late(feat, _heads(64, _couts(wh, reg), seed=3), dev)
    return torch.from_numpy(np.ascontiguousarray(heat, dtype=np.float32)).to(dev), lates


@pytest.mark.parametrize("raw_depth", [True, False], ids=["raw_depth", "depth_as_is"])
@pytest.mark.parametrize("form", ["full", "noreg", "nowh"])
def test_ddd_decode_at_cells_bit_for_bit(dev, decode_inputs, form, raw_depth):
    from centernet_amd.decode import ddd_decode_at_cells
    heat, lates = decode_inputs
    late = lates[form]
    got, inds, vals = ddd_decode_at_cells(heat, late, K=K, apply_sigmoid=True, raw_depth=raw_depth,
                                          return_inds=True, return_vals=True)
    D = 16 if form == "nowh" else 18
    assert got.shape == (B, K, D) and vals.shape == (B, K, sum(late.couts))
    want = _dense_from_cells(heat, vals, inds, late.names, K, raw_depth)
    torch.cuda.synchronize()
    got, want, vals = got.cpu().numpy(), want.cpu().numpy(), vals.cpu().numpy()
    assert (got[..., 2] > 0.5).all()                                # raised cells only
    assert np.array_equal(_bits(got), _bits(want))
    # the flag reaches column 11 and nothing else: the head's values hold both signs, the transform is positive
    same = np.array_equal(_bits(got[..., 11]), _bits(vals[..., 0]))
    assert same != raw_depth
    only = ddd_decode_at_cells(heat, late, K=K, apply_sigmoid=True, raw_depth=raw_depth)
    assert np.array_equal(_bits(only.cpu().numpy()), _bits(got))   # without head_vals: the same rows


def test_ddd_decode_at_cells_refuses_other_heads(dev, decode_inputs):
    from centernet_amd.decode import ddd_decode_at_cells
    from centernet_amd.engine import DeferredHeads, pack_cell_heads
    heat, lates = decode_inputs
    feat, _pb, _x = _feature(dev, True)
    pairs = _heads(64, {"wh": 2, "reg": 2})
    with pytest.raises(RuntimeError, match="takes the heads"):
        ddd_decode_at_cells(heat, _late(feat, pairs, dev), K=K)
    one = DeferredHeads(list(pairs), feat, 64, *pack_cell_heads([pairs[n][0] for n in pairs],
                                                                 [pairs[n][1] for n in pairs], dev))
    with pytest.raises(RuntimeError, match="takes the heads"):
        ddd_decode_at_cells(heat, one, K=K)
    with pytest.raises(RuntimeError, match="k out of range"):
        ddd_decode_at_cells(heat, lates["full"], K=H * W + 1)
    with pytest.raises(RuntimeError, match="feature map"):
        ddd_decode_at_cells(heat[:, :, :4].contiguous(), lates["full"], K=K)


# ---------------------------------------------------------------------------------------------- the detector
def _detector(arch, extra=()):
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["ddd", "--arch", arch, "--input_h", "128", "--input_w", "384"] + list(extra))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


def _dense_run_batch(det, o):
    """run_batch's dense code on the maps of a dense forward"""
    from centernet_amd.decode import ddd_decode
    dep = 1. / (o["dep"].sigmoid() + 1e-6) - 1.
    return ddd_decode(o["hm"], o["rot"], dep, o["dim"], wh=o["wh"] if det.opt.reg_bbox else None,
                      reg=o["reg"] if det.opt.reg_offset else None, K=det.opt.K, apply_sigmoid=True)


ALL = ("dep", "rot", "dim", "wh", "reg")


# K = 40: three cell groups per image, the last one partial; 32 x 96 cells.  The batch sizes: `hm` is the same bits
# in both plans when both run the heads launch on the same kernel form (as for ctdet, tests/test_gpu_heads_at_cells.py).
# The 256-wide heads of dla_34 have one form.  The 64-wide heads of resdcn_18 have two, chosen by the launch's item
# count, batch x 24 tiles x heads launched, against 256: one image is below it with one head and with six (both plans
# one tile per workgroup), twelve images are above it with one head already (both plans on the persistent kernel);
# in between (two images: 48 against 288 items) the plans run different forms, whose sums differ in the last bits.
@pytest.mark.parametrize("arch, n", [("dla_34", 2), ("resdcn_18", 1), ("resdcn_18", 12)],
                         ids=["dla_34", "resdcn_18_one_tile_per_workgroup", "resdcn_18_persistent"])
def test_deferred_ddd_plan_against_dense_plan(dev, arch, n):
    from centernet_amd.decode import ddd_decode, ddd_decode_at_cells
    det, opt = _detector(arch, ["--K", "40"])
    m = det.model
    assert m.uses_f32s() and m.deferred_names() == ALL
    x = synth.images(n, 128, 384, seed=5).to(dev)
    dets = det.run_batch(x).clone()
    plan = m.plan_for(n, 128, 384, x.device)
    assert plan.deferred is not None and plan.deferred.names == ALL
    assert plan.deferred.couts == (1, 8, 3, 2, 2) and plan.deferred.hidden == (256 if arch == "dla_34" else 64)
    assert [g[4] for g in plan.deferred.groups] == [1, 1, 1, 1, 1]
    assert sorted(plan.outputs) == ["hm"]
    late_out = m(x, deferred=True)[-1]
    late = late_out["_deferred"]
    # the deferred plan's rows with their cells and head values, while its feature map is this forward's
    got, inds, vals = ddd_decode_at_cells(late_out["hm"], late, K=opt.K, apply_sigmoid=True, raw_depth=True,
                                          return_inds=True, return_vals=True)
    got, inds, vals, late_hm = got.clone(), inds.clone(), vals.clone(), late_out["hm"].clone()
    dense = m(x)[-1]
    dense_plan = m.plan_for(n, 128, 384, x.device, deferred=False)
    assert dense_plan is not plan and dense_plan.deferred is None
    assert sorted(dense_plan.outputs) == ["dep", "dim", "hm", "reg", "rot", "wh"]
    assert len(plan.b.ops) == len(dense_plan.b.ops)            # one heads launch either way
    heads_op = [i for i, (kind, _) in enumerate(plan.b.trace) if kind == "heads"]
    assert len(heads_op) == 1
    assert [i for i, (kind, _) in enumerate(dense_plan.b.trace) if kind == "heads"] == heads_op
    assert plan.b.meta[heads_op[0]]["flops"] < dense_plan.b.meta[heads_op[0]]["flops"]
    # calibration is dense in both plans (one hidden exponent over all six heads): the same bits
    assert torch.equal(late_hm, dense["hm"])
    want = ddd_decode(dense["hm"], dense["rot"], dense["dep"], dense["dim"], wh=dense["wh"], reg=dense["reg"],
                      K=opt.K, apply_sigmoid=True, raw_depth=True)
    on_vals = _dense_from_cells(dense["hm"], vals, inds, ALL, opt.K, True, distinct=False)
    torch.cuda.synchronize()
    assert det.range_ok()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    for col in (2, 17):
        assert np.array_equal(_bits(got[..., col]), _bits(want[..., col]))
    err = (np.abs(got - want) / (1 + np.abs(want))).max()
    print("%s B = %d deferred vs dense plan: max |diff| / (1 + |value|) = %.3e" % (arch, n, float(err)))
    assert float(err) < TOL, float(err)
    assert np.array_equal(_bits(dets.cpu().numpy()), _bits(got))
    assert np.array_equal(_bits(dets.cpu().numpy()), _bits(on_vals.cpu().numpy()))


def test_nothing_deferred_above_128_rows(dev):
    """--K 130 defers nothing: the plan run_batch asks for is the dense plan with all six maps, and run_batch is the
    dense decode on them.  As the library stands, every image-level decode refuses more than 128 rows
    (cn_ddd_decode_f32 returns "unsupported"; K > 128 is nobody's path yet), so the dense decode of these maps
    raises and run_batch raises the same; should the decode take 130 rows one day, the rows are compared."""
    from centernet_amd import native
    det, opt = _detector("resdcn_18", ["--K", "130"])
    m = det.model
    assert m.deferral() == () and m.deferred_names() == ()
    x = synth.images(2, 128, 384, seed=7).to(dev)
    late_out = m(x, deferred=True)[-1]
    assert sorted(late_out) == ["dep", "dim", "hm", "reg", "rot", "wh"]
    late_out = {k: v.clone() for k, v in late_out.items()}
    plan = m.plan_for(2, 128, 384, x.device)
    assert plan.deferred is None and plan is m.plan_for(2, 128, 384, x.device, deferred=False)
    assert all(key[-1] == () for key in m.__dict__["_plans"])
    dense = m(x)[-1]
    assert all(torch.equal(late_out[k], dense[k]) for k in dense)
    try:
        want = _dense_run_batch(det, dense)
    except native.NativeError as e:
        assert "cn_ddd_decode_f32" in str(e)
        with pytest.raises(native.NativeError, match="cn_ddd_decode_f32"):
            det.run_batch(x)
        return
    got = det.run_batch(x)
    torch.cuda.synchronize()
    assert got.shape == (2, 130, 18) and det.range_ok() and torch.equal(got, want)


def test_half_compute_defers_nothing(dev):
    det, opt = _detector("hourglass", ["--K", "40"])
    m = det.model
    assert m.deferral() == ALL and m.deferred_names() == ALL
    m.half_compute()
    assert m.deferral() == ALL and m.deferred_names() == ()
    x = synth.images(1, 128, 384, seed=8).to(dev)
    got = det.run_batch(x).clone()
    plan = m.plan_for(1, 128, 384, x.device)
    assert plan.deferred is None and plan is m.plan_for(1, 128, 384, x.device, deferred=False)
    assert all(key[-1] == () for key in m.__dict__["_plans"])
    want = _dense_run_batch(det, m(x)[-1])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
