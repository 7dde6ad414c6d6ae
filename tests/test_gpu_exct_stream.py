"""The streaming exct / agnex grouping on the GPU (cn_exct_decode_stream_f32, cn_agnex_ct_decode_stream_f32): the
stored form's rows bit for bit wherever both run, the blocked host reference (tests/exct_stream_ref.py) and the
reference's own goldens beyond K = 64, ties cut by num_dets, batches, determinism, a captured graph, the refusals
of the C ABI and the exdet detector under --ex_stream."""
import contextlib
import sys

import numpy as np
import pytest
import torch

import exct_stream_ref as SR
from centernet_amd import decode as D, native, synth
from oracle import cref
from test_exct_stream_host import BIGK, BIGK_GOLD
from test_oracle_agnex import GEN as AGEN, GOLD as AGOLD
from test_oracle_exct import GEN, GOLD, assert_same

pytestmark = pytest.mark.gpu

CN_ERR_SHAPE, CN_ERR_UNSUPPORTED, CN_ERR_WORKSPACE, CN_ERR_NULL = -1, -2, -3, -5


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(fn, heats, regs, dev, **kw):
    return fn(*[_t(h, dev) for h in heats], *[_t(r, dev) for r in regs], **kw).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# 1. the same rows as the stored form
# ------------------------------------------------------------------------------------------------
SMALL_CASES = sorted(GEN.EXCT_CASES) + sorted(GEN.AGGR_CASES) + sorted(AGEN.AGNEX_CASES)      # K = 5, 6, 40


def _small_case(name):
    """(device entry, oracle, inputs, aggr_weight, the reference's rows)"""
    if name in AGEN.AGNEX_CASES:
        return D.agnex_ct_decode, cref.agnex_ct_decode, AGEN.agnex_inputs(name), 0.0, AGOLD[name + "/dets"]
    base, w = GEN.AGGR_CASES.get(name, (name, 0.0))
    return D.exct_decode, cref.exct_decode, GEN.exct_inputs(base), w, GOLD[name + "/dets"]


@pytest.mark.parametrize("name", SMALL_CASES)
def test_stream_equals_stored_and_oracle(dev, name):
    fn, oracle, (heats, regs, K, num_dets), w, gold = _small_case(name)
    kw = dict(K=K, num_dets=num_dets, aggr_weight=w)
    stream = _run(fn, heats, regs, dev, stream=True, **kw)
    stored = _run(fn, heats, regs, dev, stream=False, **kw)
    assert _same_bits(stream, stored)
    assert _same_bits(stream, oracle(*heats, *regs, **kw))
    assert_same(stream, gold)


def test_partial_regression_behaves_like_none(dev):
    """decode.py:372-373: the offsets are applied only when all four maps are given."""
    heats, regs, K, num_dets = GEN.exct_inputs("exct_small")
    got = _run(D.exct_decode, heats, [regs[0], None, regs[2], regs[3]], dev, K=K, num_dets=num_dets, stream=True)
    assert _same_bits(got, cref.exct_decode(*heats, None, None, None, None, K=K, num_dets=num_dets))


# ------------------------------------------------------------------------------------------------
# 2. beyond the stored form: K = 65, the reference's goldens at K = 72, 100, 128
# ------------------------------------------------------------------------------------------------
def _construction(cases):
    """exct_small's input construction (tests/golden/gen_golden_exct.py) over another case table."""
    return BIGK._sibling("gen_golden_exct", "EXCT_CASES", cases)


@pytest.mark.parametrize("num_dets", [60, 1024])
def test_first_k_the_stored_form_refuses(dev, num_dets):
    heats, regs, K, _ = _construction({"exct_small": (1, 3, 24, 32, 65, num_dets, True)}).exct_inputs("exct_small")
    assert K == 65 and heats[0].shape == (1, 3, 24, 32)
    got = _run(D.exct_decode, heats, regs, dev, K=K, num_dets=num_dets)           # stream=None: the streaming form
    assert _same_bits(got, SR.exct_decode(*heats, *regs, K=K, num_dets=num_dets))
    with pytest.raises(RuntimeError):
        _run(D.exct_decode, heats, regs, dev, K=K, num_dets=num_dets, stream=False)
    with pytest.raises(RuntimeError, match="128"):
        _run(D.exct_decode, heats, regs, dev, K=129, num_dets=num_dets)


@pytest.mark.parametrize("name", ["exct_k72", "exct_k100", "exct_k128", "agnex_k100"])
def test_reference_goldens_beyond_k64(dev, name):
    """exct_k72: 209 positive rows, the cut among the penalised candidates; the others: 1000 positive rows."""
    agnex = name.startswith("agnex")
    heats, regs, K, num_dets = (BIGK.agnex_inputs if agnex else BIGK.exct_inputs)(name)
    got = _run(D.agnex_ct_decode if agnex else D.exct_decode, heats, regs, dev, K=K, num_dets=num_dets)
    assert_same(got, BIGK_GOLD[name + "/dets"])
    if name in ("exct_k72", "exct_k100"):
        assert _same_bits(got, SR.exct_decode(*heats, *regs, K=K, num_dets=num_dets))
    if name == "exct_k72":
        assert 0 < int((got[..., 4] > 0).sum()) < num_dets


# ------------------------------------------------------------------------------------------------
# 3. ties cut by num_dets
# ------------------------------------------------------------------------------------------------
def _tie_inputs(K):
    """(2, 2, 24, 24): every edge map holds exactly K isolated peaks of 0.5 per image (even rows and columns, so each
    is a 3x3 peak), the centre map is 0.25 everywhere: all rule-free groupings share one score."""
    B, C, H, W = 2, 2, 24, 24
    cells = [(c, y, x) for c in range(C) for y in range(0, H, 2) for x in range(0, W, 2)]
    edges = []
    for e in range(4):
        m = np.zeros((B, C, H, W), np.float32)
        for b in range(B):
            rng = np.random.RandomState(500 + 10 * b + e)
            for j in rng.choice(len(cells), K, replace=False):
                m[(b,) + cells[j]] = 0.5
        edges.append(m)
    return edges + [np.full((B, C, H, W), 0.25, np.float32)], [None] * 4


def test_ties_cut_by_num_dets_small_k(dev):
    heats, regs = _tie_inputs(8)
    kw = dict(K=8, num_dets=1000, scores_thresh=0.1, center_thresh=0.1)
    stream = _run(D.exct_decode, heats, regs, dev, stream=True, **kw)
    assert _same_bits(stream, _run(D.exct_decode, heats, regs, dev, stream=False, **kw))
    assert _same_bits(stream, cref.exct_decode(*heats, *regs, **kw))
    assert len(np.unique(stream[..., 4])) <= 7          # a base score minus 0..6 rules: index order decides the rest


def test_ties_cut_by_num_dets_k66(dev):
    heats, regs = _tie_inputs(66)
    kw = dict(K=66, scores_thresh=0.1, center_thresh=0.1)
    wide = SR.exct_decode(*heats, *regs, num_dets=1024, **kw)       # the top 1000 are its first 1000 rows
    for b in range(2):      # the case bites: the run of equal scores crosses row 1000, index order makes the cut
        assert wide[b, 999, 4] == wide[b, 1000, 4] == wide[b, 0, 4] > 0
    got = _run(D.exct_decode, heats, regs, dev, num_dets=1000, stream=True, **kw)
    assert _same_bits(got, wide[:, :1000])


# ------------------------------------------------------------------------------------------------
# 4. batch, determinism, graph capture
# ------------------------------------------------------------------------------------------------
def test_batch_determinism_and_graph(dev):
    names = ["exct_b0", "exct_b1", "exct_b2"]
    gen = _construction({n: (1, 3, 24, 32, 65, 1000, True) for n in names})
    singles = [gen.exct_inputs(n) for n in names]
    assert not np.array_equal(singles[0][0][0], singles[1][0][0])
    heats = [_t(np.concatenate([s[0][e] for s in singles]), dev) for e in range(5)]
    regs = [_t(np.concatenate([s[1][e] for s in singles]), dev) for e in range(4)]
    kw = dict(K=65, num_dets=1000, stream=True)
    batch = D.exct_decode(*heats, *regs, **kw).cpu().numpy()
    for i, (h, r, _, _) in enumerate(singles):
        assert _same_bits(batch[i:i + 1], _run(D.exct_decode, h, r, dev, **kw)), i
    assert D.exct_decode(*heats, *regs, **kw).cpu().numpy().tobytes() == batch.tobytes()
    # one call in a graph (the workspace is the cached one the eager calls above sized), replayed twice
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D.exct_decode(*heats, *regs, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = D.exct_decode(*heats, *regs, **kw)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == batch.tobytes()


# ------------------------------------------------------------------------------------------------
# 5. refusals through the C ABI
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnex", [False, True])
def test_refusals(dev, agnex):
    lib = native.lib()
    B, C, H, W = 1, 3, 16, 16
    query = lib.cn_agnex_ct_decode_stream_workspace_bytes if agnex else lib.cn_exct_decode_stream_workspace_bytes
    entry = lib.cn_agnex_ct_decode_stream_f32 if agnex else lib.cn_exct_decode_stream_f32
    edge = torch.rand((B, 1 if agnex else C, H, W), device=dev)
    ct = torch.rand((B, C, H, W), device=dev)
    need = query(B, C, H, W, 128)
    assert need >= query(B, C, H, W, 4) > 0
    ws = torch.zeros(need, device=dev, dtype=torch.uint8)
    dets = torch.full((B, 1024, 14), -7.0, device=dev)

    def call(K=4, num_dets=100, ws_bytes=need, first=edge):
        return entry(native.ptr(first), native.ptr(edge), native.ptr(edge), native.ptr(edge), native.ptr(ct), None,
                     None, None, None, B, C, H, W, K, 0.1, 0.1, num_dets, 0, native.ptr(dets), native.ptr(ws),
                     ws_bytes, native.stream_ptr())
    assert call(K=129) == CN_ERR_UNSUPPORTED
    assert call(num_dets=1025) == CN_ERR_UNSUPPORTED
    assert call(K=2, num_dets=17) == CN_ERR_SHAPE
    assert call(ws_bytes=query(B, C, H, W, 4) - 1) == CN_ERR_WORKSPACE
    assert call(first=None) == CN_ERR_NULL
    torch.cuda.synchronize()
    assert bool((dets == -7.0).all()) and not bool(ws.any())        # nothing ran
    assert call(K=2, num_dets=16) == 0                               # (and the same call, in range, runs)
    torch.cuda.synchronize()
    assert bool((dets[:, :16] != -7.0).all()) and bool((dets[:, 16:] == -7.0).all())


# ------------------------------------------------------------------------------------------------
# 6. the detector under --ex_stream
# ------------------------------------------------------------------------------------------------
def _favour_one_class(model, cls=17, by=3.0):
    """(tests/test_gpu_tasks.py) random heads never agree on a class: one class is favoured in the last layer
    of the five maps, as a trained net's dominant object would be"""
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.split(".")[0] in ("hm_t", "hm_l", "hm_b", "hm_r", "hm_c") and k.endswith("bias") and v.numel() == 80:
                v[cls] += by


def _build(extra):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init(["exdet", "--arch", "hourglass", "--flip_test", "--input_res", "256", "--scores_thresh", "0",
                           "--center_thresh", "0"] + extra)
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    if not opt.agnostic_ex:
        _favour_one_class(det.model)
    return det


def _frame(seed):
    return np.random.RandomState(seed).randint(0, 256, (256, 256, 3)).astype(np.uint8)


def _same_results(a, b):
    return sorted(a) == sorted(b) and all(_same_bits(a[j], b[j]) for j in a)


def test_detector_k40_with_and_without_the_flag(dev):
    plain, stream = _build(["--K", "40"]), _build(["--K", "40", "--ex_stream"])
    assert not plain.ex_stream and stream.ex_stream and plain.opt.K == stream.opt.K == 40
    image = _frame(12)
    x = plain.pre_process(image, 1.0)[0].to(dev)
    a, b = plain.run_batch(x.clone()).cpu().numpy(), stream.run_batch(x.clone()).cpu().numpy()
    assert a.shape == (2, 1000, 14) and _same_bits(a, b) and int((a[..., 4] > 0).sum()) > 0
    assert _same_results(plain.run(image)["results"], stream.run(image)["results"])
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with pytest.raises(ValueError):         # the flag moves the limit, it does not lift it
        detector_factory["exdet"](opts().init(["exdet", "--arch", "hourglass", "--ex_stream", "--K", "129"]))


def _agreement(got, ref):
    """(rows of run(), rows of the pipe, run() rows with a pipe row within 5e-3 in all five columns): the bar of
    tests/test_gpu_exdet_pipe.py -- the network's own values differ in the last bits between run()'s batch of
    two and the pipe's batch of four, so rows near a cut may differ; the decode itself is pinned bit for bit"""
    n_ref, n_got, same = sum(len(v) for v in ref.values()), sum(len(v) for v in got.values()), 0
    for j in ref:
        if len(ref[j]) and len(got[j]):
            d = np.abs(got[j][:, None, :].astype(np.float64) - ref[j][None, :, :]).max(axis=2)
            same += int((d.min(axis=0) < 5e-3).sum())
    return n_ref, n_got, same


@pytest.mark.parametrize("agnostic", [False, True], ids=["classes", "agnostic"])
def test_detector_k72(dev, agnostic):
    det = _build(["--K", "72", "--ex_stream"] + (["--agnostic_ex"] if agnostic else []))
    x = det.pre_process(_frame(14), 1.0)[0].to(dev)
    assert tuple(det.process(x.clone())[1].shape) == (2, 1000, 14)
    seen, decode = [], det.decode

    def spy(*maps, **kw):       # the five post-sigmoid maps and the four offset maps run_batch decodes
        seen.append([m.cpu().numpy() for m in maps])
        return decode(*maps, **kw)
    det.decode = spy
    rows = det.run_batch(x.clone()).cpu().numpy()
    det.decode = decode
    assert det.range_ok() and len(seen) == 1 and len(seen[0]) == 9
    maps = seen[0]
    assert maps[0].shape == (2, 1 if agnostic else 80, 64, 64) and maps[4].shape == (2, 80, 64, 64)
    want = SR.exct_decode(*maps, K=72, scores_thresh=0.0, center_thresh=0.0, agnostic=agnostic)
    assert _same_bits(rows, want) and int((rows[..., 4] > 0).sum()) > 0
    frames = [_frame(21), _frame(22)]
    got = det.run_frames(frames)
    assert len(got) == 2
    for b, f in enumerate(frames):
        ref = det.run(f)["results"]
        assert sorted(got[b]) == sorted(ref) == list(range(1, 81))
        n_ref, n_got, same = _agreement(got[b], ref)
        print("run_frames vs run, frame", b, dict(rows_run=n_ref, rows_pipe=n_got, same=same))
        assert n_ref > 0 and abs(n_got - n_ref) <= max(2, n_ref // 20) and same >= 0.9 * n_ref
