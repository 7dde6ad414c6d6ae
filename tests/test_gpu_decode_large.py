"""The large-K image-level top-K (cn_ctdet_decode_large_f32 / cn_topk_large_f32, 1 <= K <= 1024) through the C ABI
and through decode.ctdet_decode / _topk: bit for bit against the C oracle (which has no limit on K and the
library's tie order), against the reference's goldens at K = 300, 500 and 1000, and against the K <= 128 entries
where both take the call."""
import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from oracle import cref
from test_decode_large_host import GEN, GOLD, assert_matches_golden, bits

pytestmark = pytest.mark.gpu
OK, SHAPE, UNSUP, WS, LAUNCH, NULL, ALIGN = 0, -1, -2, -3, -4, -5, -6


def _gpu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def large_ctdet(dev, heat, wh, reg, K, cat=False, flags=0, ws=None):
    """cn_ctdet_decode_large_f32 through the raw binding (any K it takes, K <= 128 too) -> (dets, inds), numpy."""
    lib = native.lib()
    heat, wh, reg = (a if a is None or torch.is_tensor(a) else _gpu(a, dev) for a in (heat, wh, reg))
    B, C, H, W = heat.shape
    dets = torch.full((B, K, 6), float("nan"), device=dev)
    inds = torch.full((B, K), -7, device=dev, dtype=torch.int32)
    if ws is None:
        ws = torch.empty(lib.cn_ctdet_decode_large_workspace_bytes(B, C, H, W, K), device=dev, dtype=torch.uint8)
    rc = lib.cn_ctdet_decode_large_f32(native.ptr(heat), native.ptr(wh), native.ptr(reg), B, C, H, W, K, int(cat),
                                       flags, native.ptr(dets), native.ptr(inds), native.ptr(ws), ws.numel(),
                                       native.stream_ptr())
    assert rc == OK, rc
    return dets.cpu().numpy(), inds.cpu().numpy().astype(np.int64)


def large_topk(dev, heat, K, flags=0):
    lib = native.lib()
    heat = _gpu(heat, dev)
    B, C, H, W = heat.shape
    s = torch.full((B, K), float("nan"), device=dev)
    i = torch.full((B, K), -7, device=dev, dtype=torch.int32)
    c = torch.full((B, K), -7, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.cn_ctdet_decode_large_workspace_bytes(B, C, H, W, K), device=dev, dtype=torch.uint8)
    rc = lib.cn_topk_large_f32(native.ptr(heat), B, C, H, W, K, flags, native.ptr(s), native.ptr(i), native.ptr(c),
                               native.ptr(ws), ws.numel(), native.stream_ptr())
    assert rc == OK, rc
    return s.cpu().numpy(), i.cpu().numpy().astype(np.int64), c.cpu().numpy()


def _maps(shape, seed, cat=False):
    B, C, H, W = shape
    return synth.uniform((B, 2 * C if cat else 2, H, W), 0, 40, seed), synth.uniform((B, 2, H, W), 0, 1, seed + 1)


def assert_is_oracle(dev, heat, K, seed=5, reg=True, cat=False, python=True, plus_zero=False):
    """The raw entry, and (K > 128) decode.ctdet_decode, against the oracle: every bit of every row, the indices.
    ``plus_zero``: maps with negative values, where the oracle's heat * keep leaves -0.0 in a suppressed cell and
    the library, by its contract, +0.0 (as every form: tests/test_gpu_decode.py compares those scores by value) --
    the oracle's zeros lose their sign before the comparison, everything else stays bit for bit."""
    wh, rg = _maps(heat.shape, seed, cat)
    rg = rg if reg else None
    ref, ref_inds = cref.ctdet_decode(heat, wh, rg, cat_spec_wh=cat, K=K, return_inds=True)
    if plus_zero:
        ref[..., 4] = ref[..., 4] + np.float32(0.0)
    dets, inds = large_ctdet(dev, heat, wh, rg, K, cat=cat)
    assert np.array_equal(inds, ref_inds)
    assert np.array_equal(bits(dets), bits(ref)), np.abs(dets - ref).max()
    if python and K > 128:
        from centernet_amd.decode import ctdet_decode
        d, i = ctdet_decode(_gpu(heat, dev), _gpu(wh, dev), _gpu(rg, dev), cat_spec_wh=cat, K=K, return_inds=True)
        assert np.array_equal(i.cpu().numpy(), ref_inds) and np.array_equal(bits(d.cpu().numpy()), bits(ref))
    return ref


# ---------------------------------------------------------------- 1. the reference's goldens
@pytest.mark.parametrize("name", sorted(GEN.DECODE_LARGE_CASES))
def test_bit_exact_vs_reference_golden(dev, name):
    from centernet_amd.decode import ctdet_decode
    heat, wh, reg, K = GEN.decode_large_inputs(name)
    dets = ctdet_decode(_gpu(heat, dev), _gpu(wh, dev), _gpu(reg, dev), K=K).cpu().numpy()
    assert_matches_golden(dets, GOLD[name + "/dets"])


# ---------------------------------------------------------------- 2. boundary values of K, odd geometry
@pytest.mark.parametrize("shape", [(2, 3, 32, 32, 129), (2, 3, 32, 32, 300), (2, 3, 32, 32, 1000),
                                   (2, 3, 16, 16, 256),       # K == H*W: every cell of every plane is a candidate
                                   (2, 5, 23, 17, 391),       # K == H*W, W % 4 != 0
                                   (1, 2, 132, 128, 1000)])   # a plane past 128 rows: two bands per plane
def test_vs_oracle(dev, shape):
    B, C, H, W, K = shape
    assert_is_oracle(dev, synth.heatmap((B, C, H, W), 11 + B + C), K)


def test_k_equals_the_map_with_one_class(dev):
    """(1, 1, 32, 32), K = 1024 = H*W: about a ninth of the cells are positive peaks, the rest of the rows are the
    zeros of the suppressed cells in index order."""
    heat = synth.heatmap((1, 1, 32, 32), 3)
    ref = assert_is_oracle(dev, heat, 1024)
    pos = int((ref[..., 4] > 0).sum())
    assert 64 < pos < 256 and (ref[0, pos:, 4] == 0).all()


# ---------------------------------------------------------------- 3. ties
def test_constant_map_is_class_then_index_order(dev):
    heat = np.full((2, 3, 32, 32), 0.25, np.float32)
    ref = assert_is_oracle(dev, heat, 700)
    assert (ref[..., 4] == 0.25).all() and (ref[:, :, 5] == 0).all()      # 700 < 1024 cells: all from class 0


def test_few_bumps_then_zeros_of_several_planes(dev):
    """Ten bumps over three planes, K = 500: every plane hands on its bumps and zeros, the rows below the bumps are
    zeros in (class, index) order."""
    heat = np.zeros((2, 3, 32, 32), np.float32)
    rng = np.random.RandomState(4)
    for b in range(2):
        for j in range(10):
            heat[b, rng.randint(3), rng.randint(32), rng.randint(32)] = 0.5 + 0.04 * j + 0.01 * b
        heat[b, 1, 2, 3] = heat[b, 1, 2, 4] = 0.95       # equal neighbours: both survive the == test
    ref = assert_is_oracle(dev, heat, 500)
    pos = (ref[..., 4] > 0).sum(axis=1)
    assert (pos >= 8).all() and (pos <= 12).all() and len(set(ref[0, :12, 5].astype(int))) > 1


def test_negative_heat(dev):
    """Any floats: below the positive peaks come the zeros of the suppressed cells (negative peaks rank below them)."""
    ref = assert_is_oracle(dev, synth.normal((2, 4, 16, 15), 1.0, 2), 200, plus_zero=True)
    assert (ref[..., 4] > 0).any() and (ref[..., 4] == 0).any()


# ---------------------------------------------------------------- 4. full size
@pytest.fixture(scope="module")
def full_heat():
    return synth.heatmap((1, 80, 128, 128), 21)


def test_full_size_iid(dev, full_heat):
    ref = assert_is_oracle(dev, full_heat, 1024)
    assert len(set(ref[0, :, 5].astype(int))) > 40


def test_full_size_one_class_holds_the_candidates(dev, full_heat):
    """One class biased (the others scaled by 1/8, exactly): its plane alone holds nearly all of the K best."""
    heat = full_heat * np.float32(0.125)
    heat[0, 7] = full_heat[0, 7]
    ref = assert_is_oracle(dev, heat, 1024, python=False)
    assert float((ref[0, :, 5] == 7).mean()) > 0.9


# ---------------------------------------------------------------- 5. flags
def test_fused_sigmoid_matches_oracle(dev):
    """apply_sigmoid=True (logits in), compared as tests/test_gpu_decode.py::test_fused_sigmoid_matches_oracle
    compares, with its bars: scores within 1e-6 of torch's sigmoid, same boxes wherever the oracle's own score gap
    exceeds 1e-6."""
    from centernet_amd.decode import ctdet_decode
    from oracle.parity import compare_topk
    B, C, H, W, K = 2, 80, 128, 128, 300
    logits = synth.normal((B, C, H, W), 2.0, 3, mean=-2.19)
    wh, reg = _maps((B, C, H, W), 5)
    heat = torch.from_numpy(logits.copy()).sigmoid_().numpy()
    ref, ref_inds = cref.ctdet_decode(heat, wh, reg, K=K, return_inds=True)
    dets, inds = ctdet_decode(_gpu(logits, dev), _gpu(wh, dev), _gpu(reg, dev), K=K, apply_sigmoid=True,
                              return_inds=True)
    dets, inds = dets.cpu().numpy(), inds.cpu().numpy()
    assert np.abs(dets[..., 4] - ref[..., 4]).max() < 1e-6
    ids = np.stack([inds, dets[..., 5].astype(np.int64)], -1)
    rids = np.stack([ref_inds, ref[..., 5].astype(np.int64)], -1)
    r = compare_topk(dets, ref, tie=1e-6, got_ids=ids, ref_ids=rids)
    assert r["paired"] >= 0.999 and r["in_place"] >= 0.995 and r["safe"] >= 0.9, r
    # the logistic is the one of the K <= 128 forms: the first 128 scores are theirs, bit for bit
    old = ctdet_decode(_gpu(logits, dev), _gpu(wh, dev), _gpu(reg, dev), K=128, apply_sigmoid=True).cpu().numpy()
    assert np.array_equal(bits(old), bits(dets[:, :128]))


def test_cat_spec_wh_and_no_reg(dev):
    heat = synth.heatmap((2, 4, 24, 20), 8)
    assert_is_oracle(dev, heat, 250, cat=True)
    assert_is_oracle(dev, heat, 250, reg=False)
    assert_is_oracle(dev, heat, 250, cat=True, reg=False)


@pytest.mark.parametrize("shape", [(2, 5, 24, 40, 300), (3, 2, 17, 9, 153), (1, 80, 128, 128, 1024)])
def test_topk_with_and_without_the_peak_test(dev, shape):
    """cn_topk_large_f32: the plain _topk (CN_DECODE_NO_PEAK_TEST) on maps with negative values too, and _nms + _topk."""
    from centernet_amd.decode import _topk
    B, C, H, W, K = shape
    plain = synth.normal((B, C, H, W), 1.0, 9)
    for heat, flags, want in ((plain, native.DECODE_NO_PEAK_TEST, plain),
                              (synth.heatmap((B, C, H, W), 10), 0, None)):
        rs, ri, rc, ry, rx = cref.topk(cref.nms(heat) if want is None else want, K)
        s, i, c = large_topk(dev, heat, K, flags)
        assert np.array_equal(bits(s), bits(rs)) and np.array_equal(i, ri) and np.array_equal(c, rc)
        ps, pi, pc, py, px = _topk(_gpu(heat, dev), K=K, nms=want is None)
        assert np.array_equal(bits(ps.cpu().numpy()), bits(rs)) and np.array_equal(pi.cpu().numpy(), ri)
        assert np.array_equal(pc.cpu().numpy(), rc)
        assert np.array_equal(py.cpu().numpy(), ry) and np.array_equal(px.cpu().numpy(), rx)


# ---------------------------------------------------------------- 6. agreement with the K <= 128 entries
@pytest.mark.parametrize("shape", [(3, 7, 64, 64), (1, 80, 128, 128)])
def test_same_bits_as_the_small_k_entries(dev, shape, full_heat):
    from centernet_amd.decode import ctdet_decode
    heat = full_heat if shape == full_heat.shape else synth.heatmap(shape, 13)
    wh, reg = _maps(shape, 5)
    h, w, r = _gpu(heat, dev), _gpu(wh, dev), _gpu(reg, dev)
    for K in (1, 100, 128):
        old, old_inds = ctdet_decode(h, w, r, K=K, return_inds=True)
        new, new_inds = large_ctdet(dev, h, w, r, K)
        assert np.array_equal(new_inds, old_inds.cpu().numpy())
        assert np.array_equal(bits(new), bits(old.cpu().numpy()))


# ---------------------------------------------------------------- 7. workspace reuse, capture
def test_workspace_reuse(dev):
    """Two calls on one workspace with different inputs, three images that differ: each equals a call on a fresh
    workspace.  The form keeps no state words; whatever the first call left in the workspace means nothing."""
    B, C, H, W, K = 3, 6, 40, 36, 333
    lib = native.lib()
    ws = torch.empty(lib.cn_ctdet_decode_large_workspace_bytes(B, C, H, W, K), device=dev, dtype=torch.uint8)
    ws.fill_(0xFF)
    for seed in (1, 2):
        heat = synth.heatmap((B, C, H, W), seed)
        wh, reg = _maps((B, C, H, W), seed + 10)
        shared = large_ctdet(dev, heat, wh, reg, K, ws=ws)
        fresh = large_ctdet(dev, heat, wh, reg, K)
        assert np.array_equal(bits(shared[0]), bits(fresh[0])) and np.array_equal(shared[1], fresh[1])
        assert np.array_equal(bits(shared[0]), bits(cref.ctdet_decode(heat, wh, reg, K=K)))
        assert len({shared[0][b].tobytes() for b in range(B)}) == B


def test_captures_into_a_graph(dev):
    from centernet_amd.decode import ctdet_decode
    shape, K = (2, 6, 32, 32), 300
    heat = _gpu(synth.heatmap(shape, 31), dev)
    wh, reg = (_gpu(a, dev) for a in _maps(shape, 32))
    want = ctdet_decode(heat, wh, reg, K=K).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctdet_decode(heat, wh, reg, K=K)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ctdet_decode(heat, wh, reg, K=K)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------- 8. the Python route and the return codes
def test_python_route_limits(dev):
    from centernet_amd.decode import _topk, ctdet_decode
    heat = torch.rand((1, 2, 40, 40), device=dev)
    wh = torch.rand((1, 2, 40, 40), device=dev)
    for call in (lambda K: ctdet_decode(heat, wh, K=K), lambda K: _topk(heat, K=K)):
        with pytest.raises(RuntimeError, match="1024"):
            call(1025)
        with pytest.raises(RuntimeError, match="selected index k out of range"):
            call(1601)
    assert ctdet_decode(heat, wh, K=1024).shape == (1, 1024, 6)


def test_return_codes(dev):
    """Every refusal comes before anything is launched; only NULL or short arguments that the host rejects."""
    lib = native.lib()
    B, C, H, W, K = 1, 3, 32, 32, 300
    heat = torch.rand((B, C, H, W), device=dev)
    wh = torch.rand((B, 2, H, W), device=dev)
    dets = torch.empty((B, K, 6), device=dev)
    outs = [torch.empty((B, K), device=dev, dtype=t) for t in (torch.float32, torch.int32, torch.int32)]
    query = lib.cn_ctdet_decode_large_workspace_bytes
    need = query(B, C, H, W, K)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    st, p = native.stream_ptr(), native.ptr

    def ctdet(heat_=heat, wh_=wh, dets_=dets, ws_=ws, nbytes=need, k=K, b=B, h=H):
        return lib.cn_ctdet_decode_large_f32(p(heat_), p(wh_), None, b, C, h, W, k, 0, 0, p(dets_), None, p(ws_),
                                             nbytes, st)

    def topk(heat_=heat, s_=outs[0], ws_=ws, nbytes=need, k=K, b=B, h=H):
        return lib.cn_topk_large_f32(p(heat_), b, C, h, W, k, 0, p(s_), p(outs[1]), p(outs[2]), p(ws_), nbytes, st)
    mis = torch.rand(B * C * H * W + 1, device=dev)[1:].view(B, C, H, W)   # 4-byte aligned only
    for call in (ctdet, topk):
        assert call() == OK
        assert call(nbytes=need - 1) == WS
        assert call(heat_=None) == NULL and call(ws_=None) == NULL
        assert call(heat_=None, k=0) == NULL and call(heat_=None, k=1025) == NULL          # NULL first
        assert call(k=H * W + 1) == SHAPE and call(k=0) == SHAPE and call(b=0) == SHAPE
        assert call(k=1025, h=64) == UNSUP and call(k=1025, h=64, b=0) == SHAPE             # SHAPE, then UNSUPPORTED
        assert call(k=1025, h=64, heat_=mis) == UNSUP and call(heat_=mis) == ALIGN          # ... then ALIGN
        assert call(heat_=mis, nbytes=0) == ALIGN                                           # ... then WORKSPACE
    assert ctdet(wh_=None) == NULL and ctdet(dets_=None) == NULL and topk(s_=None) == NULL
    assert query(B, C, H, W, 1025) == 0 and query(B, C, H, W, 0) == 0 and query(B, C, 16, 16, 257) == 0
    assert query(B, C, H, W, K) == need and query(B, C, H, W, 1024) > 0
    # the flag of the callers that own their workspace means nothing to a form without state
    assert lib.cn_ctdet_decode_large_f32(p(heat), p(wh), None, B, C, H, W, K, 0, native.DECODE_STATE_CLEAN, p(dets),
                                         None, p(ws), need, st) == OK
    torch.cuda.synchronize()
