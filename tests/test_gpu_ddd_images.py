"""run_images / run_images_stream of the ddd task: cn_warp_table_u8_f32_ragged against cn_warp_table_u8_f32_batch
per image and against the oracle's ddd pre-process (bit for bit), and the image pipe against the host tail on its
own raw rows, run_frames (one size), the stream, run(image, calib), the synchronous path and swapped matrices.
References are the single-size code, never the mixed-size path."""
import ctypes

import numpy as np
import pytest
import torch

from centernet_amd import native
from centernet_amd.frame_pipe import ImageTables
from centernet_amd.post_process import ddd_norm_table, ddd_results_batch
from centernet_amd.image import get_affine_transform, invert_affine
from oracle import pre_oracle
from test_ddd_images_host import _host_detector
from test_ddd_tail_host import KITTI, _bits, calib_like
from test_gpu_ddd_pipe import (EXACT, _detector, _same_results, _threshold_inside, angle_bars, compare_rows)
from test_gpu_images import _descs, _pack, _to_dev
from test_gpu_tasks import _paired_fraction

pytestmark = pytest.mark.gpu

MIXED = [(96, 300), (93, 310), (94, 309), (100, 290)]


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# 1. the kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_kind", ["ddd_norm_table", "random"])
def test_ragged_table_warp_equals_the_batch_entry_per_image(dev, table_kind):
    lib = native.lib()
    N, oh, ow = 6, 24, 130                                   # 130 columns: two blocks of 128 threads, the second partial
    shapes = [(1, 1), (7, 5), (37, 124), (64, 200), (20, 33), (0, 9)]
    images = [_img(h, w, 300 + i) for i, (h, w) in enumerate(shapes)]
    pitches = [3, 15, 3 * 124, 3 * 200, 3 * 33 + 5, 27]      # the fifth one padded, the padding = 255
    buf, offsets = _pack(images, pitches, [1, 0, 1, 0, 2, 0], 255)
    assert any(o % 2 for o in offsets)                       # images at odd byte offsets
    if table_kind == "random":      # a kernel that recomputes the normalisation instead of reading the table fails
        table = np.random.RandomState(7).uniform(-3, 3, (3, 256)).astype(np.float32)
    else:
        table = ddd_norm_table([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    mats = []
    for i, (h, w) in enumerate(shapes):                      # the image onto the output; one with a rotation term
        s = np.array([max(w, 1), max(h, 1)], np.float32)
        c = np.array([w / 2., h / 2.], np.float32)
        m = get_affine_transform(c, s, 20 if i == 2 else 0, [ow, oh])
        mats.append(np.asarray(invert_affine(m), np.float64).reshape(-1))
    descs = _descs(images, pitches, offsets)
    for i in range(N):
        descs[i]['dst_to_src'] = mats[i]
    assert descs[5]['H'] == 0
    packed, dd, tab = torch.from_numpy(buf).cuda(), _to_dev(descs), torch.from_numpy(table).to(dev)
    got = torch.full((N, 3, oh, ow), float("nan"), device=dev)
    rc = lib.cn_warp_table_u8_f32_ragged(native.ptr(packed), native.ptr(dd), N, oh, ow, native.ptr(tab),
                                         native.ptr(got), native.stream_ptr())
    assert rc == native.CN_OK
    want = torch.full((N, 3, oh, ow), float("nan"), device=dev)
    for i, (h, w) in enumerate(shapes[:5]):
        rc = lib.cn_warp_table_u8_f32_batch(ctypes.c_void_p(packed.data_ptr() + offsets[i]), 1, 0, h, w, pitches[i],
                                            (ctypes.c_double * 6)(*mats[i]), oh, ow, native.ptr(tab),
                                            native.ptr(want[i:i + 1]), native.stream_ptr())
        assert rc == native.CN_OK
    torch.cuda.synchronize()
    assert np.array_equal(packed.cpu().numpy(), buf)         # the input is only read
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert not np.isnan(want[:5]).any()
    for i in range(5):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), i
        assert len(np.unique(got[i])) > 1 or shapes[i] == (1, 1)
    assert np.isnan(got[5]).all()                            # H = 0: skipped


@pytest.mark.parametrize("keep_res", [False, True])
def test_ragged_table_warp_equals_the_oracle_pre_process(dev, keep_res):
    det = _host_detector(("--keep_res",) if keep_res else ())           # input 96 x 320
    opt = det.opt
    assert (opt.input_h, opt.input_w) == (96, 320)
    shapes = [(93, 310), (92, 306), (93, 309), (94, 310)]               # the four KITTI sizes / 4
    images = [_img(h, w, 400 + i) for i, (h, w) in enumerate(shapes)]
    desc = np.zeros((1, 2, 4), native.IMAGE_DESC)
    nbytes, offsets, _, plan = ImageTables(det, det._pipe_scales()).fill(shapes, desc, np.zeros((1, 4, 6)))
    assert plan == [(False, 0, 0, 0)]
    buf = np.concatenate([im.reshape(-1) for im in images])
    assert len(buf) == nbytes
    packed, dd = torch.from_numpy(buf).cuda(), _to_dev(np.ascontiguousarray(desc[0, 1]))
    tab = torch.from_numpy(ddd_norm_table(det.mean, det.std)).to(dev)
    got = torch.full((4, 3, 96, 320), float("nan"), device=dev)
    rc = native.lib().cn_warp_table_u8_f32_ragged(native.ptr(packed), native.ptr(dd), 4, 96, 320, native.ptr(tab),
                                                  native.ptr(got), native.stream_ptr())
    torch.cuda.synchronize()
    assert rc == native.CN_OK
    got = got.cpu().numpy()
    for i, im in enumerate(images):
        want, _ = pre_oracle.ddd_pre_process(im, opt.mean, opt.std, 96, 320, keep_res=keep_res)
        assert np.array_equal(_bits(got[i]), _bits(want[0])), i


def test_ragged_table_warp_refuses_bad_arguments(dev):
    images = [_img(4, 5, 1)]
    buf, offsets = _pack(images, [15], [0], 0)
    d = _descs(images, [15], offsets)
    d[0]['dst_to_src'] = [1, 0, 0, 0, 1, 0]
    packed, dd = torch.from_numpy(buf).cuda(), _to_dev(d)
    tab, out = torch.zeros((3, 256), device=dev), torch.zeros((1, 3, 4, 5), device=dev)

    def call(p=packed, t=dd, N=1, oh=4, ow=5, tb=tab, o=out):
        return native.lib().cn_warp_table_u8_f32_ragged(native.ptr(p), native.ptr(t), N, oh, ow, native.ptr(tb),
                                                        native.ptr(o), native.stream_ptr())
    assert call() == native.CN_OK
    assert call(tb=None) == -5 and call(p=None) == -5 and call(t=None) == -5 and call(o=None) == -5
    assert call(N=0) == -1 and call(N=65536) == -1 and call(oh=65536) == -1 and call(oh=0) == -1 and call(ow=0) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. the image pipe
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ddd(dev):
    return _detector()[0]


@pytest.fixture(scope="module")
def ddd_keep_res(dev):
    return _detector(["--keep_res"])[0]


def _images(seed, shapes=MIXED):
    return [_img(h, w, seed + i) for i, (h, w) in enumerate(shapes)]


def _calibs(seed, n):
    rng = np.random.RandomState(seed)
    return [calib_like(rng) for _ in range(n)]


def _raw_rows(det, images, calibs):
    """the image pipe's own raw rows of a batch (the network is deterministic: the batch tensor run again)"""
    pipe = det._image_pipe_for(images, 1)
    assert pipe.tail is not None
    pipe.submit(0, images, det._calibs_for(images, calibs))
    pipe.collect(0, images)
    raw = det._run_scale(pipe.batch, False).detach().cpu().numpy()
    assert det.range_ok()
    return pipe, raw


def _check_against_host_tail(det, images, calibs):
    """(a): run_images == ddd_results_batch on the pipe's own raw rows with the per-image metas"""
    n = len(images)
    pipe, raw = _raw_rows(det, images, calibs)
    assert raw.shape == (n, 40, 18)
    det.opt.peak_thresh = _threshold_inside(raw[0, :, 2])
    got = det.run_images(images, calibs)
    side = det._calibs_for(images, calibs)
    metas = [dict(m, calib=p) for m, p in zip(pipe._metas(0, 0, n), side)]
    for m, im in zip(metas, images):
        c, s, _ = det._frame_geometry(im.shape[0], im.shape[1])
        assert np.array_equal(m['c'], c) and np.array_equal(m['s'], s)
    want = ddd_results_batch(raw, metas, det.opt.num_classes, det.opt.peak_thresh)
    bars, seen, kept = angle_bars(raw, metas), [0.0, 0.0], 0
    assert len(got) == len(want) == n
    for b in range(n):
        assert sorted(got[b]) == [1, 2, 3]
        for j in (1, 2, 3):
            compare_rows(got[b][j], want[b][j], bars, seen, (b, j))
            kept += len(want[b][j])
    assert 0 < kept < n * 40                                         # a real cut
    return pipe, raw, got, bars


def test_run_images_equals_the_host_tail_on_its_own_raw_rows(dev, ddd):
    images, calibs = _images(510), _calibs(511, 4)
    calibs[2] = None                                                 # the detector's default matrix
    pipe, _, got, _ = _check_against_host_tail(ddd, images, calibs)
    assert np.array_equal(pipe.side_host[0][2], ddd.calib)
    assert len({pipe.to_source_pinned[0][0, b].numpy().tobytes() for b in range(4)}) == 4    # four maps out
    pinned = pipe.tail.host('rows', 0).numpy()
    assert not any(np.shares_memory(r[j], pinned) for r in got for j in r)


def test_run_images_of_one_size_equals_run_frames(dev, ddd):
    frames, calibs = _images(520, [(96, 300)] * 3), _calibs(521, 3)
    _, raw = _raw_rows(ddd, frames, calibs)
    ddd.opt.peak_thresh = _threshold_inside(raw[:, :, 2])
    a, b = ddd.run_images(frames, calibs), ddd.run_frames(frames, calibs)
    assert len(a) == len(b) == 3
    for ra, rb in zip(a, b):
        _same_results(ra, rb)
    assert any(len(r[j]) for r in a for j in r)


def test_run_images_stream_equals_run_images_batch_by_batch(dev, ddd):
    small = [(60, 200), (64, 190), (58, 210)]
    batches = [(_images(530 + 10 * i, small if i == 0 else MIXED[i % 2:i % 2 + 3]), _calibs(540 + i, 3))
               for i in range(5)]
    first = sum(im.nbytes for im in batches[0][0])
    assert all(sum(im.nbytes for im in b[0]) > first for b in batches[1:])      # the buffers grow
    _, raw = _raw_rows(ddd, *batches[1])
    ddd.opt.peak_thresh = _threshold_inside(raw[:, :, 2])
    alone = [ddd.run_images(f, c) for f, c in batches]
    streamed = list(ddd.run_images_stream(iter(batches), depth=2))
    assert len(streamed) == len(batches)
    for ra, rs in zip(alone, streamed):
        assert len(ra) == len(rs) == 3
        for a, b in zip(ra, rs):
            _same_results(a, b)
    assert any(len(r[j]) for ra in alone for r in ra for j in r)
    pipe = ddd._image_pipe_for(batches[0][0], 2)
    assert min(pipe.capacity) > first
    pinned = [pipe.tail.host('rows', slot).numpy() for slot in range(2)]
    assert not any(np.shares_memory(r[j], p) for rs in streamed for r in rs for j in r for p in pinned)


def test_run_images_against_run_image_by_image(dev, ddd):
    """Batch-size-dependent summation order rules out bit equality: the paired-row bars of
    test_run_frames_against_run_frame_by_frame."""
    images, calibs = _images(550), _calibs(551, 4)
    calibs[1] = None
    _, raw = _raw_rows(ddd, images, calibs)
    ddd.opt.peak_thresh = _threshold_inside(raw[:, :, 2])
    batched = ddd.run_images(images, calibs)
    n_rows = 0
    for f, p, rb in zip(images, calibs, batched):
        one = ddd.run(f, p)["results"]
        top = lambda r: np.sort(np.concatenate([r[j][:, 12] for j in r if len(r[j])]))[::-1]
        sa, sb = top(rb), top(one)
        n = min(len(sa), len(sb))
        assert abs(len(sa) - len(sb)) <= 1 and n > 0
        assert np.abs(sa[:n] - sb[:n]).max() < 1e-4                  # scores
        for j in (1, 2, 3):
            assert abs(len(rb[j]) - len(one[j])) <= 1
            if len(one[j]) == 0:
                continue
            frac = _paired_fraction(rb[j], one[j], EXACT, 2e-2, 2e-3, window=8)
            ang = _paired_fraction(rb[j], one[j], [0, 11, 12], 2e-3, 1e-3, window=8)
            print("image %s class %d: paired %.3f, angles %.3f" % (f.shape[:2], j, frac, ang))
            assert frac >= 0.95 and ang >= 0.9, (j, frac, ang)
            n_rows += len(one[j])
    assert n_rows > 10


def test_keep_res_with_mixed_sizes(dev, ddd_keep_res):
    assert ddd_keep_res.opt.keep_res and not ddd_keep_res.opt.fix_res
    images, calibs = _images(560), _calibs(561, 4)
    pipe, _, _, _ = _check_against_host_tail(ddd_keep_res, images, calibs)
    assert all(list(m['s']) == [384, 128] for m in pipe._metas(0, 0, 4))


def test_run_images_sync_equals_the_pipe(dev, ddd):
    """the re-calibration route: the same batch bits, the same raw rows, the host tail against the device tail"""
    images, calibs = _images(570), _calibs(571, 4)
    calibs[0] = None
    pipe, raw, got, bars = _check_against_host_tail(ddd, images, calibs)
    side = ddd._calibs_for(images, calibs)
    batch = pipe.batch.clone()
    sync = ddd._run_images_sync(images, pipe.scales, side=side)
    assert len(sync) == 4
    seen = [0.0, 0.0]
    for b in range(4):
        for j in (1, 2, 3):
            compare_rows(got[b][j], sync[b][j], bars, seen, (b, j))
    # and its batch: pre_process_device image by image == the one launch
    again = torch.empty_like(batch)
    for i, im in enumerate(images):
        ddd.pre_process_device(im, 1.0, out=again[i:i + 1])
    assert torch.equal(again.view(torch.int32), batch.view(torch.int32))


def test_matrix_b_goes_with_image_b(dev, ddd_keep_res):
    """Two images of equal pixels inside zero borders of different sizes, under --keep_res: centred at scale 1,
    they give the same network input, hence the same raw rows, and only the maps out and the matrices differ.
    The score, the dimensions and alpha are equal.  The border moves the map out by t = (8, 4) pixels; the
    reference sends the (w, h) pair through the point map too, translation included, so the centre AND the pair
    move by t and the box centre -+ pair / 2 moves by (t / 2, 3 t / 2) = (4, 2, 12, 6).  With u the float32
    spacing at twice the largest box coordinate (it bounds the centre, the pair and the box), each image rounds the
    centre (u / 2), the pair (u / 2, halved) and the box (u / 2): 1.25 u, the difference of two 2.5 u.
    With the matrices swapped the lifted columns 8-10 are those of the other matrix, taken from the runs
    where ONE matrix serves both images."""
    det = ddd_keep_res
    inner = _img(96, 300, 580)
    outer = np.zeros((104, 316, 3), np.uint8)
    outer[4:100, 8:308] = inner
    images = [inner, outer]
    P1, P2 = KITTI, calib_like(np.random.RandomState(581))
    pipe, raw = _raw_rows(det, images, [P1, P2])
    assert torch.equal(pipe.batch[0].view(torch.int32), pipe.batch[1].view(torch.int32))
    assert np.array_equal(_bits(raw[0]), _bits(raw[1]))
    det.opt.peak_thresh = _threshold_inside(raw[0, :, 2])
    a1, b2 = det.run_images(images, [P1, P2])
    a2, b1 = det.run_images(images, [P2, P1])
    with_1, with_2 = det.run_images(images, P1), det.run_images(images, P2)
    _same_results(a1, with_1[0])
    _same_results(b2, with_2[1])
    _same_results(a2, with_2[0])
    _same_results(b1, with_1[1])
    n = 0
    for j in (1, 2, 3):
        assert a1[j].shape == b2[j].shape
        if not len(a1[j]):
            continue
        for x, y in ((a1[j], b2[j]), (a1[j], b1[j]), (a1[j], a2[j])):
            assert np.array_equal(_bits(x[:, [0, 5, 6, 7, 12]]), _bits(y[:, [0, 5, 6, 7, 12]]))
        assert np.array_equal(_bits(a1[j][:, 1:5]), _bits(a2[j][:, 1:5]))          # the box does not see the matrix
        bar = 2.5 * float(np.spacing(np.float32(2 * np.abs(b1[j][:, 1:5]).max())))
        shift = b1[j][:, 1:5].astype(np.float64) - a1[j][:, 1:5] - np.array([4., 2., 12., 6.])
        assert np.abs(shift).max() <= bar, (j, np.abs(shift).max(), bar)
        assert not np.array_equal(a1[j][:, 8:11], a2[j][:, 8:11])                  # another camera: other locations
        assert not np.array_equal(b1[j][:, 8:11], b2[j][:, 8:11])
        n += len(a1[j])
    assert n > 0
