"""NV12 frames on the device: cn_nv12_to_bgr_u8_batch against the host entry point bit for bit, and everything
above it -- pre_process_device, run_frames / run_frames_stream of ctdet, ddd and multi_pose, the hand-back route
of the frame pipe -- against the same call on image.nv12_to_bgr(frame): the conversion is exact, so every result
for an NV12 frame equals the BGR result bit for bit."""
import contextlib
import ctypes
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from centernet_amd.image import nv12_to_bgr

pytestmark = pytest.mark.gpu

GUARD = 256       # bytes behind the output that the kernel must leave alone


def _host(buf, N, stride, H, W, pitch):
    out = np.empty((N, H, W, 3), np.uint8)
    for n in range(N):
        frame = np.ascontiguousarray(buf[n * stride:n * stride + pitch * (H * 3 // 2)])
        rc = native.lib().cn_nv12_to_bgr_u8_host(frame.ctypes.data_as(ctypes.c_void_p), H, W, pitch,
                                                 out[n].ctypes.data_as(ctypes.c_void_p))
        assert rc == native.CN_OK
    return out


def _device(buf, N, stride, H, W, pitch, offset=0):
    """The batch entry on `buf` (flat uint8) uploaded `offset` bytes into an allocation; the output is followed by
    guard bytes that must come back untouched."""
    src = torch.zeros(offset + buf.size, dtype=torch.uint8, device="cuda")
    src[offset:] = torch.from_numpy(buf).cuda()
    out = torch.full((N * H * W * 3 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = native.lib().cn_nv12_to_bgr_u8_batch(ctypes.c_void_p(src.data_ptr() + offset), N, stride, H, W, pitch,
                                              native.ptr(out), native.stream_ptr())
    assert rc == native.CN_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[N * H * W * 3:] == 0xA5).all()
    return got[:N * H * W * 3].reshape(N, H, W, 3)


def _exhaustive_frame():
    """4096 x 4096, every (Y, U, V) triple once: block k of the 2048 x 2048 2 x 2 blocks holds
    (U, V) = (k >> 14, (k >> 6) & 255) and the luma values 4 (k & 63) + 0..3."""
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    frame = np.empty((6144, 4096), np.uint8)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        frame[dy:4096:2, dx::2] = (k & 63) * 4 + i
    frame[4096:, 0::2] = k >> 14
    frame[4096:, 1::2] = (k >> 6) & 255
    return frame


def test_kernel_every_yuv_triple(dev):
    buf = _exhaustive_frame().reshape(-1)
    assert np.array_equal(_device(buf, 1, 0, 4096, 4096, 4096), _host(buf, 1, 0, 4096, 4096, 4096))


# (N, H, W, pitch, bytes between frames beyond the frame, pointer offset): the byte form with its partial last
# group of a row (W % 16 != 0), frames with padding, and the 16-byte form with pitch and stride of its own
KERNEL_CASES = [
    (3, 34, 62, 80, 48, 0),
    (1, 2, 2, 2, 0, 0),
    (1, 2, 18, 18, 0, 0),
    (1, 6, 130, 130, 0, 0),
    (1, 514, 1026, 1026, 0, 0),
    (3, 34, 64, 80, 48, 0),          # 16-byte loads and stores, pitch > W, stride > frame
    (2, 6, 32, 32, 0, 0),            # 16-byte form, dense
    (2, 6, 32, 32, 0, 2),            # the same frames 2 bytes off: byte form
    (2, 6, 32, 40, 4, 0),            # pitch / stride no multiples of 16: byte form
]


@pytest.mark.parametrize("case", range(len(KERNEL_CASES)))
def test_kernel_equals_host_entry(dev, case):
    N, H, W, pitch, gap, offset = KERNEL_CASES[case]
    stride = pitch * (H * 3 // 2) + gap
    rng = np.random.RandomState(700 + case)
    buf = rng.randint(0, 256, (N - 1) * stride + pitch * (H * 3 // 2)).astype(np.uint8)
    assert np.array_equal(_device(buf, N, stride, H, W, pitch, offset), _host(buf, N, stride, H, W, pitch))


# ------------------------------------------------------------------------------------------------
# the detectors
# ------------------------------------------------------------------------------------------------
def _detector(task, args):
    from centernet_amd.detectors.detector_factory import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task] + list(args))
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det, opt


def _nv12_frames(seed, n, h=100, w=140):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8) for _ in range(n)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Two per-image results, bit for bit."""
    assert sorted(a) == sorted(b)
    for j in a:
        x, y = np.asarray(a[j], np.float32), np.asarray(b[j], np.float32)
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), j


def _same_batches(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        _same(a, b)


CTDET = ["--arch", "resdcn_18", "--input_h", "128", "--input_w", "128"]


@pytest.fixture(scope="module")
def ctdet(dev):
    det, opt = _detector("ctdet", CTDET)
    warm = [nv12_to_bgr(f) for f in _nv12_frames(1, 3)]
    det.run_frames(warm)                        # plans and calibration settle before anything is compared
    assert det.range_ok()
    return det


@pytest.mark.parametrize("flip", [False, True])
def test_pre_process_device_nv12_equals_bgr(dev, ctdet, flip):
    det = ctdet
    frame = _nv12_frames(2, 1)[0]
    bgr = nv12_to_bgr(frame)
    before = det.opt.flip_test
    det.opt.flip_test = flip
    try:
        for scale in (1, 0.5, 0.75):
            want, meta = det.pre_process_device(bgr, scale)
            assert want.shape[0] == (2 if flip else 1)
            for src in (frame, torch.from_numpy(frame).cuda()):
                got, m = det.pre_process_device(src, scale, pixel_format='nv12')
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), scale
                assert sorted(m) == sorted(meta) and all(np.array_equal(m[k], meta[k]) for k in m)
    finally:
        det.opt.flip_test = before
    with pytest.raises(ValueError):
        det.pre_process_device(frame, 1, pixel_format='yuv')
    with pytest.raises(ValueError):
        det.pre_process_device(bgr, 1, pixel_format='nv12')
    with pytest.raises(ValueError):
        det.pre_process_device(torch.from_numpy(frame), 1, pixel_format='nv12')      # a CPU tensor


def test_ctdet_run_frames_nv12_equals_bgr(dev, ctdet):
    det = ctdet
    nv12 = _nv12_frames(3, 3)
    want = det.run_frames([nv12_to_bgr(f) for f in nv12])
    assert sum(len(r[j]) for r in want for j in r) > 0
    _same_batches(det.run_frames(nv12, pixel_format='nv12'), want)
    _same_batches(det.run_frames(torch.from_numpy(np.stack(nv12)).cuda(), pixel_format='nv12'), want)
    pipe = det._pipe_for(nv12, 1, 'nv12')
    assert pipe.pixel_format == 'nv12' and tuple(pipe.dev_in[0].shape) == (3, 150, 140)
    assert tuple(pipe.pinned_in[0].shape) == (3, 150, 140) and tuple(pipe.bgr.shape) == (3, 100, 140, 3)
    assert pipe is not det._pipe_for([nv12_to_bgr(f) for f in nv12], 1)
    assert det.range_ok()


def test_ctdet_run_frames_nv12_flip_multi_scale_equals_bgr(dev):
    det, opt = _detector("ctdet", CTDET + ["--flip_test", "--test_scales", "0.75,1"])
    nv12 = _nv12_frames(4, 3)
    bgr = [nv12_to_bgr(f) for f in nv12]
    det.run_frames(bgr)
    want = det.run_frames(bgr)
    pipe = det._pipe_for(nv12, 1, 'nv12')
    assert pipe.flip and len(pipe.levels) == 2 and pipe.levels[0].resize
    _same_batches(det.run_frames(nv12, pixel_format='nv12'), want)
    assert det.range_ok()


def test_ctdet_run_frames_stream_nv12(dev, ctdet):
    det = ctdet
    batches = [_nv12_frames(10 + i, 3) for i in range(5)]
    want = [det.run_frames([nv12_to_bgr(f) for f in b]) for b in batches]
    streamed = list(det.run_frames_stream(iter(batches), depth=3, pixel_format='nv12'))
    assert len(streamed) == 5
    for got, ref in zip(streamed, want):
        _same_batches(got, ref)
    assert any(not np.array_equal(a[j], b[j]) for a, b in zip(want[0], want[1]) for j in a)   # the order is tested
    resident = [torch.from_numpy(np.stack(b)).cuda() for b in batches]
    streamed = list(det.run_frames_stream(iter(resident), depth=3, pixel_format='nv12'))
    assert len(streamed) == 5
    for got, ref in zip(streamed, want):
        _same_batches(got, ref)
    mixed = [batches[0], resident[1], batches[2], batches[3], resident[4]]       # host and device batches, one format
    for got, ref in zip(det.run_frames_stream(iter(mixed), depth=3, pixel_format='nv12'), want):
        _same_batches(got, ref)
    assert det.range_ok()


def test_mixing_formats_in_a_stream_raises(dev, ctdet):
    det = ctdet
    nv12 = _nv12_frames(20, 3)
    bgr = [nv12_to_bgr(f) for f in nv12]
    for batches, fmt in (([nv12, bgr], 'nv12'), ([bgr, nv12], 'bgr'),
                         ([bgr, torch.from_numpy(np.stack(nv12)).cuda()], 'bgr')):
        stream = det.run_frames_stream(iter(batches), depth=3, pixel_format=fmt)
        with pytest.raises(ValueError):
            list(stream)
        torch.cuda.synchronize()
    with pytest.raises(ValueError):
        det.run_frames(bgr, pixel_format='nv12')
    with pytest.raises(ValueError):
        det.run_frames(nv12)
    with pytest.raises(ValueError):
        det.run_frames(torch.from_numpy(np.stack(nv12)).cuda())          # a device batch is NV12 only
    with pytest.raises(ValueError):
        det.run_frames(torch.from_numpy(np.stack(nv12)), pixel_format='nv12')   # a CPU tensor
    _same_batches(det.run_frames(nv12, pixel_format='nv12'), det.run_frames(bgr))     # the pipes still serve
    assert det.range_ok()


def test_hand_back_route_nv12(dev, ctdet):
    """Both hand-back routes of collect end in pipe._run_sync(frames): on NV12 frames it is the synchronous path
    on the converted frames, bit for bit -- from host frames and from a device batch -- and it agrees with the
    pipe's result as closely as the synchronous BGR path does (another batch shape of the network: the bar of
    test_gpu_frames_tta.test_ctdet_run_frames_flip_equals_run, 2e-3 on rows that pair up by position)."""
    det = ctdet
    nv12 = _nv12_frames(30, 3)
    bgr = [nv12_to_bgr(f) for f in nv12]
    pipe = det._pipe_for(nv12, 1, 'nv12')
    piped = det.run_frames(nv12, pixel_format='nv12')
    want = det._run_frames_sync(bgr, pipe.scales)
    _same_batches(pipe._run_sync(nv12), want)
    _same_batches(pipe._run_sync(torch.from_numpy(np.stack(nv12)).cuda()), want)
    bgr_pipe = det._pipe_for(bgr, 1)
    _same_batches(bgr_pipe._run_sync(bgr), want)
    for a, b in zip(piped, want):
        for j in a:
            assert a[j].shape == b[j].shape, j
            if len(a[j]):
                assert np.abs(a[j] - b[j]).max() < 2e-3, j
    assert det.range_ok()


def test_ddd_run_frames_nv12_equals_bgr(dev):
    det, opt = _detector("ddd", ["--arch", "dla_34", "--input_h", "128", "--input_w", "384", "--K", "40"])
    nv12 = _nv12_frames(40, 2, 96, 300)
    bgr = [nv12_to_bgr(f) for f in nv12]
    rng = np.random.RandomState(41)
    calibs = [np.array([[700 + 20 * rng.rand(), 0, 150 + rng.rand(), 40 * rng.rand()],
                        [0, 700 + 20 * rng.rand(), 48 + rng.rand(), rng.rand()],
                        [0, 0, 1, 0.005 * rng.rand()]], np.float32) for _ in range(2)]
    det.run_frames(bgr, calibs)
    opt.peak_thresh = 0.0                      # every row of the tail, not an empty cut
    want = det.run_frames(bgr, calibs)
    assert sum(len(r[j]) for r in want for j in r) > 0
    pipe = det._pipe_for(nv12, 1, 'nv12')
    assert pipe.tail is not None and pipe.side_dev is not None
    _same_batches(det.run_frames(nv12, calibs, pixel_format='nv12'), want)
    _same_batches(det.run_frames(torch.from_numpy(np.stack(nv12)).cuda(), calibs, pixel_format='nv12'), want)
    _same_batches(next(iter(det.run_frames_stream([(nv12, calibs)], pixel_format='nv12'))), want)
    got, _ = det.pre_process_device(nv12[0], 1.0, pixel_format='nv12')
    ref, _ = det.pre_process_device(bgr[0], 1.0)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    side = det._calibs_for(nv12, calibs)
    _same_batches(pipe._run_sync(nv12, side=side), det._run_frames_sync(bgr, pipe.scales, side=side))
    _same_batches(pipe._run_sync(torch.from_numpy(np.stack(nv12)).cuda(), side=side),
                  det._run_frames_sync(bgr, pipe.scales, side=side))
    assert det.range_ok()


def test_multi_pose_run_frames_nv12_equals_bgr(dev):
    det, opt = _detector("multi_pose", ["--arch", "dla_34", "--input_h", "128", "--input_w", "128"])
    nv12 = _nv12_frames(50, 2, 96, 120)
    bgr = [nv12_to_bgr(f) for f in nv12]
    det.run_frames(bgr)
    want = det.run_frames(bgr)
    assert all(len(r[1]) for r in want)
    _same_batches(det.run_frames(nv12, pixel_format='nv12'), want)
    got = det.run_frames(nv12, arrays=True, pixel_format='nv12')
    assert all(isinstance(r[1], np.ndarray) for r in got)
    _same_batches(got, want)
    assert det.range_ok()
