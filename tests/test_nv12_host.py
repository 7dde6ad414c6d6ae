"""NV12 frames on the host: cn_nv12_to_bgr_u8_host against an independent restatement of the integer BT.601
limited-range conversion (20-bit fixed point, no chroma interpolation), the argument errors of both NV12 entry
points, the image helpers and the argument checks of the frame entry points.  No GPU."""
import ctypes

import numpy as np
import pytest

from centernet_amd import native
from centernet_amd.image import bgr_to_nv12, check_pixel_format, nv12_to_bgr

CN_ERR_SHAPE, CN_ERR_NULL = -1, -5


def reference_bgr(buf, H, W, pitch):
    """The definition, in numpy int64: rows `pitch` bytes apart, H rows of Y, then H / 2 rows of (U, V) pairs."""
    rows = np.asarray(buf).reshape(-1)[:pitch * (H * 3 // 2)].reshape(H * 3 // 2, pitch)
    out = np.empty((H, W, 3), np.uint8)
    for lo in range(0, H, 512):                       # strips: the int64 temporaries of 4096 x 4096 stay small
        hi = min(lo + 512, H)
        Y = rows[lo:hi, :W].astype(np.int64)
        uv = rows[H + lo // 2:H + hi // 2, :W].astype(np.int64)
        U = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1) - 128
        V = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1) - 128
        yy = np.maximum(0, Y - 16) * 1220542
        out[lo:hi, :, 0] = np.clip((yy + 2116026 * U + (1 << 19)) >> 20, 0, 255)
        out[lo:hi, :, 1] = np.clip((yy - 409993 * U - 852492 * V + (1 << 19)) >> 20, 0, 255)
        out[lo:hi, :, 2] = np.clip((yy + 1673527 * V + (1 << 19)) >> 20, 0, 255)
    return out


def exhaustive_frame():
    """4096 x 4096: block k of the 2048 x 2048 2 x 2 blocks holds (U, V) = (k >> 14, (k >> 6) & 255) and the four
    luma values 4 (k & 63) + 0..3, so every (Y, U, V) triple occurs exactly once."""
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    frame = np.empty((6144, 4096), np.uint8)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        frame[dy:4096:2, dx::2] = (k & 63) * 4 + i
    frame[4096:, 0::2] = k >> 14
    frame[4096:, 1::2] = (k >> 6) & 255
    return frame


def host_convert(buf, H, W, pitch):
    buf = np.ascontiguousarray(buf)
    out = np.empty((H, W, 3), np.uint8)
    rc = native.lib().cn_nv12_to_bgr_u8_host(buf.ctypes.data_as(ctypes.c_void_p), H, W, pitch,
                                             out.ctypes.data_as(ctypes.c_void_p))
    assert rc == native.CN_OK
    return out


def test_host_entry_every_yuv_triple():
    frame = exhaustive_frame()
    triples = np.stack([frame[:4096].reshape(2048, 2, 2048, 2).transpose(0, 2, 1, 3).reshape(-1, 4),
                        np.repeat(frame[4096:, 0::2].reshape(-1, 1), 4, axis=1),
                        np.repeat(frame[4096:, 1::2].reshape(-1, 1), 4, axis=1)], -1).reshape(-1, 3).astype(np.int64)
    codes = triples[:, 0] << 16 | triples[:, 1] << 8 | triples[:, 2]
    assert (np.bincount(codes, minlength=1 << 24) == 1).all()     # the frame is what it claims to be
    got = host_convert(frame, 4096, 4096, 4096)
    assert np.array_equal(got, reference_bgr(frame, 4096, 4096, 4096))


@pytest.mark.parametrize("yuv,bgr", [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)),
                                     ((81, 90, 240), (0, 0, 254))])
def test_fixed_vectors(yuv, bgr):
    frame = np.empty((3, 2), np.uint8)
    frame[:2] = yuv[0]
    frame[2] = yuv[1:]
    for out in (host_convert(frame, 2, 2, 2), reference_bgr(frame, 2, 2, 2), nv12_to_bgr(frame)):
        assert out.shape == (2, 2, 3) and (out.reshape(-1, 3) == np.array(bgr)).all()


@pytest.mark.parametrize("H,W,pitch", [(2, 2, 5), (2, 18, 19), (6, 130, 160), (34, 62, 80)])
def test_host_entry_small_frames_with_pitch(H, W, pitch):
    rng = np.random.RandomState(H * 1000 + W)
    buf = rng.randint(0, 256, (H * 3 // 2, pitch)).astype(np.uint8)
    got = host_convert(buf, H, W, pitch)
    assert np.array_equal(got, reference_bgr(buf, H, W, pitch))
    dense = np.ascontiguousarray(buf[:, :W])
    assert np.array_equal(got, nv12_to_bgr(dense))            # the padding bytes are never read into the result


def test_argument_errors_of_both_entry_points():
    lib = native.lib()
    buf = np.zeros((64 * 3 // 2) * 64 * 2, np.uint8)
    out = np.zeros(2 * 64 * 64 * 3, np.uint8)
    src, dst = buf.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

    def host(H, W, pitch, s=src, d=dst):
        return lib.cn_nv12_to_bgr_u8_host(s, H, W, pitch, d)

    def batch(N, stride, H, W, pitch, s=src, d=dst):
        # every call below is refused by the argument check, in front of anything that needs a device
        return lib.cn_nv12_to_bgr_u8_batch(s, N, stride, H, W, pitch, d, None)

    assert host(64, 64, 64) == native.CN_OK
    assert host(64, 64, 64, s=None) == CN_ERR_NULL and host(64, 64, 64, d=None) == CN_ERR_NULL
    assert batch(1, 0, 64, 64, 64, s=None) == CN_ERR_NULL and batch(1, 0, 64, 64, 64, d=None) == CN_ERR_NULL
    for H, W, pitch in ((63, 64, 64), (64, 63, 64), (0, 64, 64), (64, 0, 64), (-2, 64, 64), (64, -2, 64),
                        (64, 64, 62), (32768, 64, 64), (64, 32768, 32768)):
        assert host(H, W, pitch) == CN_ERR_SHAPE, (H, W, pitch)
        assert batch(1, 0, H, W, pitch) == CN_ERR_SHAPE, (H, W, pitch)
    assert batch(2, 64 * 96 - 1, 64, 64, 64) == CN_ERR_SHAPE      # frames that overlap
    assert batch(2, 80 * 96 - 1, 64, 64, 80) == CN_ERR_SHAPE      # ... counted with the pitch
    assert batch(0, 64 * 96, 64, 64, 64) == CN_ERR_SHAPE
    assert batch(65536, 64 * 96, 64, 64, 64) == CN_ERR_SHAPE


def test_nv12_to_bgr_rejects_odd_sizes_and_wrong_dtype():
    assert nv12_to_bgr(np.zeros((9, 4), np.uint8)).shape == (6, 4, 3)
    for shape in ((8, 4), (9, 5), (3, 3), (9, 4, 1), (0, 4), (9,)):
        with pytest.raises(ValueError):
            nv12_to_bgr(np.zeros(shape, np.uint8))
    for dtype in (np.int8, np.uint16, np.float32):
        with pytest.raises(ValueError):
            nv12_to_bgr(np.zeros((9, 4), dtype))
    with pytest.raises(ValueError):
        nv12_to_bgr([[0, 0]] * 3)


def test_bgr_to_nv12_shape_grey_and_round_trip():
    rng = np.random.RandomState(5)
    with pytest.raises(ValueError):
        bgr_to_nv12(np.zeros((5, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        bgr_to_nv12(np.zeros((4, 4, 3), np.float32))
    grey = np.repeat(rng.randint(0, 256, (6, 10, 1)), 3, axis=2).astype(np.uint8)
    frame = bgr_to_nv12(grey)
    assert frame.shape == (9, 10) and frame.dtype == np.uint8 and (frame[6:] == 128).all()
    assert frame[:6].min() >= 16 and frame[:6].max() <= 235
    # two roundings of 8-bit limited-range luma: a grey level comes back within 2 steps
    assert np.abs(nv12_to_bgr(frame).astype(int) - grey).max() <= 2
    # a picture that is constant over every 2 x 2 block loses nothing to the chroma sub-sampling: the
    # round trip stays within the rounding of the two 8-bit matrices
    blocks = np.repeat(np.repeat(rng.randint(0, 256, (8, 12, 3)), 2, axis=0), 2, axis=1).astype(np.uint8)
    assert np.abs(nv12_to_bgr(bgr_to_nv12(blocks)).astype(int) - blocks).max() <= 4


def _detector_without_a_device():
    from centernet_amd.detectors.base_detector import BaseDetector
    return object.__new__(BaseDetector)       # the argument checks run in front of anything that needs __init__


def test_unknown_pixel_format_raises():
    det = _detector_without_a_device()
    frames = [np.zeros((6, 4), np.uint8)] * 2
    assert check_pixel_format("bgr") == "bgr" and check_pixel_format("nv12") == "nv12"
    for call in (lambda: check_pixel_format("yuv"),
                 lambda: det.pre_process_device(frames[0], 1.0, pixel_format="yuv"),
                 lambda: det.run_frames(frames, pixel_format="yuv"),
                 lambda: list(det.run_frames_stream([frames], pixel_format="yuv"))):
        with pytest.raises(ValueError, match="pixel_format"):
            call()


def test_ddd_unknown_pixel_format_raises():
    from centernet_amd.detectors.ddd import DddDetector
    det = object.__new__(DddDetector)
    frames = [np.zeros((6, 4), np.uint8)] * 2
    with pytest.raises(ValueError, match="pixel_format"):
        det.run_frames(frames, calibs=np.zeros((3, 4), np.float32), pixel_format="yuv")
    with pytest.raises(ValueError, match="pixel_format"):
        list(det.run_frames_stream([(frames, np.zeros((3, 4), np.float32))], pixel_format="yuv"))


def test_run_frames_rejects_frames_of_the_other_format():
    det = _detector_without_a_device()
    bgr = [np.zeros((6, 4, 3), np.uint8)] * 2
    nv12 = [np.zeros((9, 4), np.uint8)] * 2
    assert det._frames_geometry(bgr) == (2, 6, 4) and det._frames_geometry(nv12, "nv12") == (2, 6, 4)
    with pytest.raises(ValueError, match="NV12"):
        det.run_frames(bgr, pixel_format="nv12")
    with pytest.raises(ValueError, match="BGR"):
        det.run_frames(nv12)
    with pytest.raises(ValueError, match="BGR"):
        det.run_frames(nv12, pixel_format="bgr")
    with pytest.raises(ValueError):
        det.run_frames([np.zeros((9, 4), np.uint8), np.zeros((9, 6), np.uint8)], pixel_format="nv12")
    with pytest.raises(ValueError):
        det.run_frames([np.zeros((8, 4), np.uint8)], pixel_format="nv12")     # 8 rows are no H * 3 / 2
    with pytest.raises(ValueError):
        det.run_frames([np.zeros((9, 4), np.float32)], pixel_format="nv12")
