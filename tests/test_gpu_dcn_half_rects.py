"""cn_dcn_v2_forward_nhwc_f16_rects: an image that sits OFF the origin of a canvas gets, inside its rectangle, the
output of its own forward bit for bit -- in both forms of the half deformable convolution (the implicit GEMM's
gather and the LDS window) -- where the plain entry rounds its bilinear fractions by the absolute position and does
not; with a null table the entry is the plain one, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from centernet_amd import native

pytestmark = pytest.mark.gpu
CIN, COUT = 64, 64
IMAGE = (8, 16)              # rows, columns of the image: one 8 x 16 tile of the window form
CANVAS = (16, 48)
ORIGIN = (8, 16)             # y0, x0 of the image's rectangle on the canvas
FORMS = {"gather": (1, native.DCN_GATHER), "window": (2, native.DCNH_WINDOW)}      # cn_set_tuning key 23


@pytest.fixture(autouse=True)
def _default_tuning():
    yield
    native.lib().cn_reset_tuning()


def _operands(dev):
    g = torch.Generator().manual_seed(41)
    h, w = IMAGE
    x = torch.randn((1, h, w, CIN), generator=g).half()
    om = torch.zeros((1, h, w, 32))
    om[..., :18] = 7.0 * (torch.rand((1, h, w, 18), generator=g) - 0.5)       # +-3.5 px: beyond the window's reach too
    om[..., 18:27] = torch.randn((1, h, w, 9), generator=g)                    # mask logits
    wt = (torch.randn((COUT, CIN, 3, 3), generator=g) / 24.0).to(dev)
    lib = native.lib()
    wp = torch.empty(lib.cn_packed_conv_weight_elems(COUT, CIN, 3, 3, native.DTYPE_F16), device=dev, dtype=torch.float16)
    native.check(lib.cn_pack_conv_weight(native.ptr(wt), native.ptr(wp), COUT, CIN, 3, 3, native.DTYPE_F16,
                                         native.stream_ptr()), "cn_pack_conv_weight")
    bias = torch.randn(COUT, generator=g).to(dev)
    # the canvas: the image at ORIGIN with zeros around it (what the masks leave), a second image that fills its
    # slice; offsets outside the rectangle are whatever the offset convolution left there
    (hc, wc), (y0, x0) = CANVAS, ORIGIN
    xc = torch.zeros((2, hc, wc, CIN), dtype=torch.float16)
    xc[0, y0:y0 + h, x0:x0 + w] = x[0]
    xc[1] = torch.randn((hc, wc, CIN), generator=g).half()
    omc = 5.0 * torch.randn((2, hc, wc, 32), generator=g)
    omc[0, y0:y0 + h, x0:x0 + w] = om[0]
    rects = torch.tensor([[x0, y0, x0 + w, y0 + h], [0, 0, wc, hc]], dtype=torch.int32)
    return [t.to(dev) for t in (x, om, xc, omc, rects)] + [wp, bias]


def _run(entry, x, om, wp, bias, *more):
    lib = native.lib()
    B, H, W, _ = x.shape
    y = torch.full((B, H, W, COUT), float("nan"), device=x.device, dtype=torch.float16)
    native.check(entry(native.ptr(x), native.ptr(wp), native.ptr(bias), native.ptr(om), 32, None, None, native.ptr(y),
                       COUT, B, CIN, H, W, COUT, 1, 1, None, 0, *more, native.stream_ptr()), "half deformable entry")
    info = native.DcnRouteInfo()
    native.check(lib.cn_dcn_v2_route_f16(native.ptr(x), native.ptr(wp), native.ptr(bias), native.ptr(om), 32, None, None,
                                         native.ptr(y), COUT, B, CIN, H, W, COUT, 1, 1, None, 0, native.stream_ptr(),
                                         ctypes.byref(info)), "cn_dcn_v2_route_f16")
    torch.cuda.synchronize()
    return y.view(torch.int16).cpu().numpy(), info.form


@pytest.mark.parametrize("form", list(FORMS))
def test_an_image_off_the_canvas_origin_equals_its_own_forward(dev, form):
    lib = native.lib()
    key, want = FORMS[form]
    x, om, xc, omc, rects, wp, bias = _operands(dev)
    (h, w), (y0, x0) = IMAGE, ORIGIN
    with native.tuning({23: key}):
        alone, f0 = _run(lib.cn_dcn_v2_forward_nhwc_f16, x, om, wp, bias)
        plain, f1 = _run(lib.cn_dcn_v2_forward_nhwc_f16, xc, omc, wp, bias)
        placed, f2 = _run(lib.cn_dcn_v2_forward_nhwc_f16_rects, xc, omc, wp, bias, native.ptr(rects), 0)
        null, f3 = _run(lib.cn_dcn_v2_forward_nhwc_f16_rects, xc, omc, wp, bias, None, 0)
        # a table one level up (shift 1): the same origins from rectangles in the units of a tensor twice the size
        up, _ = _run(lib.cn_dcn_v2_forward_nhwc_f16_rects, xc, omc, wp, bias, native.ptr(rects * 2), 1)
    assert f0 == f1 == f2 == f3 == want, (f0, f1, f2, f3)
    assert np.array_equal(null, plain)
    assert np.array_equal(placed[0, y0:y0 + h, x0:x0 + w], alone[0])
    assert np.array_equal(up, placed)
    assert np.array_equal(placed[1], plain[1])                   # a rectangle at the origin: the plain arithmetic
    moved = int((plain[0, y0:y0 + h, x0:x0 + w] != alone[0]).sum())
    print("%s form: the plain entry differs from the image's own forward in %d of %d values" % (form, moved, alone.size))
    assert moved > 0
    assert (alone != np.int16(0x7E00)).all() and np.isfinite(alone.view(np.float16)).all()


def test_rects_entry_refuses_a_bad_shift(dev):
    lib = native.lib()
    x, om, xc, omc, rects, wp, bias = _operands(dev)
    y = torch.empty((2,) + CANVAS + (COUT,), device=dev, dtype=torch.float16)
    for shift in (-1, 31):
        assert lib.cn_dcn_v2_forward_nhwc_f16_rects(native.ptr(xc), native.ptr(wp), native.ptr(bias), native.ptr(omc), 32,
                                                    None, None, native.ptr(y), COUT, 2, CIN, 16, 48, COUT, 1, 1, None, 0,
                                                    native.ptr(rects), shift, native.stream_ptr()) == -1
