"""The element-wise and layout kernels of csrc/cn_misc.hip, each against torch on the CPU: the depthwise
transposed convolution of IDAUp, nearest x2 up-sampling + add (fp32 and fp16), the channel-slice copy
behind concat, the NCHW <-> NHWC transposes, the plain-fp32 and the f32s max-pool on NEGATIVE data
(padding must be -inf, not 0) and the abs-max reduction of the calibration pass.  Every output is
pre-filled with NaN, so an element a kernel did not write shows; where the expected result is exact
the comparison is on the bits."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centernet_amd import synth

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(autouse=True)
def _default_tuning():
    """Every test of this module leaves the cn_set_tuning keys at the library's defaults."""
    yield
    from centernet_amd import native
    native.lib().cn_reset_tuning()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return torch.equal(_bits(got), _bits(want))


def _act(x_nchw, dev, dtype=torch.float32):
    from centernet_amd.engine import Act
    B, C, H, W = x_nchw.shape
    return Act(x_nchw.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=dtype), B, H, W, C)


def _run_filled(pb, *outs):
    for o in outs:
        o.t.fill_(NAN)
    for op in pb.ops:
        op()
    torch.cuda.synchronize()


def _plain_builder(dev, B, H, W, dtype=torch.float32):
    from centernet_amd.engine import PlanBuilder
    if dtype == torch.float16:
        return PlanBuilder(dev, B, H, W, dtype=torch.float16)
    return PlanBuilder(dev, B, H, W, dtype=torch.float32, split=False)


def _nchw(act):
    return act.t.permute(0, 3, 1, 2).cpu()


# ---- dw_deconv ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("shape", [(2, 64, 5, 7), (1, 4, 1, 1), (1, 36, 3, 16)])
@pytest.mark.parametrize("f", [2, 4, 8])
def test_dw_deconv_vs_float64(dev, f, shape, use_add):
    """cn_dw_conv_transpose_f32 against float64 conv_transpose2d(stride f, padding f // 2, groups C) (+ add),
    with normal (asymmetric) weights.  An output is at most 4 products and 4 additions:
    (1 + 2^-24)^5 - 1 < 2^-21 of S = conv_transpose(|x|, |w|) + |add|."""
    B, C, H, W = shape
    x = torch.from_numpy(synth.normal((B, C, H, W), 1.0, 61))
    w = torch.from_numpy(synth.normal((C, 1, 2 * f, 2 * f), 0.5, 62))
    add = torch.from_numpy(synth.normal((B, C, H * f, W * f), 1.0, 63)) if use_add else None
    ref = F.conv_transpose2d(x.double(), w.double(), None, f, f // 2, groups=C)
    S = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, f, f // 2, groups=C)
    if use_add:
        ref, S = ref + add.double(), S + add.double().abs()
    pb = _plain_builder(dev, B, H, W)
    y = pb.dw_deconv(_act(x, dev), w, f, add=_act(add, dev) if use_add else None)
    _run_filled(pb, y)
    got = _nchw(y)
    assert got.shape == ref.shape and not torch.isnan(got).any()
    over = (got.double() - ref).abs() > 2.0 ** -21 * S
    assert not bool(over.any()), (int(over.sum()), float(((got.double() - ref).abs() / S.clamp_min(1e-300)).max()))


# ---- upsample2x_add -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,C", [(torch.float32, 4), (torch.float32, 12), (torch.float32, 256),
                                     (torch.float16, 8), (torch.float16, 24), (torch.float16, 256)],
                         ids=["f32-4", "f32-12", "f32-256", "f16-8", "f16-24", "f16-256"])
def test_upsample2x_add_bit_exact(dev, dtype, C):
    """cn_upsample2x_add_f32 / _f16 against F.interpolate(nearest, x2) + add.  fp16: the sum of two halves is
    exact in fp32, so (x.float() + add.float()).half() -- one rounding -- is the whole kernel."""
    for (H, W) in [(1, 1), (3, 5), (7, 2)]:
        for B in (1, 2):
            for use_add in (False, True):
                x = torch.from_numpy(synth.normal((B, C, H, W), 1.0, 71 + B)).to(dtype)
                add = torch.from_numpy(synth.normal((B, C, 2 * H, 2 * W), 1.0, 73 + B)).to(dtype) if use_add else None
                up = F.interpolate(x.float(), scale_factor=2, mode="nearest")
                want = ((up + add.float()) if use_add else up).to(dtype)
                pb = _plain_builder(dev, B, H, W, dtype)
                y = pb.upsample2x_add(_act(x, dev, dtype), _act(add, dev, dtype) if use_add else None)
                assert y.t.dtype == dtype
                _run_filled(pb, y)
                assert _same_bits(_nchw(y), want), (H, W, B, use_add)


# ---- cn_copy_channels_f32 / concat ----------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 36, 64])
def test_copy_channels_between_slices(dev, C):
    """Source: channels [4, 4 + C) of a wider tensor; destination: channels [32, 32 + C) of a 104-wide one.
    The destination slice equals the source bit for bit, everything else in it is still NaN.  (The source
    pitch is 44 where the slice fits -- C = 4, 36 -- and 76 for C = 64.)"""
    from centernet_amd import native
    lib = native.lib()
    npix, s_off, d_off, d_pitch = 3 * 7 * 5, 4, 32, 104
    s_pitch = 44 if s_off + C <= 44 else s_off + C + 8
    src = torch.from_numpy(synth.normal((npix, s_pitch), 1.0, 81)).to(dev)
    dst = torch.full((npix, d_pitch), NAN, device=dev)
    native.check(lib.cn_copy_channels_f32(ctypes.c_void_p(src.data_ptr() + 4 * s_off), s_pitch,
                                          ctypes.c_void_p(dst.data_ptr() + 4 * d_off), d_pitch, npix, C,
                                          native.stream_ptr()), "cn_copy_channels_f32")
    torch.cuda.synchronize()
    got = dst.cpu()
    assert _same_bits(got[:, d_off:d_off + C], src.cpu()[:, s_off:s_off + C])
    assert bool(torch.isnan(got[:, :d_off]).all()) and bool(torch.isnan(got[:, d_off + C:]).all())


def test_concat_of_plain_tensors(dev):
    B, H, W = 2, 5, 7
    parts = [torch.from_numpy(synth.normal((B, c, H, W), 1.0, 85 + i)) for i, c in enumerate((36, 4, 24))]
    pb = _plain_builder(dev, B, H, W)
    cat = pb.concat([_act(p, dev) for p in parts])
    assert cat.fmt == "f32" and cat.pitch == 64
    _run_filled(pb, cat)
    assert _same_bits(_nchw(cat), torch.cat(parts, 1))


# ---- NCHW <-> NHWC --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 27, 33, 80])
def test_layout_transposes(dev, C):
    """cn_nchw_to_nhwc_f32: channels < C are the permute, channels C .. pitch exactly 0; cn_nhwc_to_nchw_f32
    ignores the pad channels (NaN here); the round trip is bit-identical.  Maps of 1, 63 (two ragged 32-pixel
    tiles) and 1023 pixels, channel counts on both sides of the 32-channel tile."""
    from centernet_amd import native
    lib = native.lib()
    B = 2
    for (H, W) in [(1, 1), (7, 9), (33, 31)]:
        for pitch in sorted({C, (C + 31) // 32 * 32}):
            x = torch.from_numpy(synth.normal((B, C, H, W), 1.0, 91 + C))
            xd = x.to(dev)
            y = torch.full((B, H, W, pitch), NAN, device=dev)
            native.check(lib.cn_nchw_to_nhwc_f32(native.ptr(xd), native.ptr(y), B, C, H, W, pitch,
                                                 native.stream_ptr()), "cn_nchw_to_nhwc_f32")
            torch.cuda.synchronize()
            got = y.cpu()
            assert _same_bits(got[..., :C], x.permute(0, 2, 3, 1).contiguous()), (H, W, pitch)
            if pitch > C:
                assert torch.equal(_bits(got[..., C:]), torch.zeros_like(_bits(got[..., C:]))), (H, W, pitch)
            y[..., C:] = NAN                      # pad channels the way back must not read
            z = torch.full((B, C, H, W), NAN, device=dev)
            native.check(lib.cn_nhwc_to_nchw_f32(native.ptr(y), native.ptr(z), B, C, H, W, pitch,
                                                 native.stream_ptr()), "cn_nhwc_to_nchw_f32")
            torch.cuda.synchronize()
            back = z.cpu()
            assert not torch.isnan(back).any(), (H, W, pitch)
            assert _same_bits(back, x), (H, W, pitch)


# ---- max-pool on negative data --------------------------------------------------------------------------
def _negative(shape, seed):
    return -torch.from_numpy(synth.normal(shape, 1.0, seed)).abs() - 0.1


@pytest.mark.parametrize("ksp", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
@pytest.mark.parametrize("shape", [(2, 4, 7, 9), (1, 36, 16, 5)])
def test_maxpool_plain_fp32_negative_input(dev, shape, ksp):
    """maxpool_nhwc_kernel<false> on a strictly negative map: a kernel that pads with 0 instead of -inf
    returns 0 along the border."""
    B, C, H, W = shape
    k, s, p = ksp
    x = _negative(shape, 101)
    pb = _plain_builder(dev, B, H, W)
    y = pb.maxpool(_act(x, dev), k, s, p)
    assert y.fmt == "f32"
    _run_filled(pb, y)
    assert _same_bits(_nchw(y), F.max_pool2d(x, k, s, p))


@pytest.mark.parametrize("ksp", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
def test_maxpool_f32s_to_f32s_negative_input(dev, ksp):
    """cn_maxpool_nhwc_f32s (f32s in, f32s out) on the same kind of map: max commutes with the join of a
    (high, low) pair, so the decoded output is max_pool2d of the decoded input, exactly."""
    from centernet_amd.engine import PlanBuilder
    B, C, H, W = 2, 32, 7, 9
    k, s, p = ksp
    pb = PlanBuilder(dev, B, H, W, split=True)
    xs = pb.packed(_act(_negative((B, C, H, W), 103), dev))
    y = pb.maxpool(xs, k, s, p, to_s=True)
    assert xs.fmt == "f32s" and y.fmt == "f32s"
    _run_filled(pb, y)
    xin = xs.to_float().permute(0, 3, 1, 2).cpu()
    assert bool((xin < 0).all())
    assert _same_bits(y.to_float().permute(0, 3, 1, 2).contiguous().cpu(), F.max_pool2d(xin, k, s, p))


# ---- cn_absmax_f32 --------------------------------------------------------------------------------------
def test_absmax_word(dev):
    """The word is the bit pattern of max |x| over the C real channels, accumulated with an integer atomic max
    (non-negative floats order like integers; cn_rng_commit1), +inf for any NaN / inf.  200 000 elements are
    more than the 512 x 256 threads of the grid, so the stride loop runs; the pad channels hold 1e30."""
    from centernet_amd import native
    lib = native.lib()
    npix, C, pitch = 8000, 25, 32
    x = torch.from_numpy(synth.normal((npix, pitch), 1.0, 111))
    x[:, C:] = 1e30
    x[6543, 21] = -7.25                            # the maximum is a negative value late in the tensor
    word = torch.zeros(1, device=dev, dtype=torch.int32)

    def absmax(t):
        td = t.to(dev)
        word.zero_()
        native.check(lib.cn_absmax_f32(native.ptr(td), npix, C, pitch, native.ptr(word), native.stream_ptr()),
                     "cn_absmax_f32")
        return int(word.cpu()[0])

    want = int(np.float32(float(x[:, :C].abs().max())).view(np.int32))
    assert want == int(np.float32(7.25).view(np.int32))
    assert absmax(x) == want
    INF = 0x7f800000
    for bad in (NAN, float("inf"), -float("inf")):
        t = x.clone()
        t[4321, 7] = bad
        assert absmax(t) == INF, bad
    # the word accumulates: a second call on smaller data leaves the larger value
    small = (x * 0.5).clone()
    small[:, C:] = 1e30
    td = small.to(dev)
    assert absmax(x) == want
    native.check(lib.cn_absmax_f32(native.ptr(td), npix, C, pitch, native.ptr(word), native.stream_ptr()),
                 "cn_absmax_f32")
    assert int(word.cpu()[0]) == want
