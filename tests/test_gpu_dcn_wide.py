"""The wide deformable form (csrc/cn_dcn4.hip, cn_set_tuning key 23 = 6 / 7) through the C ABI
cn_dcn_v2_forward_nhwc, with every branch of its launcher reached on purpose: the K split that ran is
READ BACK from a workspace the test owns (sentinel fill, slabs counted), not inferred from the shape.

  * K split 1 / 2 / 4 / 8 steered with key 42, each reached, each against the C oracle, bit-identical
    when repeated; a workspace one float short of split s runs the next smaller split and leaves the
    bytes behind `workspace_bytes` alone; no workspace -> split 1;
  * out_pitch > Cout (a member of a concatenation buffer, f32s and plain), om_pitch 27 / 40;
  * the BatchNorm-fold + ReLU epilogue against the oracle's output transformed in fp64;
  * shapes the form does not take fall through to the next form and still meet the bar;
  * identical bits over 50 launches while a second stream keeps the chip busy.

The bar is that of tests/test_gpu_dcn.py: |diff| <= 2e-5 * (1 + |ref|) against the C oracle, which is
bit-identical to the reference's own kernel (tests/test_oracle_ref.py).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from centernet_amd import native, synth
from oracle import cref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dcn_cases import TOL, _Layer, _case, _check, _is_sentinel, _nchw, _sentinel   # noqa: E402

pytestmark = pytest.mark.gpu
WIDE_FORMS = [6, 7]        # 6: blocks of 32 output channels per workgroup by shape (8 at Cout % 256 == 0), 7: four


@pytest.fixture(autouse=True)
def _default_tuning():
    """Every test of this module leaves the cn_set_tuning keys at the library's defaults."""
    yield
    native.lib().cn_reset_tuning()


def _key42_for(split, wgs):
    """the smallest 'K split until a launch has this many workgroups' (key 42) that asks for `split`"""
    return 1 if split == 1 else wgs * split // 2 + 1


@pytest.mark.parametrize("form", WIDE_FORMS)
@pytest.mark.parametrize("shape,splits", [((2, 512, 16, 16, 256), (1, 2, 4, 8)),      # 16 chunks
                                          ((2, 256, 16, 16, 128), (1, 2, 4))])         # 8 chunks: >= 2 per workgroup
def test_every_k_split_is_reached_and_right(dev, shape, splits, form):
    B, Cin, H, W, Cout = shape
    x, off, mask, w, b = _case(B, Cin, H, W, Cout, 4100 + Cin, off_std=1.5)
    want = cref.dcn_v2_forward(x, off, mask, w, b)
    L = _Layer(dev, x, off, mask, w, b)
    guard = 4096
    reached = set()
    for split in splits:
        with native.tuning({23: form, 42: _key42_for(split, L.wgs(form))}):
            for out_plain in (False, True):
                for msig in (False, True):
                    first = None
                    for rep in range(2):
                        ws = _sentinel((8 * L.slab + guard,), dev)
                        rc, t, act = L.run(out_plain, msig=msig, ws=ws, ws_bytes=8 * L.slab * 4)
                        assert rc == 0
                        ran = L.slabs_written(ws[:8 * L.slab])
                        ran = 1 if ran == 0 else ran              # split 1 writes no slab at all
                        assert ran == split, (form, split, ran)
                        assert bool(_is_sentinel(ws[8 * L.slab:]).all())
                        reached.add(ran)
                        _check(_nchw(act), want, "form %d split %d plain %d msig %d:" % (form, split, out_plain, msig))
                        if first is None:
                            first = t.clone()
                        assert torch.equal(t.view(torch.int32), first.view(torch.int32))   # same bits when repeated
    print("form %d, %d -> %d: K splits reached %s" % (form, Cin, Cout, sorted(reached)))
    assert reached == set(splits)
    if 8 not in splits:
        # eight chunks leave one per workgroup at split 8: the launcher stays at 4 however many are asked for
        with native.tuning({23: form, 42: 4096}):
            ws = _sentinel((8 * L.slab,), dev)
            rc, t, act = L.run(False, ws=ws, ws_bytes=8 * L.slab * 4)
            assert rc == 0 and L.slabs_written(ws) == 4
            _check(_nchw(act), want)


@pytest.mark.parametrize("form", WIDE_FORMS)
def test_a_short_workspace_runs_the_next_smaller_split(dev, form):
    B, Cin, H, W, Cout = 2, 512, 16, 16, 256
    x, off, mask, w, b = _case(B, Cin, H, W, Cout, 4300, off_std=1.5)
    want = cref.dcn_v2_forward(x, off, mask, w, b)
    L = _Layer(dev, x, off, mask, w, b)
    for split in (2, 4, 8):
        with native.tuning({23: form, 42: _key42_for(split, L.wgs(form))}):
            for out_plain in (False, True):
                ws = _sentinel((8 * L.slab,), dev)
                nbytes = split * L.slab * 4 - 4                  # one float short of what `split` needs
                rc, t, act = L.run(out_plain, ws=ws, ws_bytes=nbytes)
                assert rc == 0
                # everything behind workspace_bytes keeps its sentinel (the last float of slab `split` included)
                assert bool(_is_sentinel(ws[nbytes // 4:]).all()), (form, split)
                ran = L.slabs_written(ws)
                assert ran == (split // 2 if split > 2 else 0), (form, split, ran)     # split 1 writes no slab
                _check(_nchw(act), want, "form %d, workspace short of split %d:" % (form, split))
    with native.tuning({23: form, 42: 4096}):
        rc, t, act = L.run(False, ws=None, ws_bytes=0)           # no workspace at all: split 1
        assert rc == 0
        _check(_nchw(act), want, "no workspace:")
        ws = _sentinel((8 * L.slab,), dev)
        rc, t, act = L.run(False, ws=ws, ws_bytes=0)             # a workspace of no bytes
        assert rc == 0 and bool(_is_sentinel(ws).all())
        _check(_nchw(act), want, "workspace of 0 bytes:")


@pytest.mark.parametrize("form", WIDE_FORMS)
@pytest.mark.parametrize("split", [1, 2])
def test_a_member_of_a_wider_buffer_and_other_offset_pitches(dev, form, split):
    """out_pitch > Cout: 128 channels written as the member at channel offset 64 / 32 of a pitch-256 / 192
    buffer, addressed as the engine addresses concat members (base + c_off, pitch of the buffer; f32s: a
    member starts on a 32-channel group): every column outside the member keeps its sentinel.  Directly
    and through the K split's reduce kernel.  om_pitch 27 (no padding) and 40."""
    B, Cin, H, W, Cout = 2, 256, 16, 16, 128
    x, off, mask, w, b = _case(B, Cin, H, W, Cout, 4400)
    want = cref.dcn_v2_forward(x, off, mask, w, b)
    for om_pitch in (32, 27, 40):
        L = _Layer(dev, x, off, mask, w, b, om_pitch=om_pitch)
        with native.tuning({23: form, 42: _key42_for(split, L.wgs(form))}):
            for out_plain in (False, True):
                for pitch, c_off in ((256, 64), (192, 32)) if om_pitch == 32 else ((256, 96),):
                    ws = _sentinel((8 * L.slab,), dev)
                    rc, t, act = L.run(out_plain, msig=True, pitch=pitch, c_off=c_off, ws=ws, ws_bytes=8 * L.slab * 4)
                    assert rc == 0
                    assert max(L.slabs_written(ws), 1) == split
                    s = _is_sentinel(t)
                    assert bool(s[..., :c_off].all()) and bool(s[..., c_off + Cout:].all()), (form, out_plain, pitch, c_off)
                    assert not bool(s[..., c_off:c_off + Cout].any())
                    _check(_nchw(act), want, "form %d om_pitch %d plain %d pitch %d + %d:" % (form, om_pitch, out_plain, pitch, c_off))


@pytest.mark.parametrize("form", WIDE_FORMS)
@pytest.mark.parametrize("split", [1, 2])
def test_batchnorm_fold_and_relu_epilogue(dev, form, split):
    """y = relu?((acc + bias) * scale + shift) with per-channel scale and shift, against the oracle's output
    transformed in fp64; the shift centres the outputs so that the ReLU zeroes about half of them (a missing
    clamp cannot pass) and scale and shift differ in sign and size (swapped, they cannot pass)."""
    B, Cin, H, W, Cout = 2, 256, 16, 16, 256
    x, off, mask, w, b = _case(B, Cin, H, W, Cout, 4500)
    conv = cref.dcn_v2_forward(x, off, mask, w, b).astype(np.float64)
    scale = synth.uniform((Cout,), 0.5, 1.5, 4501) * np.where(np.arange(Cout) % 5 == 0, -1.0, 1.0).astype(np.float32)
    shift = (-np.median(conv, axis=(0, 2, 3)) * scale).astype(np.float32) + synth.normal((Cout,), 0.05, 4502)
    lin = conv * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
    L = _Layer(dev, x, off, mask, w, b)
    from centernet_amd.engine import exponent_for
    with native.tuning({23: form, 42: _key42_for(split, L.wgs(form))}):
        for relu in (False, True):
            want = np.maximum(lin, 0.0) if relu else lin
            if relu:
                zeros = float((want == 0).mean())
                assert 0.35 < zeros < 0.65, zeros
            for out_plain in (False, True):
                ws = _sentinel((8 * L.slab,), dev)
                rc, t, act = L.run(out_plain, msig=True, scale=scale, shift=shift, relu=relu,
                                   ey=exponent_for(float(np.abs(want).max())), ws=ws, ws_bytes=8 * L.slab * 4)
                assert rc == 0 and max(L.slabs_written(ws), 1) == split
                got = _nchw(act)
                _check(got, want.astype(np.float32), "form %d split %d relu %d plain %d:" % (form, split, relu, out_plain))
                if relu:
                    assert got.min() >= 0.0 and abs(float((got == 0).mean()) - zeros) < 0.01


@pytest.mark.parametrize("shape", [(2, 64, 12, 16, 128),      # H % 8 != 0
                                   (2, 64, 8, 24, 128),       # W % 16 != 0
                                   (2, 48, 8, 16, 128),       # Cin % 32 != 0
                                   (2, 64, 8, 16, 64)])       # Cout % 128 != 0
def test_shapes_the_wide_form_does_not_take_fall_through(dev, shape):
    """form 6 forced on a shape outside its domain: CN_OK through the next form, same bar"""
    B, Cin, H, W, Cout = shape
    x, off, mask, w, b = _case(B, Cin, H, W, Cout, 4600 + H + W + Cin + Cout)
    want = cref.dcn_v2_forward(x, off, mask, w, b)
    L = _Layer(dev, x, off, mask, w, b)
    need = native.lib().cn_dcn_v2_forward_nhwc_workspace_bytes(B, Cin, H, W, Cout)
    with native.tuning({23: 6}):
        for out_plain in (False, True):
            for msig in (False, True):
                ws = _sentinel((need // 4 + 64,), dev)
                rc, t, act = L.run(out_plain, msig=msig, ws=ws, ws_bytes=need)
                assert rc == 0, rc
                assert bool(_is_sentinel(ws[need // 4:]).all())
                assert not bool(_is_sentinel(t).any())
                _check(_nchw(act), want, "%r plain %d msig %d:" % (shape, out_plain, msig))


# ---- identical bits under a busy chip ------------------------------------------------------------------------
LAUNCHES = 50          # fixed: a determinism check with a correctness purpose, not a search for a fault
SIDE_LAUNCHES = 100    # fixed length of the second stream's loop


@pytest.mark.parametrize("shape", [(256, 32, 256), (256, 32, 128), (512, 16, 256), (128, 64, 128)])
def test_identical_bits_over_fifty_launches_beside_a_busy_second_stream(dev, shape):
    """The four wide-form layer shapes at B = 32 under the library's default selection (the wide form; K split
    on the 16^2 map): 50 launches on one stream while a second stream runs the persistent 3x3 convolution of
    the same map and width, every result kept on the device and compared with the first, images 0, 13 and 31
    of the first against the C oracle.  The comparison stops at the first mismatch; a mismatch is a finding to
    explain from the barrier audit (tests/test_isa_audit.py), not something to run again."""
    from centernet_amd.engine import PlanBuilder, Act
    Cin, HW, Cout = shape
    B = 32
    x, off, mask, w, b = _case(B, Cin, HW, HW, Cout, 4700 + Cin + Cout)
    L = _Layer(dev, x, off, mask, w, b)
    need = native.lib().cn_dcn_v2_forward_nhwc_workspace_bytes(B, Cin, HW, HW, Cout)
    ws = _sentinel((max(need // 4, 4),), dev)
    # the second stream's work: a 3x3 / stride 1 convolution Cin -> Cin on the same map, f32s, persistent kernel
    pb = PlanBuilder(dev, B, HW, HW, split=True)
    xa = pb.packed(Act(L.x, B, HW, HW, Cin))
    pb.conv(xa, torch.from_numpy(synth.normal((Cin, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, 4799)), padding=1)
    convert, side_ops = pb.ops[0], pb.ops[1:]
    assert side_ops
    convert()
    torch.cuda.synchronize()
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [_sentinel((B, HW, HW, Cout), dev) for _ in range(LAUNCHES)]
    bias = (L.bias * 2.0 ** -L.ex / L.factor).contiguous()
    sc = (L.factor * 2.0 ** (L.ex - L.ey_f32s)).contiguous()
    torch.cuda.synchronize()
    lib = native.lib()
    for i in range(LAUNCHES):
        with torch.cuda.stream(side):
            for _ in range(SIDE_LAUNCHES // LAUNCHES):
                for op in side_ops:
                    op()
        with torch.cuda.stream(main):
            rc = lib.cn_dcn_v2_forward_nhwc(
                native.ptr(L.x), native.ptr(L.wp), native.ptr(bias), native.ptr(L.om[True]), 32, native.ptr(sc), None,
                native.ptr(outs[i]), Cout, B, Cin, HW, HW, Cout, 1, 0, native.DTYPE_F32S, 0, ctypes.byref(L.ctl),
                native.ptr(ws), need, native.stream_ptr())
        assert rc == 0
    torch.cuda.synchronize()
    first = outs[0].view(torch.int32)
    assert not bool(_is_sentinel(outs[0]).any())
    for i in range(1, LAUNCHES):
        assert torch.equal(outs[i].view(torch.int32), first), "launch %d differs from launch 0 in %d words" % (
            i, int((outs[i].view(torch.int32) != first).sum()))
    y = _nchw(Act(outs[0], B, HW, HW, Cout, fmt="f32s", exp=L.ey_f32s))
    for i in (0, 13, 31):
        _check(y[i:i + 1], cref.dcn_v2_forward(x[i:i + 1], off[i:i + 1], mask[i:i + 1], w, b), "image %d:" % i)
