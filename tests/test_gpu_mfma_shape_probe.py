"""cn_calib_mfma_shape (csrc/cn_misc.hip; tools/bench_mfma_shape.py): the measurement aid behind the MFMA shape of
the persistent 3x3 kernel.  No reference counterpart and no output to compare: the launch arithmetic it reports, the
stamps of the stamped build, the untouched sink, and the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu
OPERAND_BYTES = 98304      # CN_CALIB_SHAPE_OPERAND_BYTES


def test_both_shapes_and_arrangements_launch_and_stamp(dev):
    from centernet_amd import native
    lib = native.lib()
    st, p = native.stream_ptr(), native.ptr
    g = torch.Generator().manual_seed(3)
    ops = torch.randn(OPERAND_BYTES // 2, generator=g).to(torch.float16).to(dev)
    sink = torch.zeros(64, device=dev)
    stamps = torch.zeros(2 * 256, device=dev, dtype=torch.int64)
    iters = 200
    flops = 256 * 8 * iters * 3 * 2 * 64 * 32 * 32
    for shape in (32, 16):
        for from_lds in (0, 1):
            assert lib.cn_calib_mfma_shape(p(ops), p(sink), None, shape, from_lds, iters, st) == flops
            stamps.zero_()
            assert lib.cn_calib_mfma_shape(p(ops), p(sink), p(stamps), shape, from_lds, iters, st) == flops
            torch.cuda.synchronize()
            s = stamps.view(256, 2).cpu().double()
            assert bool((s[:, 1] > 0).all()), "every workgroup stamps its loop"
            # one wave's loop: at least its own 384 matrix cycles per step, at most the pair's with slack
            cyc = s[:, 0] / iters
            assert 380.0 <= float(cyc.min()) and float(cyc.max()) < 4 * 768.0, (shape, from_lds, float(cyc.min()), float(cyc.max()))
            mhz = 100.0 * s[:, 0] / s[:, 1]
            assert 300.0 < float(mhz.min()) and float(mhz.max()) < 5000.0
    assert float(sink.abs().max()) == 0.0
    assert lib.cn_calib_mfma_shape(p(ops), p(sink), None, 8, 0, iters, st) == 0.0
    assert lib.cn_calib_mfma_shape(None, p(sink), None, 16, 0, iters, st) == 0.0
    assert lib.cn_calib_mfma_shape(p(ops), None, None, 16, 0, iters, st) == 0.0
    assert lib.cn_calib_mfma_shape(p(ops), p(sink), None, 16, 0, 0, st) == 0.0
    torch.cuda.synchronize()
