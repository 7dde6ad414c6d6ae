"""What the GPU tests of the deformable entry cn_dcn_v2_forward_nhwc share (tests/test_gpu_dcn_wide.py,
tests/test_gpu_dcn_route.py): seeded cases, sentinel-filled buffers, the bar against the C oracle, and one layer held
the way the engine holds it.  Not a test module.

The bar is that of tests/test_gpu_dcn.py: |diff| <= 2e-5 * (1 + |ref|) against the C oracle, which is
bit-identical to the reference's own kernel (tests/test_oracle_ref.py)."""
import ctypes

import numpy as np
import torch

from centernet_amd import native, synth

TOL = 2e-5
SENT = 0x7FC5A5A5          # a NaN no kernel produces: the fill of everything a launch may or may not write


def _check(y, ref, what=""):
    err = np.abs(y - ref) / (1 + np.abs(ref))
    if not err.max() < TOL:
        idx = np.unravel_index(np.argmax(err), err.shape)
        raise AssertionError("%s max err %.3e at %s (got %r, want %r); %d of %d cells beyond the bar"
                             % (what, err.max(), idx, float(y[idx]), float(ref[idx]), int((err >= TOL).sum()), err.size))


def _case(B, Cin, H, W, Cout, seed, off_std=2.0):
    x = synth.normal((B, Cin, H, W), 1.0, seed)
    w = synth.normal((Cout, Cin, 3, 3), (2.0 / (Cin * 9)) ** 0.5, seed + 1)
    b = synth.normal((Cout,), 0.1, seed + 2)
    off = synth.normal((B, 18, H, W), off_std, seed + 3)
    mask = 1.0 / (1.0 + np.exp(-synth.normal((B, 9, H, W), 1.0, seed + 4)))
    return x, off, mask.astype(np.float32), w, b


def _sentinel(shape, dev):
    t = torch.empty(shape, device=dev, dtype=torch.float32)
    t.view(torch.int32).fill_(SENT)
    return t


def _is_sentinel(t):
    return t.view(torch.int32) == SENT


class _Layer:
    """One deformable layer held the way PlanBuilder.dcn holds it (f32s-packed row-prescaled weight, input
    exponent in cn_f32s_ctl.x_mul, bias / scale / shift in stored units), launched through the C ABI with
    an output buffer, pitches and a workspace of the caller's choosing."""

    def __init__(self, dev, x, off, mask, w, b, om_pitch=32):
        from centernet_amd.engine import prescale_rows, exponent_for
        self.dev, self.lib = dev, native.lib()
        self.B, self.Cin, self.H, self.W = x.shape
        self.Cout = w.shape[0]
        self.x = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).to(dev)
        self.om_pitch = om_pitch
        self.om = {}
        for msig in (False, True):
            om = np.full((self.B, self.H, self.W, om_pitch), np.nan, np.float32)   # columns >= 27 are never read
            om[..., :18] = off.transpose(0, 2, 3, 1)
            m = mask.transpose(0, 2, 3, 1)
            if msig:
                m64 = m.astype(np.float64)
                m = np.log(m64 / (1.0 - m64)).astype(np.float32)
            om[..., 18:27] = m
            self.om[msig] = torch.from_numpy(om).to(dev)
        ws, self.factor = prescale_rows(torch.from_numpy(w).to(dev))
        ws = ws.contiguous()
        n = self.lib.cn_packed_conv_weight_elems(self.Cout, self.Cin, 3, 3, native.DTYPE_F32S)
        self.wp = torch.empty(n, device=dev, dtype=torch.float32)
        native.check(self.lib.cn_pack_conv_weight(native.ptr(ws), native.ptr(self.wp), self.Cout, self.Cin, 3, 3,
                                                  native.DTYPE_F32S, native.stream_ptr()), "cn_pack_conv_weight")
        self.ex = exponent_for(float(np.abs(x).max()))
        self.bias = torch.from_numpy(b).to(dev)
        self.ey_f32s = exponent_for(4.0 * float(np.abs(x).max()))
        self.ctl = native.F32sCtl()
        self.ctl.x_mul, self.ctl.res_mul, self.ctl.range = float(2.0 ** -self.ex), 1.0, None
        self.npix = self.B * self.H * self.W
        self.slab = self.npix * ((self.Cout + 31) // 32 * 32)     # floats of one K-split slab

    def _call(self, fn, more, out_plain, msig, scale, shift, relu, ey, pitch, c_off, ws, ws_bytes):
        from centernet_amd.engine import Act
        pitch = self.Cout if pitch is None else pitch
        ey = 0 if out_plain else (self.ey_f32s if ey is None else ey)
        bias = (self.bias * 2.0 ** -self.ex / self.factor).contiguous()
        sc = self.factor * 2.0 ** (self.ex - ey)
        if scale is not None:
            sc = sc * torch.from_numpy(scale).to(self.dev)
        sc = sc.contiguous()
        sh = None if shift is None else (torch.from_numpy(shift).to(self.dev) * 2.0 ** -ey).contiguous()
        t = _sentinel((self.B, self.H, self.W, pitch), self.dev)
        act = Act(t, self.B, self.H, self.W, self.Cout, pitch=pitch, c_off=c_off, fmt="f32" if out_plain else "f32s", exp=ey)
        rc = fn(
            native.ptr(self.x), native.ptr(self.wp), native.ptr(bias), native.ptr(self.om[bool(msig)]), self.om_pitch,
            native.ptr(sc), native.ptr(sh), act.ptr(), pitch, self.B, self.Cin, self.H, self.W, self.Cout, int(bool(msig)),
            int(bool(relu)), native.DTYPE_F32S, native.CONV_Y_PLAIN if out_plain else 0, ctypes.byref(self.ctl),
            native.ptr(ws), ws_bytes, native.stream_ptr(), *more)
        torch.cuda.synchronize()
        return rc, t, act

    def run(self, out_plain, msig=False, scale=None, shift=None, relu=False, ey=None, pitch=None, c_off=0,
            ws=None, ws_bytes=0):
        """-> (return code, the whole (B, H, W, pitch) output tensor, the Act of the member written)"""
        return self._call(self.lib.cn_dcn_v2_forward_nhwc, (), out_plain, msig, scale, shift, relu, ey, pitch, c_off,
                          ws, ws_bytes)

    def route(self, out_plain, msig=False, scale=None, shift=None, relu=False, ey=None, pitch=None, c_off=0,
              ws=None, ws_bytes=0):
        """what cn_dcn_v2_route says of the call run() would make, under the keys set now -> native.DcnRouteInfo"""
        info = native.DcnRouteInfo()
        rc = self._call(self.lib.cn_dcn_v2_route, (ctypes.byref(info),), out_plain, msig, scale, shift, relu, ey, pitch,
                        c_off, ws, ws_bytes)[0]
        assert rc == 0, rc
        return info

    def slabs_written(self, ws):
        """how many leading [B * H * W][cout_pad] slabs of the sentinel-filled workspace a launch wrote: the K
        split that ran.  A slab is written whole or not at all, and none behind an untouched one."""
        touched = [bool((~_is_sentinel(ws[k * self.slab:(k + 1) * self.slab])).any()) for k in range(ws.numel() // self.slab)]
        whole = [not bool(_is_sentinel(ws[k * self.slab:(k + 1) * self.slab]).any()) for k in range(ws.numel() // self.slab)]
        assert touched == whole, ("a partly written slab", touched, whole)
        n = sum(touched)
        assert touched == [True] * n + [False] * (len(touched) - n), touched
        return n

    def wgs(self, form):
        """workgroups of the unsplit launch with key 23 = form: tiles x blocks of output channels, from the query"""
        with native.tuning({23: form}):
            r = self.route(True)
        return r.grid_x * r.grid_y


def _nchw(act):
    return act.to_float().permute(0, 3, 1, 2).cpu().numpy()
