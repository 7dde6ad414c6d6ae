"""What the raw-ABI route tests share (tests/test_gpu_conv_route.py, tests/test_gpu_deconv_heads_route.py): the f32s
tensor format on the host and sentinel buffers between guards.  Not a test module."""
import torch

from dcn_cases import SENT

SENT16 = 0x7E5A            # a half NaN no kernel produces


# ---- f32s tensors: 32 channels = 32 fp16 high parts, then 32 fp16 low parts (csrc/cn_common.h) ---------------------
def pack_f32s(t):
    g = t.reshape(-1, t.shape[-1] // 32, 32)
    hi = g.half()
    lo = (g - hi.float()).half()
    return torch.cat([hi, lo], -1).contiguous().view(torch.float32).reshape(t.shape)


def unpack_f32s(t):
    g = t.reshape(-1, t.shape[-1] // 32, 32).contiguous().view(torch.float16)
    return (g[..., :32].float() + g[..., 32:].float()).reshape(t.shape)


class Buf:
    """`n` elements of 2 or 4 bytes between two guards, all sentinel; the body 256-byte aligned"""

    def __init__(self, dev, n, esize, guard):
        self.esize, self.n = esize, n
        self.g = (guard + 127) // 128 * 128
        self.sent = SENT16 if esize == 2 else SENT
        self.t = torch.empty(self.g + n + self.g, device=dev, dtype=torch.int16 if esize == 2 else torch.int32)
        self.t.fill_(self.sent)
        self.body = self.t[self.g:self.g + n]
        assert self.body.data_ptr() % 256 == 0

    def ptr(self, off=0):
        return self.body.data_ptr() + off * self.esize

    def is_sentinel(self, t):
        return t == self.sent

    def guards_untouched(self):
        return bool(self.is_sentinel(self.t[:self.g]).all()) and bool(self.is_sentinel(self.t[self.g + self.n:]).all())

    def values(self, fmt):
        """the body as floats: "f16" halves, "f32" floats (f32s tensors: still packed)"""
        return self.body.view(torch.float16 if fmt == "f16" else torch.float32)
