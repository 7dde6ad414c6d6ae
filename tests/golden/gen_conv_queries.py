"""Answers of the four host-only convolution queries over a fixed grid of descriptors ->
tests/golden/conv_queries.json.

    cn_conv2d_res_pitch_supported, cn_conv2d_workspace_bytes, cn_stem_maxpool_supported, cn_stem_f32s_supported

The file in the repository was written by the library as it was BEFORE the queries moved onto cn_conv.hip's
conv_route (CENTERNET_AMD_LIB pointing at a build of that commit); tests/test_conv_route_host.py asserts that
the library of the tree gives the same answers.  Needs no GPU.

    CENTERNET_AMD_LIB=/path/to/libcenternet_amd.so python tests/golden/gen_conv_queries.py
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_queries.json")

BATCHES = (1, 8, 32)
# (Cin, Cout, H, W): the trunk layers of resdcn_18 and dla_34 at a 512 x 512 image (input side of the layer),
# a deep layer on a 4 x 4 map and a 32 -> 64 layer on one 8 x 16 tile
PAIRS = (
    (16, 16, 512, 512), (16, 32, 512, 512), (32, 64, 256, 256),                       # dla_34 level0 .. level2
    (64, 64, 128, 128), (64, 128, 128, 128), (128, 128, 64, 64), (128, 256, 64, 64),   # both trunks
    (256, 256, 32, 32), (256, 512, 32, 32), (512, 512, 16, 16),
    (512, 512, 4, 4), (32, 64, 8, 16),
)
FORMS = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1))       # kernel, stride, pad
F32, F16, F32S = 0, 1, 2
X_PLAIN, Y_PLAIN, R_PLAIN, STEM_F32S, STEM_MAXPOOL, STEM_Y_F32S = 1, 2, 4, 8, 16, 32
# dtype, flags: the plain flags mean something to f32s layers only
DTYPE_FLAGS = ((F32, 0), (F16, 0)) + tuple((F32S, f) for f in range(8))
STEM_SIZES = ((512, 512), (128, 128), (64, 256))            # H, W of the image
STEM_FLAGS = (0, STEM_F32S, STEM_MAXPOOL, STEM_F32S | STEM_MAXPOOL, STEM_F32S | STEM_MAXPOOL | STEM_Y_F32S)
# cn_set_tuning: the defaults, then one key flipped at a time
KNOBS = ({}, {5: 1}, {6: 1}, {10: 1}, {12: 0}, {27: 0})


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _r32(c):
    return (c + 31) // 32 * 32


def descriptors():
    """The grid, in a fixed order."""
    from centernet_amd.native import ConvDesc, LAYOUT_NCHW, LAYOUT_NHWC
    for B in BATCHES:
        for (ci, co, H, W) in PAIRS:
            for (k, s, p) in FORMS:
                Ho, Wo = _out(H, k, s, p), _out(W, k, s, p)
                for (dt, fl) in DTYPE_FLAGS:
                    ip = _r32(ci) if (dt == F32S and not fl & X_PLAIN) else ci
                    op = _r32(co) if (dt == F32S and not fl & Y_PLAIN) else co
                    for rp in (0, 2 * co):
                        yield ConvDesc(B=B, H=H, W=W, Cin=ci, Ho=Ho, Wo=Wo, Cout=co, KH=k, KW=k, stride=s,
                                       pad_h=p, pad_w=p, dil=1, in_layout=LAYOUT_NHWC, in_pitch=ip,
                                       out_layout=LAYOUT_NHWC, out_pitch=op, OH=Ho, OW=Wo, oy_mul=1, ox_mul=1,
                                       relu=1, dtype=dt, flags=fl, res_pitch=rp)
        # the stems: 7x7 / pad 3 on the 3-channel NCHW image
        for (H, W) in STEM_SIZES:
            for s in (2, 1):
                Ho, Wo = _out(H, 7, s, 3), _out(W, 7, s, 3)
                for co in (16, 64):
                    for dt in (F32, F16, F32S):
                        for fl in STEM_FLAGS:
                            op = _r32(co) if fl & STEM_Y_F32S else co
                            yield ConvDesc(B=B, H=H, W=W, Cin=3, Ho=Ho, Wo=Wo, Cout=co, KH=7, KW=7, stride=s,
                                           pad_h=3, pad_w=3, dil=1, in_layout=LAYOUT_NCHW, in_pitch=0,
                                           out_layout=LAYOUT_NHWC, out_pitch=op, OH=Ho, OW=Wo, oy_mul=1,
                                           ox_mul=1, relu=1, dtype=dt, flags=fl)


def answers():
    """{knob setting: {query: one character per descriptor of the grid}}.  The 0 / 1 queries as digits; the
    workspace as the number of K slices it holds (bytes / (4 B Ho Wo Cout_pad32), base 36, 0 = no workspace).
    A flipped key lists only the queries whose answers differ from the defaults'."""
    from centernet_amd import native
    lib = native.lib()
    grid = list(descriptors())
    out = {"n": len(grid), "knobs": {}}
    digits = "0123456789abcdefghijklmnopqrstuvwxyz"
    for knobs in KNOBS:
        with native.tuning(knobs):
            refs = [ctypes.byref(d) for d in grid]
            ws = []
            for d, r in zip(grid, refs):
                b, slab = int(lib.cn_conv2d_workspace_bytes(r)), 4 * d.B * d.Ho * d.Wo * _r32(d.Cout)
                assert b % slab == 0 and b // slab < 36, (b, slab)
                ws.append(digits[b // slab])
            got = {
                "res_pitch": "".join(str(int(lib.cn_conv2d_res_pitch_supported(r))) for r in refs),
                "stem_maxpool": "".join(str(int(lib.cn_stem_maxpool_supported(r))) for r in refs),
                "stem_f32s": "".join(str(int(lib.cn_stem_f32s_supported(r))) for r in refs),
                "workspace": "".join(ws),
            }
        base = out["knobs"].get("{}", {})
        out["knobs"][json.dumps(knobs, sort_keys=True)] = {q: v for q, v in got.items() if v != base.get(q)}
    return out


if __name__ == "__main__":
    a = answers()
    with open(OUT, "w") as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in a["knobs"].items():
        print(k, {q: len(x) - x.count("0") for q, x in v.items()}, "of", a["n"])
