"""The large-K image-level top-K (csrc/cn_decode_large.hip), host side: the three prototypes in the header, the exported
symbols and their bindings, the workspace query, the --max_per_image flag, and the oracle against the reference's
goldens at K = 300, 500 and 1000.  No GPU."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from oracle import cref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load_gen():
    spec = importlib.util.spec_from_file_location("gen_golden_decode_large",
                                                  os.path.join(HERE, "golden", "gen_golden_decode_large.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = load_gen()
GOLD = np.load(os.path.join(HERE, "golden", "decode_large_golden.npz"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_matches_golden(dets, gold):
    """Scores bit for bit everywhere, whole rows wherever the score is unique in its image -- and on these
    inputs that is every row: the rule may not hide a failure."""
    assert dets.shape == gold.shape
    assert np.array_equal(bits(dets[..., 4]), bits(gold[..., 4]))
    unique = GEN.unique_rows(gold)
    assert int((~unique).sum()) == 0
    assert np.array_equal(bits(dets)[unique], bits(gold)[unique])


def test_golden_file_holds_only_the_rows():
    assert set(GOLD.files) == {n + "/dets" for n in GEN.DECODE_LARGE_CASES}
    for name, (B, C, H, W, K, _) in GEN.DECODE_LARGE_CASES.items():
        assert GOLD[name + "/dets"].shape == (B, K, 6) and GOLD[name + "/dets"].dtype == np.float32
        assert 128 < K <= 1024


@pytest.mark.parametrize("name", sorted(GEN.DECODE_LARGE_CASES))
def test_oracle_reproduces_the_reference_at_large_k(name):
    heat, wh, reg, K = GEN.decode_large_inputs(name)
    assert_matches_golden(cref.ctdet_decode(heat, wh, reg, K=K), GOLD[name + "/dets"])


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "centernet_amd.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert "#define CN_DECODE_LARGE_MAX_K 1024" in text
    assert "size_t cn_ctdet_decode_large_workspace_bytes(int B, int C, int H, int W, int K);" in text
    # the parameter lists of the K <= 128 entries
    for new, old in (("cn_ctdet_decode_large_f32", "cn_ctdet_decode_f32"), ("cn_topk_large_f32", "cn_topk_f32")):
        params = {n: re.search(r"int %s\(([^)]*)\);" % n, text) for n in (new, old)}
        assert params[new] and params[old], new
        assert params[new].group(1) == params[old].group(1)


def test_symbols_and_bindings():
    from centernet_amd import native
    lib = native.lib()
    raw = ctypes.CDLL(lib._name)
    for name in ("cn_ctdet_decode_large_workspace_bytes", "cn_ctdet_decode_large_f32", "cn_topk_large_f32"):
        assert hasattr(raw, name), name
    assert native.DECODE_LARGE_MAX_K == 1024
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert lib.cn_ctdet_decode_large_workspace_bytes.argtypes == [i] * 5
    assert lib.cn_ctdet_decode_large_workspace_bytes.restype is sz
    assert lib.cn_ctdet_decode_large_f32.argtypes == [vp, vp, vp] + [i] * 7 + [vp, vp, vp, sz, vp]
    assert lib.cn_topk_large_f32.argtypes == [vp] + [i] * 6 + [vp, vp, vp, vp, sz, vp]
    assert lib.cn_ctdet_decode_large_f32.restype is i and lib.cn_topk_large_f32.restype is i
    assert lib.cn_version() == 313


def test_workspace_query():
    from centernet_amd import native
    q = native.lib().cn_ctdet_decode_large_workspace_bytes
    # refused for the shape or K: 0
    assert q(2, 3, 32, 32, 1025) == 0 and q(2, 3, 32, 32, 0) == 0 and q(2, 3, 32, 32, -1) == 0
    assert q(1, 3, 16, 16, 257) == 0                        # K > H*W
    assert q(0, 3, 32, 32, 300) == 0 and q(2, 0, 32, 32, 300) == 0 and q(2, 3, 0, 32, 300) == 0
    assert q(1, 1, 4, 8192, 300) == 0                       # a row longer than the form takes
    for shape in ((2, 3, 32, 32, 129), (2, 3, 32, 32, 1000), (1, 1, 32, 32, 1024), (2, 5, 23, 17, 391),
                  (1, 2, 132, 128, 1000), (32, 80, 128, 128, 1024), (1, 80, 128, 128, 1), (3, 7, 64, 64, 100)):
        B, C, H, W, K = shape
        n = q(*shape)
        assert n > 0 and n % 16 == 0, shape
        assert n >= B * C * min(K, H * W) * 8, shape        # every plane can hand on its K best keys


def test_null_and_shape_are_refused_without_a_device():
    """The checks in front of the launch need no device: NULL, shape and K are answered on the host."""
    from centernet_amd import native
    lib = native.lib()
    NULL, SHAPE, UNSUP = -5, -1, -2
    buf = (ctypes.c_char * 512)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)     # 16-byte aligned, never dereferenced

    def ctdet(heat=p, B=1, C=1, H=32, W=32, K=300):
        return lib.cn_ctdet_decode_large_f32(heat, p, None, B, C, H, W, K, 0, 0, p, None, None, 0, None)

    def topk(heat=p, B=1, C=1, H=32, W=32, K=300):
        return lib.cn_topk_large_f32(heat, B, C, H, W, K, 0, p, p, p, None, 0, None)
    for call in (ctdet, topk):
        assert call(heat=None) == NULL
        assert call(heat=None, K=0) == NULL                 # NULL before SHAPE
        assert call(B=0) == SHAPE and call(K=0) == SHAPE and call(K=1025) == SHAPE     # 1025 > 32 * 32
        assert call(H=64, K=1025) == UNSUP
        assert call(B=0, H=64, K=1025) == SHAPE             # SHAPE before UNSUPPORTED
        assert call() == NULL                               # a good shape, no workspace: refused, nothing launched


def test_max_per_image_flag(monkeypatch):
    from centernet_amd.opts import opts
    plain = opts().init(["ctdet"])
    assert plain.max_per_image == 100
    flagged = opts().init(["ctdet", "--K", "300", "--max_per_image", "300"])
    assert flagged.max_per_image == 300 and flagged.K == 300
    a, b = dict(vars(plain)), dict(vars(opts().init(["ctdet", "--max_per_image", "250"])))
    assert b.pop("max_per_image") == 250 and a.pop("max_per_image") == 100 and a == b
    # ... and reaches the detector (a stand-in network: no device is touched)
    from centernet_amd.detectors import base_detector

    class Net(object):
        def to(self, device):
            return self

        def eval(self):
            return self

        def defer_heads(self, names):
            self.deferred = names
    monkeypatch.setattr(base_detector, "create_model", lambda *a, **k: Net())
    from centernet_amd.detectors.ctdet import CtdetDetector
    assert CtdetDetector(flagged).max_per_image == 300
    assert CtdetDetector(plain).max_per_image == 100
    flagged.max_per_image = 0
    with pytest.raises(ValueError, match="max_per_image"):
        CtdetDetector(flagged)
