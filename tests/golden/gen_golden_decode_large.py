#!/usr/bin/env python
"""Golden vectors for ctdet_decode at K > 128 (the range of the large-K image-level top-K), produced by RUNNING the
reference's src/lib/models/decode.py on seeded CPU tensors.  Only the `dets` arrays are kept.

The inputs are chosen so that every score of the K best is unique within its image (asserted here): torch.topk
leaves the order of equal scores open, and with unique scores every row of the reference is determined -- a test can
compare whole rows everywhere and must find no row to leave out.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_decode_large.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

DECODE_LARGE_CASES = {
    # name: (B, C, H, W, K, fraction of the cells set to zero)
    "small_k300": (2, 3, 32, 32, 300, 0.0),       # K near the number of peaks of an image
    "tall_k1000": (1, 2, 132, 128, 1000, 0.0),    # a plane past 128 rows, K just below the limit
    "sparse_k500": (2, 4, 64, 64, 500, 0.6),      # most cells exactly zero: plateaus of tied zeros around the peaks
}


def decode_large_inputs(name):
    """(heat, wh, reg, K) of a case, float32 arrays from seeds derived from the name."""
    from centernet_amd import synth
    B, C, H, W, K, zero_frac = DECODE_LARGE_CASES[name]
    seed = 9000 + sum(ord(ch) for ch in name)
    heat = synth.heatmap((B, C, H, W), seed)
    if zero_frac:
        heat = np.where(synth.uniform((B, C, H, W), 0, 1, seed + 1) < zero_frac, np.float32(0), heat)
    wh = synth.uniform((B, 2, H, W), 0, 40, seed + 2)
    reg = synth.uniform((B, 2, H, W), 0, 1, seed + 3)
    return np.ascontiguousarray(heat, np.float32), wh, reg, K


def unique_rows(dets):
    """(B, K) bool: the score of the row occurs once in its image."""
    s = dets[..., 4]
    return np.stack([np.array([(row == v).sum() == 1 for v in row]) for row in s])


def main():
    import torch
    sys.path.insert(0, "/root/reference/src/lib")
    import models.decode as ref_decode

    out = {}
    for name in DECODE_LARGE_CASES:
        heat, wh, reg, K = decode_large_inputs(name)
        with torch.no_grad():
            dets = ref_decode.ctdet_decode(torch.from_numpy(heat.copy()), torch.from_numpy(wh.copy()),
                                           reg=torch.from_numpy(reg.copy()), K=K).numpy()
        assert dets.shape == (heat.shape[0], K, 6) and dets.dtype == np.float32
        assert unique_rows(dets).all() and (dets[..., 4] > 0).all(), name     # every row is determined
        out[name + "/dets"] = dets
        print(name, dets.shape, "lowest score %.3e" % float(dets[..., 4].min()), flush=True)
    np.savez_compressed(os.path.join(HERE, "decode_large_golden.npz"), **out)


if __name__ == "__main__":
    main()
