#!/usr/bin/env python
"""Golden vectors for exct_decode / agnex_ct_decode at K > 64 (the streaming grouping's range), produced by
RUNNING the reference's src/lib/models/decode.py on CPU tensors.  Only the `dets` arrays are kept; the
reference materialises (B, K^4) tensors, so the K = 128 case needs about 22 GB of host memory.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_exct_bigk.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

EXCT_BIGK_CASES = {
    # name: (B, C, H, W, K, num_dets, regr)
    "exct_k72": (1, 4, 64, 64, 72, 1000, True),       # few rule-free groupings: the cut lies in the penalty tail
    "exct_k100": (1, 4, 64, 64, 100, 1000, True),     # the reference's --K default
    "exct_k128": (1, 2, 32, 32, 128, 1000, True),     # the largest K (K^4 = 2^28)
}
AGNEX_BIGK_CASES = {
    # name: (B, classes of the centre map, H, W, K, num_dets, regr, aggr_weight)
    "agnex_k100": (1, 80, 64, 64, 100, 1000, True, 0.0),
}


def _sibling(name, table_name, table):
    """A private instance of a sibling generator with this file's case table: the same input construction and
    seed rule (3000 / 7000 + sum(ord(name))), other cases."""
    spec = importlib.util.spec_from_file_location("_bigk_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    setattr(mod, table_name, table)
    return mod


_EXCT = _sibling("gen_golden_exct", "EXCT_CASES", EXCT_BIGK_CASES)
_AGNEX = _sibling("gen_golden_agnex", "AGNEX_CASES", AGNEX_BIGK_CASES)


def exct_inputs(name):
    return _EXCT.exct_inputs(name)


def agnex_inputs(name):
    return _AGNEX.agnex_inputs(name)


def stats(dets):
    """(rows with a positive score, distinct scores, length of the run of equal scores that ends at the cut)"""
    s = dets[..., 4].reshape(-1)
    run = 1
    while run < len(s) and s[len(s) - 1 - run] == s[-1]:
        run += 1
    return int((s > 0).sum()), len(np.unique(s)), run


def main():
    import torch
    sys.path.insert(0, "/root/reference/src/lib")
    import models.decode as ref_decode

    def t(a):
        return None if a is None else torch.from_numpy(a.copy())
    out = {}
    for cases, inputs, fn in ((EXCT_BIGK_CASES, exct_inputs, ref_decode.exct_decode),
                              (AGNEX_BIGK_CASES, agnex_inputs, ref_decode.agnex_ct_decode)):
        for name in cases:
            heats, regs, K, num_dets = inputs(name)
            with torch.no_grad():
                dets = fn(*[t(h) for h in heats], *[t(r) for r in regs], K=K, num_dets=num_dets).numpy()
            out[name + "/dets"] = dets
            print(name, dets.shape, "positive: %d  distinct scores: %d  tie run at the cut: %d" % stats(dets),
                  flush=True)
    np.savez_compressed(os.path.join(HERE, "exct_bigk_golden.npz"), **out)


if __name__ == "__main__":
    main()
