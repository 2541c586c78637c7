#!/usr/bin/env python3
"""Writes tests/golden/din_train_csr_tolerances.json: the constants k of the bound |gpu - ref| <= k[tensor] eps32 A of
tests/test_gpu_din_train_csr.py (ref, A: the ROW step of tests/train_ref.py in float64 on the expanded rows, A through
train_ref.element_scale; eps32 = 2^-24).  Runs on the CPU; never derived from what the device gives.

For every GPU case the ragged restatement (tests/din_train_csr_ref.py) is run in float32 twice, every sum in order and reversed, and
compared with the float64 row step: ratio = max |f32 - f64| / (eps32 A) per tensor.  k = 8 x the largest ratio over the cases — the
margin of train_tolerances.json and of make_deepfm_train_csr_tolerances.py.  The loss has its own bound (1e-5 + 1e-4 |x|, as
tests/test_gpu_train_edges.py) and no k.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_ref as R  # noqa: E402
import din_train_csr_ref as S  # noqa: E402

MARGIN = 8.0
PATH = os.path.join(ROOT, "tests", "golden", "din_train_csr_tolerances.json")
CLASSES = R.TENSORS


def all_cases():
    return S.all_cases()


def measure(w, E, L, seq, umask, row_off, codes, y):
    NI = S.NUM_INDEX
    up = S.row_reference(w, E, L, seq, umask, row_off, codes, y)
    out = {k: 0.0 for k in CLASSES}
    for reverse in (False, True):
        lo = S.step_csr(w, E, L, NI, seq, umask, row_off, codes, y, dtype=np.float32, reverse=reverse)
        ratios, zeros_exact = R.tensor_ratios(lo["g"], up, S.EPS32, E, NI)
        assert zeros_exact
        for k, v in ratios.items():
            out[k] = max(out[k], v)
    return out


def compute():
    cases = {n: measure(*c) for n, c in all_cases().items()}
    k = {t: MARGIN * max(c[t] for c in cases.values()) for t in CLASSES}
    return dict(margin=MARGIN, k=k, cases=cases)


def main():
    out = compute()
    for t in CLASSES:
        print("%-6s k = %9.3f" % (t, out["k"][t]))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
