#!/usr/bin/env python3
"""Writes tests/golden/deepfm_train_csr_tolerances.json: the constants k of the bound |gpu - ref| <= k[tensor] eps32 A of
tests/test_gpu_deepfm_train_csr.py (ref, A: the ROW step of tests/deepfm_train_ref.py in float64 on the expanded rows;
eps32 = 2^-24).  Runs on the CPU; never derived from what the device gives.

For every GPU case the ragged restatement (tests/deepfm_train_csr_ref.py) is run in float32 twice, every user's row sums in order and
reversed, and compared with the float64 row step: ratio = max |f32 - f64| / (eps32 A) per tensor class and for the loss.
k = 8 x the largest ratio over the cases — margin and method of make_deepfm_train_grouped_tolerances.py.  No case here sums a long run
of identical addends (the long-segment structure of the rectangular step's tests is not a ragged structure), so there is one k.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deepfm_train_ref as T  # noqa: E402
import deepfm_train_csr_ref as S  # noqa: E402

MARGIN = 8.0
PATH = os.path.join(ROOT, "tests", "golden", "deepfm_train_csr_tolerances.json")
CLASSES = T.TENSORS + ("loss",)


def all_cases():
    return S.all_cases()


def measure(w, E, L, seq, row_off, codes, y):
    NI = S.NUM_INDEX
    up = S.row_reference(w, E, L, seq, row_off, codes, y)
    out = {k: 0.0 for k in CLASSES}
    for reverse in (False, True):
        lo = S.step_csr(w, E, L, NI, seq, row_off, codes, y, dtype=np.float32, reverse=reverse)
        for k, v in T.ratios(lo["g"], up["g"], up["A"], E, L, NI).items():
            out[k] = max(out[k], v)
        out["loss"] = max(out["loss"], abs(lo["loss"] - up["loss"]) / (T.EPS32 * up["A_loss"]))
    return out


def compute():
    cases = {n: measure(*c) for n, c in all_cases().items()}
    k = {t: MARGIN * max(c[t] for c in cases.values()) for t in CLASSES}
    return dict(margin=MARGIN, k=k, cases=cases)


def main():
    out = compute()
    for t in CLASSES:
        print("%-5s k = %9.3f" % (t, out["k"][t]))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
