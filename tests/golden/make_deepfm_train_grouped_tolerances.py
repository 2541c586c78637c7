#!/usr/bin/env python3
"""Writes tests/golden/deepfm_train_grouped_tolerances.json: the constants k of the bound |gpu - ref| <= k[tensor] eps32 A of
tests/test_gpu_deepfm_train_grouped.py (ref, A: the ROW step of tests/deepfm_train_ref.py in float64 on the expanded rows;
eps32 = 2^-24).  Runs on the CPU; never derived from what the device gives.

For every GPU case the grouped restatement (tests/deepfm_train_grouped_ref.py) is run in float32 twice, per-user row sums in order and
reversed, and compared with the float64 row step: ratio = max |f32 - f64| / (eps32 A) per tensor class and for the loss.
k = 8 x the largest ratio over the cases — margin and method of make_deepfm_train_tolerances.py.

The long-segment structure (3 users x 513 identical candidates) has a k of its own, "k_long_segment", measured the same way on that
case alone: a sequential float32 sum of 1 539 nearly identical addends errs systematically (every addition rounds the same way), which
no drawn shape does, and one k for both would loosen the bound of every other case by an order of magnitude.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deepfm_train_ref as T  # noqa: E402
import deepfm_train_grouped_ref as G  # noqa: E402

MARGIN = 8.0
PATH = os.path.join(ROOT, "tests", "golden", "deepfm_train_grouped_tolerances.json")
CLASSES = T.TENSORS + ("loss",)
LONG = "long_segment"


def case_name(shape):
    return "E%d-L%d-U%d-R%d" % shape


def all_cases():
    """name -> (weights, E, L, seq, codes, y)"""
    out = {}
    for shape in G.SHAPES + (G.GRID_CASE,):
        w, s, c, y, _ = G.shape_case(*shape)
        out[case_name(shape)] = (w, shape[0], shape[1], s, c, y)
    for name in G.STRUCTURES:
        w, s, c, y, _ = G.structure_case(name)
        out[name] = (w, 16, 10, s, c, y)
    return out


def measure(w, E, L, seq, codes, y):
    NI = G.NUM_INDEX
    up = G.row_reference(w, E, L, seq, codes, y)
    out = {k: 0.0 for k in CLASSES}
    for reverse in (False, True):
        lo = G.step_grouped(w, E, L, NI, seq, codes, y, dtype=np.float32, reverse=reverse)
        for k, v in T.ratios(lo["g"], up["g"], up["A"], E, L, NI).items():
            out[k] = max(out[k], v)
        out["loss"] = max(out["loss"], abs(lo["loss"] - up["loss"]) / (T.EPS32 * up["A_loss"]))
    return out


def compute():
    cases = {n: measure(*c) for n, c in all_cases().items()}
    k = {t: MARGIN * max(c[t] for n, c in cases.items() if n != LONG) for t in CLASSES}
    # (a single case is one sample of the error: where it happens to land below the drawn cases' worst, their k holds for it too)
    k_long = {t: max(k[t], MARGIN * cases[LONG][t]) for t in CLASSES}
    return dict(margin=MARGIN, k=k, k_long_segment=k_long, cases=cases)


def main():
    out = compute()
    for t in CLASSES:
        print("%-5s k = %9.3f   long segment %9.3f" % (t, out["k"][t], out["k_long_segment"][t]))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
