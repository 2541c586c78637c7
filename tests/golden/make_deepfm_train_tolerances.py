#!/usr/bin/env python3
"""Writes tests/golden/deepfm_train_tolerances.json: the constants k of the bound |gpu - ref| <= k[tensor] eps32 A of
tests/test_gpu_deepfm_train.py (ref, A: tests/deepfm_train_ref.py in float64; eps32 = 2^-24).  Runs on the CPU; never derived from
what the device gives.

For every GPU case the restatement is run in float32 twice, rows in order and rows reversed, and compared with the float64 one:
ratio = max |f32 - f64| / (eps32 A) per tensor class (emb, l1.W, l1.b, l2.W, l2.b) and |loss32 - loss64| / (eps32 A_loss) for the loss.
k = 8 x the largest ratio over the cases: three bits for a device whose summation order (MFMA blocks of 4 along k, slabs of the batch,
sorted segments, workgroup partials) differs from both CPU orders and samples the same error distribution — the margin
tests/golden/train_tolerances.json and dr_train_tolerances.json already use.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deepfm_train_ref as T  # noqa: E402

MARGIN = 8.0
PATH = os.path.join(ROOT, "tests", "golden", "deepfm_train_tolerances.json")
CLASSES = T.TENSORS + ("loss",)


def all_cases():
    """name -> (weights, E, L, codes, seqs, y)"""
    out = {}
    for E, L, B in T.SHAPES + (T.GRID_CASE,):
        w, c, s, y, _ = T.shape_case(E, L, B)
        out["E%d-L%d-B%d" % (E, L, B)] = (w, E, L, c, s, y)
    for name in T.STRUCTURES:
        w, c, s, y, _ = T.structure_case(name)
        out[name] = (w, 16, 10, c, s, y)
    return out


def measure(w, E, L, codes, seqs, y):
    NI = T.NUM_INDEX
    up = T.step(w, E, L, NI, codes, seqs, y)
    out = {k: 0.0 for k in CLASSES}
    for reverse in (False, True):
        lo = T.step(w, E, L, NI, codes, seqs, y, dtype=np.float32, reverse=reverse)
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
    for t, v in out["k"].items():
        print("%-5s k = %9.3f" % (t, v))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
