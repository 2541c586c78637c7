#!/usr/bin/env python3
"""Writes tests/golden/dr_rerank_tolerances.json: the constants k of the bound |gpu - ref| <= k[tensor] eps_T A of
tests/test_gpu_dr_rerank.py (ref, A: tests/dr_rerank_ref.py; eps_T = 2^-24 for an f32 model, 2^-53 for an f64 one).  Runs on the CPU;
never derived from what the device gives.  The method is tests/golden/make_dr_train_tolerances.py's.

For every case the restatement is run IN THE CASE'S PRECISION T twice, rows in order and rows reversed, and compared with the
restatement one precision up (float64 for T = float32, np.longdouble for T = float64): ratio = max |T - up| / (eps_T A) per tensor
(rerank_emb, rerank_w, rerank_b, softmax_w, softmax_b) and |loss_T - loss_up| / (eps_T A_loss) for the sampled loss; the full-softmax
loss likewise over its own cases.  k = 8 x the largest ratio over the cases of that precision: three bits for a device whose summation
order (MFMA blocks of 4 along k, slabs of the batch, lane groups, sorted segments) differs from both CPU orders and samples the same
error distribution.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dr_rerank_ref as R  # noqa: E402

MARGIN = 8.0
PATH = os.path.join(ROOT, "tests", "golden", "dr_rerank_tolerances.json")
UP = {"f32": np.float64, "f64": np.longdouble}


def measure(name):
    c = R.make_case(name)
    dt = c["dtype"]
    eps = R.EPS[dt]
    args = (c["weights"], c["dims"], c["seq"], c["targets"], c["negatives"])
    up = R.step(*args, dtype=UP[dt])
    out = {k: 0.0 for k in R.TENSORS + ("loss",)}
    for reverse in (False, True):
        lo = R.step(*args, dtype=R.NP[dt], reverse=reverse)
        ratios, zeros_exact = R.ratios(lo["g"], up, eps)
        assert zeros_exact, name
        for k, v in ratios.items():
            out[k] = max(out[k], v)
        out["loss"] = max(out["loss"], float(abs(UP[dt](lo["loss"]) - up["loss"]) / (eps * up["A_loss"])))
    return out


def measure_full(name, dt):
    c = R.make_full_case(name, dt)
    eps = R.EPS[dt]
    up, A = R.full_loss(c["weights"], c["dims"], c["seq"], c["targets"], dtype=UP[dt])
    worst = 0.0
    for reverse in (False, True):
        lo, _ = R.full_loss(c["weights"], c["dims"], c["seq"], c["targets"], dtype=R.NP[dt], reverse=reverse)
        worst = max(worst, float(abs(UP[dt](lo) - up) / (eps * A)))
    return worst


def main():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 on this platform"
    out = {"margin": MARGIN}
    for dt in ("f32", "f64"):
        cases = {n: measure(n) for n in R.CASES if R.CASES[n][-1] == dt}
        full = {n: measure_full(n, dt) for n in R.FULL_CASES}
        k = {t: MARGIN * max(c[t] for c in cases.values()) for t in R.TENSORS + ("loss",)}
        k["full_loss"] = MARGIN * max(full.values())
        out[dt] = dict(k=k, cases=cases, full_loss_cases=full)
        for t, v in k.items():
            print("%s %-10s k = %9.3f" % (dt, t, v))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
