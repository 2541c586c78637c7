#!/usr/bin/env python3
"""Writes tests/golden/dr_train_grouped_tolerances.json: the constants k of the bound |gpu - ref| <= k[tensor] eps_T A of
tests/test_gpu_dr_train_grouped.py (ref, A: tests/dr_train_ref.py's row step on the EXPANDED batch; eps_T = 2^-24 for an f32 model,
2^-53 for an f64 one).  Runs on the CPU; never derived from what the device gives.  The twin of make_dr_train_tolerances.py.

For every case the grouped restatement (tests/dr_train_grouped_ref.py) is run IN THE CASE'S PRECISION T twice, samples and paths in
order and both reversed, and compared with the row restatement on the expanded batch one precision up (float64 for T = float32,
np.longdouble for T = float64): ratio = max |T - up| / (eps_T A) per tensor class (emb, W, b) and |loss_T - loss_up| / (eps_T A_loss)
for the loss, A and A_loss from that row restatement.  k = 8 x the largest ratio over the cases of that precision: three bits for a
device whose summation order (MFMA blocks of 4 along k, slabs of the batch, sorted segments) is a third order over the same error
distribution — the margin tests/golden/dr_train_tolerances.json already uses.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dr_train_grouped_ref as G  # noqa: E402
import dr_train_ref as R  # noqa: E402

MARGIN = 8.0
PATH = os.path.join(ROOT, "tests", "golden", "dr_train_grouped_tolerances.json")
UP = {"f32": np.float64, "f64": np.longdouble}


def measure(name):
    c = G.make_case(name)
    dt = c["dtype"]
    eps = R.EPS[dt]
    up = R.step(c["w"], c["dims"], *G.expand(c["seq"], c["paths"]), dtype=UP[dt])
    out = {k: 0.0 for k in R.CLASSES + ("loss",)}
    for reverse in (False, True):
        lo = G.step(c["w"], c["dims"], c["seq"], c["paths"], dtype=R.NP[dt], reverse_samples=reverse, reverse_paths=reverse)
        ratios, zeros_exact = R.class_ratios(lo["g"], up, eps, c["dims"])
        assert zeros_exact, name
        for k, v in ratios.items():
            out[k] = max(out[k], v)
        out["loss"] = max(out["loss"], G.loss_ratio(lo["loss"], up, eps))
    return out


def main():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 on this platform"
    out = {"margin": MARGIN}
    for dt in ("f32", "f64"):
        cases = {n: measure(n) for n in G.CASES if G.CASES[n][-1] == dt}
        k = {t: MARGIN * max(c[t] for c in cases.values()) for t in R.CLASSES + ("loss",)}
        out[dt] = dict(k=k, cases=cases)
        for t, v in k.items():
            print("%s %-5s k = %9.3f" % (dt, t, v))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
