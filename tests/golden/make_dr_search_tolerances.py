#!/usr/bin/env python3
"""Writes tests/golden/dr_search_tolerances.json: the relative tolerance of an f32 Deep-Retrieval path probability against the fp64
oracle for the f32 cases of tests/dr_search_cases.py (tests/test_gpu_dr_search_ranges.py).  Runs on the CPU; never derived from what
the device gives.

At the wide cases' logit magnitudes (|logit| reaches about 100) an f32 logit carries an absolute error of 1e-5 .. 1e-4, which the
softmax turns into a relative error of the probability: the 1e-4 of test_gpu_dr.py::test_beam_search_f32 does not transfer.  For every
case the search is restated in numpy float32 (tests/dr_search_cases.py: sequential f32 dots, f32 softmax) and compared with the same
restatement in float64 over every path the fp64 search returns: err = max |p32 - p64| / p64.  rtol = MARGIN x max(err, D 2^-24), two
bits for a device whose summation order (MFMA GEMM, node tables, slice-wise denominators) differs from the sequential one — the margin
tests/test_attention_cases_host.py uses the other way round; D 2^-24, one rounding per layer of the probability product, is the least
the format allows however lucky the restatement's roundings are (the ties cases: 1 / 70 three times).
"same" is the fraction of users whose whole f32 path list equals the fp64 one (tests/test_dr_search_cases_host.py asks >= 0.95 of the
wide cases, the GPU test >= 0.9).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dr_search_cases as R  # noqa: E402

MARGIN = 4.0
PATH = os.path.join(ROOT, "tests", "golden", "dr_search_tolerances.json")


def measure(name):
    c = R.build(name)
    paths, probs, cnt, _ = R.beam64(name)
    p32 = R.beam_search(name, np.float32)[0]
    err = 0.0
    for u in range(c["U"]):
        ref = probs[u, :cnt[u]]
        got = R.path_probs(name, u, paths[u, :cnt[u]], np.float32).astype(np.float64)
        err = max(err, float((np.abs(got - ref) / ref).max()))
    same = float(np.mean([np.array_equal(p32[u], paths[u]) for u in range(c["U"])]))
    return dict(err=err, same=same, rtol=MARGIN * max(err, c["D"] * 2.0 ** -24))


def main():
    out = {"margin": MARGIN, "cases": {n: measure(n) for n in R.CASES if R.CASES[n]["dtype"] == "f32"}}
    for n, v in out["cases"].items():
        print("%-14s err = %.3e  rtol = %.3e  same = %.3f" % (n, v["err"], v["rtol"], v["same"]))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
