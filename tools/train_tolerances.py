#!/usr/bin/env python3
"""Writes tests/golden/train_tolerances.json: the per-tensor constants k_T of the gradient bound |g - ref| <= k_T eps A of
tests/test_gpu_train_edges.py (ref, A: tests/train_ref.py; eps = 2^-24 for an f32 model, 2^-53 for an f64 one).  Runs on the CPU.

For every batch of every case the C oracle's backward in the case's arithmetic (oracle/din_body.inc: sequential sums, two-pass
softmax) is compared with the fp64 numpy restatement, per tensor: ratio = max |oracle - ref| / (eps A).  k_T = 8 x the largest ratio
over the cases of that arithmetic: three bits for an evaluation that sums the same terms in another order (MFMA accumulation, 16-row
trees, atomics, online softmax).  Never derived from what the device gives.

"tightening" is how many times smaller than the suite's older whole-vector floor (2e-5, fp64: 1e-10, of the gradient's largest
element) the largest bound of a tensor is, at the case where it is least so.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_ref as R  # noqa: E402

MARGIN = 8.0
OLD_FLOOR = {"f32": 2e-5, "f64": 1e-10}
PATH = os.path.join(ROOT, "tests", "golden", "train_tolerances.json")


def oracle_grads(po, c, b):
    pad = b["pad"] if b["pad"] is not None else np.zeros(0, np.int32)
    return po.Din(c["w"].copy(), c["E"], c["L"], c["NI"]).train_grads(b["codes"], b["seqs"], pad, b["y"])


def measure(po, name):
    """-> {batch key: dict(ratios per tensor, scale per tensor = max A / the gradient's largest element, loss_err)}"""
    c = R.make_case(name)
    out = {}
    for i, b in enumerate(c["batches"]):
        ref = R.reference(name, i)
        oloss, og = oracle_grads(po, c, b)
        ratios, zeros_exact = R.tensor_ratios(og, ref, R.EPS[c["dtype"]], c["E"], c["NI"])
        assert zeros_exact, name
        scale, gmax = R.element_scale(ref["A"], c["E"], c["NI"]), float(np.abs(ref["g"]).max())
        rel = {t: float(scale[a:e].max()) / gmax for t, (a, e) in R.sections(c["E"], c["NI"]).items()}
        out[name if len(c["batches"]) == 1 else "%s/%d" % (name, i)] = dict(ratio=ratios, max_A_over_gmax=rel, loss_err=abs(oloss - ref["loss"]))
    return out


def compute(po, names=None):
    out = {"margin": MARGIN}
    for dt in ("f32", "f64"):
        cases = {}
        for name in (names or R.CASES):
            if R.CASES[name]["dtype"] == dt:
                cases.update(measure(po, name))
        k = {t: MARGIN * max(c["ratio"][t] for c in cases.values()) for t in R.TENSORS}
        tight = {t: min(OLD_FLOOR[dt] / (k[t] * R.EPS[dt] * c["max_A_over_gmax"][t]) for c in cases.values()) for t in R.TENSORS}
        out[dt] = dict(k=k, tightening=tight, cases={n: c["ratio"] for n, c in cases.items()})
    return out


def main():
    from oracle import pyoracle as po
    po.build()
    out = compute(po)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for dt in ("f32", "f64"):
        for t in R.TENSORS:
            print("%s %-6s k_T = %9.3f   bound / old floor = 1 / %.1f" % (dt, t, out[dt]["k"][t], out[dt]["tightening"][t]))


if __name__ == "__main__":
    main()
