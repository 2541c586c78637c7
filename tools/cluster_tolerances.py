#!/usr/bin/env python3
"""Writes tests/golden/cluster_tolerances.json: the numerical bounds of tests/test_gpu_cluster.py, derived from the error of a plain
float32 numpy evaluation against fp64 on the tests' own data (never from what the device gives).

  distance  relative error of ||x - c||^2 evaluated in float32, maximum over the rows and over the centroids the numpy restatement
            (tests/cluster_ref.py) finds at every node of its own tree; the device is allowed 4 x that (its summation order differs).
  centroid  absolute error of a float32 column mean over the members of every node of the restatement's tree, plus one float32
            rounding of the largest coordinate (the centroid is handed back as float32: 2^-24 of its magnitude is the format's own
            precision); the device is allowed 4 x the sum.
  centroid_multi_tile, distance_edges  the bounds of tests/test_gpu_cluster_edges.py (G8, G10, G11), the same two rules measured on
            each case's whole data.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_ref as R  # noqa: E402


def node_members(codes):
    out = {}
    for i, c in enumerate(np.asarray(codes).tolist()):
        while c > 0:
            c = (c - 1) // 2
            out.setdefault(c, []).append(i)
    return out


def measure(x, seed):
    codes = R.recursive_cluster(x, restarts=2, seed=seed)
    dist, mean = 0.0, 0.0
    for c, idx in node_members(codes).items():
        if len(idx) < 3:
            continue
        xs = x[np.asarray(idx)]
        c0 = xs.astype(np.float64).mean(axis=0).astype(np.float32)
        dist = max(dist, R.f32_distance_error(xs, c0))
        mean = max(mean, R.f32_mean_error(xs))
    return dist, mean


def main():
    rng_u = lambda n, E, s: np.random.default_rng(s).random((n, E), dtype=np.float32)
    cases = {"planted_1024x16": R.planted(10, 16, 1e-4, 7)[0], "uniform_5000x16": rng_u(5000, 16, 21), "uniform_1000x128": rng_u(1000, 128, 22)}
    out = {"distance": {}, "centroid": {}}
    for name, x in cases.items():
        d, m = measure(x, 1)
        out["distance"][name] = {"measured_rel": d, "bound_rel": 4 * d}
        if name == "planted_1024x16":
            fmt = float(np.abs(x).max()) * 2.0 ** -24
            out["centroid"] = {"measured_f32_mean_abs": m, "f32_rounding_abs": fmt, "bound_abs": 4 * (m + fmt)}
    # tests/test_gpu_cluster_edges.py: the same two rules on each case's whole data (tests/test_cluster_host.py recomputes these)
    out["centroid_multi_tile"], out["distance_edges"] = {}, {}
    for E in (16, 32, 64, 128):
        x = R.g8_data(E)
        m, fmt = R.f32_mean_error(x), float(np.abs(x).max()) * 2.0 ** -24
        out["centroid_multi_tile"]["hierarchy_2500x%d" % E] = {"measured_f32_mean_abs": m, "f32_rounding_abs": fmt, "bound_abs": 4 * (m + fmt)}
    edges = {"uniform_600x%d" % E: rng_u(600, E, 40 + E) for E in (1, 24, 48, 100)}
    edges["hierarchy_2500x16"] = R.g8_data(16)
    for name, x in edges.items():
        d = R.f32_distance_error(x, x.mean(axis=0))
        out["distance_edges"][name] = {"measured_rel": d, "bound_rel": 4 * d}
    with open(os.path.join(ROOT, "tests", "golden", "cluster_tolerances.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
