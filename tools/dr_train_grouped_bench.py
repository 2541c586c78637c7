#!/usr/bin/env python3
"""The sample-grouped Deep-Retrieval training step (dm_dr_train_forward_backward_grouped_dev) against the row step
(dm_dr_train_forward_backward_dev) on the SAME expanded batch in the same run, at config 5's shape: K = 1000, D = 3, L = 10, E = 128,
1 M items, R = S J rows of 16 384 (S = 16 384 // J) for J = 1, 2, 3, fp64 and fp32, one GPU.  Per (dtype, J) and per step kind:
2 warm-up steps, then the median wall time of 7 steps (forward/backward + dm_dr_adam_step, each ends in a stream synchronize), then one
more step under DM_DR_TIME_LAUNCHES=1 for the per-kind event times.  By flop count the grouped step keeps (30 / J + 3) / 33 of the row
step's products (30 of 33 column blocks are history columns, computed once per sample instead of once per row): printed beside each
measured ratio.  Writes profiles/dr_train_grouped_bench.json (--out).  Not profiled: counters, occupancy, memory traffic."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine  # noqa: E402

KINDS = {"forward": 50, "softmax_ce": 51, "dX": 52, "dW_db": 53, "emb_grad": 54, "adam": 55}


def measure(eng, fb, warmup, steps):
    def step():
        loss = fb()
        eng.dr_adam_step(1.0)
        eng.synchronize()
        return loss
    for _ in range(warmup):
        step()
    times, losses = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        losses.append(step().tolist())
        times.append((time.perf_counter() - t0) * 1e3)
    os.environ["DM_DR_TIME_LAUNCHES"] = "1"
    try:
        eng.timing_reset()
        step()
    finally:
        os.environ.pop("DM_DR_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}
    return dict(step_ms_median=float(np.median(times)), step_ms_all=times, kernels_ms=kernels, kernel_ms_sum=sum(k["ms"] for k in kernels.values()),
                first_loss=losses[0], last_loss=losses[-1])


def run(dtype, K, D, L, E, rows, J, num_item, warmup, steps):
    rng = np.random.default_rng(1)
    S = rows // J
    seq = rng.integers(0, num_item, size=(S, L)).astype(np.int32)
    seq[rng.random((S, L)) < 0.1] = -1
    paths = rng.integers(0, K, size=(S, J, D)).astype(np.int32)
    row_seq = np.repeat(seq, J, axis=0)                      # the expanded batch: what transformLayerData hands the row step
    out = dict(dtype=np.dtype(dtype).name, J=J, S=S, R=S * J, flop_expectation=(3.0 * L / J + D) / (3.0 * L + D))
    for kind in ("row", "grouped"):                          # a fresh model each: both start from the same weights
        eng = Engine(0)
        eng.dr_load_model_synthetic(E, L, K, D, num_item, seed=3, rerank=False, dtype=dtype)
        eng.dr_train_init(lr=1e-3)
        a, b = (row_seq, paths.reshape(S * J, D)) if kind == "row" else (seq, paths)
        d_seq, d_paths = eng.dev_alloc(a.nbytes), eng.dev_alloc(b.nbytes)
        eng.h2d(d_seq, a)
        eng.h2d(d_paths, b)
        fb = (lambda: eng.dr_train_forward_backward_dev(d_seq, d_paths, S * J)) if kind == "row" else \
             (lambda: eng.dr_train_forward_backward_grouped_dev(d_seq, d_paths, S, J))
        out[kind] = measure(eng, fb, warmup, steps)
        eng.dev_free(d_seq)
        eng.dev_free(d_paths)
        eng.close()
    out["ratio_grouped_over_row"] = out["grouped"]["step_ms_median"] / out["row"]["step_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dr_train_grouped_bench.json"))
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    K, D, L, E = 1000, 3, 10, 128
    out = dict(shape=dict(K=K, D=D, L=L, E=E, rows=a.rows, num_item=a.items), warmup=a.warmup, steps=a.steps,
               not_profiled="hardware counters, occupancy, memory traffic; the per-kind times are event pairs of one extra step",
               runs=[run(dt, K, D, L, E, a.rows, J, a.items, a.warmup, a.steps) for dt in (np.float64, np.float32) for J in (1, 2, 3)])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for r in out["runs"]:
        print("%s J=%d S=%d  row %.2f ms  grouped %.2f ms  ratio %.3f (flop count %.3f)   grouped kinds %s" % (
            r["dtype"], r["J"], r["S"], r["row"]["step_ms_median"], r["grouped"]["step_ms_median"], r["ratio_grouped_over_row"], r["flop_expectation"],
            "  ".join("%s %.2f" % (k, v["ms"]) for k, v in r["grouped"]["kernels_ms"].items())))


if __name__ == "__main__":
    main()
