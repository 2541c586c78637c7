#!/usr/bin/env python3
"""Deep-Retrieval training step (dm_dr_train_forward_backward_dev + dm_dr_adam_step) at config 5's shape: K = 1000, D = 3, L = 10, E = 128,
B = 16 384 rows, 1 M items, fp64 and fp32, one GPU.  2 warm-up steps, then the median wall time of 7 steps (each ends in a stream
synchronize), then one more step under DM_DR_TIME_LAUNCHES=1 for the per-kernel event times (an event pair around each group of
launches; host work between the groups is in the step time and in none of them).  A step is 6 B K (L + (L+1) + (L+2)) E flop by count
(forward plus the two backward products): the achieved fraction is against the 78.6 TFLOP/s this project has measured for the fp64
matrix pipe, for both runs — the rate of the fp32 16x16x4 instruction has not been measured here, so the fp32 fraction is a
comparison with the fp64 figure and nothing more.  Writes profiles/dr_train_bench.json (--out).  Not profiled: counters, occupancy,
memory traffic."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine  # noqa: E402

KINDS = {"forward": 50, "softmax_ce": 51, "dX": 52, "dW_db": 53, "emb_grad": 54, "adam": 55}
PEAK_TFLOPS = 78.6


def run(dtype, K, D, L, E, B, num_item, warmup, steps):
    rng = np.random.default_rng(1)
    eng = Engine(0)
    eng.dr_load_model_synthetic(E, L, K, D, num_item, seed=3, rerank=False, dtype=dtype)
    eng.dr_train_init(lr=1e-3)
    seq = rng.integers(0, num_item, size=(B, L)).astype(np.int32)
    seq[rng.random((B, L)) < 0.1] = -1
    paths = rng.integers(0, K, size=(B, D)).astype(np.int32)
    d_seq, d_paths = eng.dev_alloc(seq.nbytes), eng.dev_alloc(paths.nbytes)
    eng.h2d(d_seq, seq)
    eng.h2d(d_paths, paths)

    def step():
        loss = eng.dr_train_forward_backward_dev(d_seq, d_paths, B)
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
    eng.timing_reset()
    step()
    os.environ.pop("DM_DR_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}
    eng.dev_free(d_seq)
    eng.dev_free(d_paths)
    eng.close()
    flop = 6.0 * B * K * sum(L + d for d in range(D)) * E
    ms = float(np.median(times))
    return dict(dtype=np.dtype(dtype).name, step_ms_median=ms, step_ms_all=times, flop=flop, tflops=flop / ms * 1e-9,
                fraction_of_fp64_matrix_peak=flop / ms * 1e-9 / PEAK_TFLOPS, floor_ms=flop / PEAK_TFLOPS * 1e-9,
                kernels_ms=kernels, kernel_ms_sum=sum(k["ms"] for k in kernels.values()), first_loss=losses[0], last_loss=losses[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dr_train_bench.json"))
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    K, D, L, E = 1000, 3, 10, 128
    out = dict(shape=dict(K=K, D=D, L=L, E=E, B=a.rows, num_item=a.items), warmup=a.warmup, steps=a.steps, peak_tflops=PEAK_TFLOPS,
               not_profiled="hardware counters, occupancy, memory traffic; the per-kernel times are event pairs of one extra step",
               runs=[run(dt, K, D, L, E, a.rows, a.items, a.warmup, a.steps) for dt in (np.float64, np.float32)])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for r in out["runs"]:
        print("%s  %.2f ms/step  %.1f TFLOP/s  %.3f of the fp64 matrix peak   kernels %s" % (
            r["dtype"], r["step_ms_median"], r["tflops"], r["fraction_of_fp64_matrix_peak"],
            "  ".join("%s %.2f" % (k, v["ms"]) for k, v in r["kernels_ms"].items())))


if __name__ == "__main__":
    main()
