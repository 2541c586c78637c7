#!/usr/bin/env python3
"""Rerank training step (dm_dr_rerank_forward_backward_dev with device-drawn negatives + dm_dr_rerank_adam_step) at E = 128, L = 10,
B = 16 384 rows, 1 M items, S in {1, 20, 100}, fp64 and fp32, one GPU, accumulating softmax-table gradient (the default).  2 warm-up
steps, then the median wall time of 7 steps (each ends in a stream synchronize), then one more step under DM_DR_TIME_LAUNCHES=1 for the
per-kernel event times (an event pair around each group of launches; host work between the groups is in the step time and in none of
them).  The three new kernels are timed as "sample" (items + sampler), "sampled_softmax" and "softmax_grad" — the last bracket also
holds the pairs kernel and the radix sort its segment sums need.

floor_ms is a count of bytes against the 9.5 TB/s at which this project's gathers saturate: the gathered softmax_w
rows once, the U rows the segment sums read, the sort's passes (8-bit digits over the item bits; per pass and pair 8 bytes counted, 12
read and 12 written) and the two Adam updates over the rows they visit (w, g, s, r read; w, s, r written, g too where it is cleared).
The number of distinct rows is the expectation for uniform ids, not a count.  One process, no retries, its own time limit (--time-limit,
exit status 124).  Writes profiles/dr_rerank_bench.json (--out).  Not profiled: counters, occupancy, measured memory traffic."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine  # noqa: E402

KINDS = {"user_vectors": 60, "sample": 61, "sampled_softmax": 62, "softmax_grad": 63, "dX": 64, "dW_db": 65, "emb_grad": 66, "adam": 67}
NEW = ("sample", "sampled_softmax", "softmax_grad")
GATHER_TBS = 9.5


def floor_ms(es, E, L, B, S, num_item):
    distinct = lambda m: num_item * (1.0 - (1.0 - 1.0 / num_item) ** m)
    m2 = B * (S + 1)
    bits = max(1, int(num_item).bit_length())
    passes = (bits + 7) // 8
    gathered = 2.0 * m2 * E * es                               # softmax_w rows once + the U rows of the segment sums
    sort = passes * m2 * (8 + 12 + 12)
    adam = distinct(m2) * (E + 1) * es * 7 + (distinct(0.9 * B * L) * E + E * L * E + E) * es * 8
    total = gathered + sort + adam
    return dict(bytes_gathered=gathered, bytes_sort=sort, bytes_adam=adam, floor_ms=total / (GATHER_TBS * 1e12) * 1e3)


def run(dtype, L, E, B, S, num_item, warmup, steps):
    rng = np.random.default_rng(1)
    eng = Engine(0)
    eng.dr_load_model_synthetic(E, L, 16, 2, num_item, seed=3, rerank=True, dtype=dtype)
    eng.dr_rerank_train_init(S, seed=5, lr=1e-3)
    seq = rng.integers(0, num_item, size=(B, L)).astype(np.int32)
    seq[rng.random((B, L)) < 0.1] = -1
    tg = rng.integers(0, num_item, size=B).astype(np.int32)
    d_seq, d_tg = eng.dev_alloc(seq.nbytes), eng.dev_alloc(tg.nbytes)
    eng.h2d(d_seq, seq)
    eng.h2d(d_tg, tg)

    def step():
        loss = eng.dr_rerank_forward_backward_dev(d_seq, d_tg, None, B)
        eng.dr_rerank_adam_step(1.0)
        eng.synchronize()
        return loss
    for _ in range(warmup):
        step()
    times, losses = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        losses.append(step())
        times.append((time.perf_counter() - t0) * 1e3)
    os.environ["DM_DR_TIME_LAUNCHES"] = "1"
    eng.timing_reset()
    step()
    os.environ.pop("DM_DR_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}
    eng.dev_free(d_seq)
    eng.dev_free(d_tg)
    eng.close()
    ms = float(np.median(times))
    new_ms = sum(kernels[k]["ms"] for k in NEW)
    out = dict(dtype=np.dtype(dtype).name, S=S, step_ms_median=ms, step_ms_all=times, kernels_ms=kernels,
               kernel_ms_sum=sum(k["ms"] for k in kernels.values()), new_kernels_ms=new_ms, new_kernels_share_of_step=new_ms / ms,
               first_loss=losses[0], last_loss=losses[-1])
    out.update(floor_ms(np.dtype(dtype).itemsize, E, L, B, S, num_item))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dr_rerank_bench.json"))
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--time-limit", type=int, default=300, help="seconds for the whole run")
    a = ap.parse_args()

    def too_long(*_):
        print("dr_rerank_bench: time limit of %d s reached" % a.time_limit, file=sys.stderr)
        os._exit(124)
    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(a.time_limit)
    L, E = 10, 128
    out = dict(shape=dict(L=L, E=E, B=a.rows, num_item=a.items), warmup=a.warmup, steps=a.steps, gather_tb_per_s=GATHER_TBS,
               not_profiled="hardware counters, occupancy, measured memory traffic; the per-kernel times are event pairs of one extra step",
               runs=[run(dt, L, E, a.rows, S, a.items, a.warmup, a.steps) for S in (1, 20, 100) for dt in (np.float64, np.float32)])
    signal.alarm(0)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for r in out["runs"]:
        print("S = %3d %s  %.2f ms/step  new kernels %.2f ms (%.2f of the step)  floor %.3f ms   kernels %s" % (
            r["S"], r["dtype"], r["step_ms_median"], r["new_kernels_ms"], r["new_kernels_share_of_step"], r["floor_ms"],
            "  ".join("%s %.2f" % (k, v["ms"]) for k, v in r["kernels_ms"].items())))


if __name__ == "__main__":
    main()
