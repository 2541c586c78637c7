#!/usr/bin/env python3
"""The resident Deep-Retrieval mapping and training set against the existing host paths in the same run, one GPU.

(a) the path -> items CSR of an item -> paths table, J = 2, K = 1000, D = 3, at --items (1 M; add 10 000 000 if there is time):
    host = synth.dr_path_items_fast (numpy) + Engine.dr_load_path_items (the host sort inside the library), against
    device = Engine.dr_set_item_paths (upload + device build).  Wall time of each, best of --reps; the CSRs are compared.
(b) the training step at §10's shape (K = 1000, D = 3, L = 10, E = 128, 1 M items, 8 192 targets x J = 2 -> 16 384 rows, fp64, rerank
    on with 20 negatives): DRTrainer.step on host batches (fancy-indexed on the host, uploaded for the layer step and again for the
    rerank step) against DRTrainer.step_range on the resident set.  The two alternate for three rounds: 2 warm-up steps, then the median
    of 7, each step ending in a synchronize.
Writes profiles/dr_resident_bench.json (--out).  Not measured: the M-step over the resident set against dm_dr_mstep_optimize, the
conf tasks end to end, the data-parallel step, hardware counters."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine, synth  # noqa: E402
from dismember_amd.dr_train import DRTrainer  # noqa: E402


def bench_mapping(num_item, J, K, D, reps):
    rng = np.random.default_rng(5)
    paths = rng.integers(0, K, size=(num_item, J, D), dtype=np.int32)
    eng = Engine(0)
    eng.dr_load_model_synthetic(16, 4, K, D, num_item, seed=1, rerank=False, dtype=np.float32)
    host, host_invert, dev = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        csr = synth.dr_path_items_fast(paths, K)
        t1 = time.perf_counter()
        eng.dr_load_path_items(*csr)
        eng.synchronize()
        t2 = time.perf_counter()
        host_invert.append((t1 - t0) * 1e3); host.append((t2 - t0) * 1e3)
        want = eng.dr_path_items_download()
        t0 = time.perf_counter()
        eng.dr_set_item_paths(paths)
        eng.synchronize()
        dev.append((time.perf_counter() - t0) * 1e3)
        got = eng.dr_path_items_download()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    eng.close()
    return dict(num_item=num_item, J=J, K=K, D=D, n_paths=int(len(got[0])), host_ms_best=min(host), host_numpy_ms_best=min(host_invert), device_ms_best=min(dev),
                host_ms_all=host, device_ms_all=dev, ratio_device_over_host=min(dev) / min(host))


def bench_step(num_item, targets_per_batch, J, K, D, L, E, rounds, warmup, steps, num_sampled):
    rng = np.random.default_rng(7)
    n_set = targets_per_batch * (warmup + steps)
    seqs = rng.integers(0, num_item, size=(n_set, L)).astype(np.int32)
    seqs[rng.random((n_set, L)) < 0.1] = -1
    targets = rng.integers(0, num_item, n_set).astype(np.int32)
    item_paths = rng.integers(0, K, size=(num_item, J, D), dtype=np.int32)
    trainers = {}
    for kind in ("host", "resident"):                        # a model each, both from the same weights
        eng = Engine(0)
        eng.dr_load_model_synthetic(E, L, K, D, num_item, seed=3, rerank=True, dtype=np.float64)
        trainers[kind] = DRTrainer(eng, item_paths, lr=1e-3, rerank=True, num_sampled=num_sampled, seed=1, resident=kind == "resident")
    trainers["resident"].load_set(seqs, targets)
    trainers["resident"].shuffle(9)
    order = trainers["resident"].engine.dr_train_set_order()
    out = dict(rounds=[])
    T = targets_per_batch
    for _ in range(rounds):
        r = {}
        for kind in ("host", "resident"):
            tr = trainers[kind]
            times = []
            for k in range(warmup + steps):
                t0 = time.perf_counter()
                if kind == "host":
                    idx = order[k * T:(k + 1) * T]
                    tr.step(seqs[idx], targets[idx])
                else:
                    tr.step_range(k * T, T)
                tr.engine.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            r[kind] = dict(step_ms_median=float(np.median(times[warmup:])), step_ms_all=times)
        r["ratio_resident_over_host"] = r["resident"]["step_ms_median"] / r["host"]["step_ms_median"]
        out["rounds"].append(r)
    same = trainers["host"].engine.dr_train_download("weights").tobytes() == trainers["resident"].engine.dr_train_download("weights").tobytes()
    for tr in trainers.values():
        tr.engine.close()
    out.update(weights_identical_after_all_rounds=bool(same), resident_faster_in_every_round=all(r["ratio_resident_over_host"] < 1 for r in out["rounds"]),
               shape=dict(K=K, D=D, L=L, E=E, J=J, num_item=num_item, targets_per_batch=T, rows=T * J, dtype="float64", num_sampled=num_sampled))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dr_resident_bench.json"))
    ap.add_argument("--items", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-items", type=int, default=1_000_000)
    ap.add_argument("--targets", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    out = dict(mapping=[bench_mapping(n, 2, 1000, 3, a.reps) for n in a.items],
               step=bench_step(a.step_items, a.targets, 2, 1000, 3, 10, 128, a.rounds, a.warmup, a.steps, 20),
               not_measured="the M-step over the resident set against dm_dr_mstep_optimize; the conf tasks end to end; the data-parallel step; hardware counters")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for m in out["mapping"]:
        print("mapping %d items: host %.1f ms (numpy %.1f)  device %.1f ms  ratio %.3f" % (m["num_item"], m["host_ms_best"], m["host_numpy_ms_best"],
                                                                                           m["device_ms_best"], m["ratio_device_over_host"]))
    for i, r in enumerate(out["step"]["rounds"]):
        print("step round %d: host %.2f ms  resident %.2f ms  ratio %.3f" % (i, r["host"]["step_ms_median"], r["resident"]["step_ms_median"], r["ratio_resident_over_host"]))
    print("weights identical: %s" % out["step"]["weights_identical_after_all_rounds"])


if __name__ == "__main__":
    main()
