#!/usr/bin/env python3
"""Deep-Retrieval streaming M-step path scores at config 5's shape — the shape, seed and Zipf targets of tools/dr_mstep_bench.py
(configs/c5_dr_10m.conf: K, D, L, E, cd.candidate_path_num and cd.decay_factor; 1 M items, fp32 model): the device call
(Engine.dr_mstep_streaming_path_scores: search, order by item, per-item fold, CSR, download) against the host route
(dr_mstep.streaming_path_scores: the same searches, download of every candidate, one Python merge per sample) on the same engine and the
same inputs.  1 warm-up and the median wall time of `--steps` calls for the device route; the host route takes many seconds, so it runs
`--host-steps` times after the device calls have warmed the engine.  The batch device route (Engine.dr_mstep_path_scores) is timed in the
same run as the yardstick, and a search-only call (Engine.dr_beam_search_dev).  Then one device call under DM_DR_TIME_LAUNCHES=1 for the
event times per kind of launch (an event pair around each group drains the device between groups).

The fold kernel is bounded by its longest chain whatever the width of the machine: an item's merges are sequential.  Reported: the longest
chain (max_occurrence) and the fold's event time divided by it, the time per merge on the critical path.

Writes profiles/dr_mstep_streaming_bench.json (--out).  Not measured: hardware counters, other N / skews / C above 32 (the workgroup form) /
an fp64 model, the greedy assignment that follows (host, unchanged), more than one box."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dismember_amd import Engine, conf, dr_mstep  # noqa: E402

KINDS = {"search_history_gemm": 0, "codes": 89, "order": 90, "fold": 91, "emit": 92}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dr_mstep_streaming_bench.json"))
    ap.add_argument("--conf", default=os.path.join(ROOT, "configs", "c5_dr_10m.conf"))
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=2)
    a = ap.parse_args()
    m = conf.read_conf(a.conf, "model")
    cd = conf.read_conf(a.conf, "cd")
    K, D, L, E, C = int(m["num_node"]), int(m["num_layer"]), int(m["seq_len"]), int(m["embed_size"]), int(cd["candidate_path_num"])
    decay = float(cd["decay_factor"])
    N, items = a.samples, a.items
    rng = np.random.default_rng(1)
    eng = Engine(0)
    eng.dr_load_model_synthetic(E, L, K, D, items, seed=3, rerank=False, dtype=np.float32)
    seqs = rng.integers(0, items, size=(N, L)).astype(np.int32)
    seqs[rng.random((N, L)) < 0.1] = -1
    rank = rng.zipf(a.zipf, size=4 * N)
    targets = (rank[rank <= items][:N] - 1).astype(np.int32)            # item 0 the most popular
    assert len(targets) == N

    def timed(fn, warm, steps):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return r, t
    dev, t_dev = timed(lambda: eng.dr_mstep_streaming_path_scores(seqs, targets, C, decay), 1, a.steps)
    _, t_batch = timed(lambda: eng.dr_mstep_path_scores(seqs, targets, C), 1, a.steps)
    d_seq, d_p, d_pr, d_c = eng.dev_alloc(seqs.nbytes), eng.dev_alloc(N * C * D * 4), eng.dev_alloc(N * C * 8), eng.dev_alloc(N * 4)
    eng.h2d(d_seq, seqs)

    def search_only():
        eng.dr_beam_search_dev(d_seq, N, C, d_p, d_pr, d_c)
        eng.synchronize()
    _, t_search = timed(search_only, 1, a.steps)
    for p in (d_seq, d_p, d_pr, d_c):
        eng.dev_free(p)
    host, t_host = timed(lambda: dr_mstep.streaming_path_scores(eng, seqs, targets, C, decay), 0, a.host_steps)
    os.environ["DM_DR_TIME_LAUNCHES"] = "1"
    eng.timing_reset()
    eng.dr_mstep_streaming_path_scores(seqs, targets, C, decay)
    os.environ.pop("DM_DR_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}
    layers = [eng.timing_get_kind(kind) for kind in range(10, 30)]             # the sliced search's launches, every layer (EV_DR_*)
    kernels["search_layers"] = dict(launches=sum(n for n, _ in layers), ms=sum(ms for _, ms in layers))
    eng.close()
    # the two routes on the same inputs.  N > 65 536: the host route searches in chunks of 65 536 and the device route in its own, so a
    # beam may differ where the search's pipelines differ; what agrees is counted, nothing is asserted
    off, codes, scores, occ = dev
    same_items = sorted(host) == np.flatnonzero(occ).tolist()
    same_codes = sum(1 for v, (c, _) in host.items() if c.tolist() == codes[off[v]:off[v + 1]].tolist())
    same_scores = sum(1 for v, (c, s) in host.items() if c.tolist() == codes[off[v]:off[v + 1]].tolist() and s.tobytes() == scores[off[v]:off[v + 1]].tobytes())
    dev_ms, host_ms, search_ms, batch_ms = (float(np.median(t)) for t in (t_dev, t_host, t_search, t_batch))
    longest = int(occ.max())
    out = dict(shape=dict(K=K, D=D, L=L, E=E, C=C, decay_factor=decay, num_item=items, N=N, zipf=a.zipf, dtype="float32", slots=N * C,
                          items_hit=int((occ > 0).sum()), max_occurrence=longest, entries=int(len(codes))),
               device_ms_median=dev_ms, device_ms_all=t_dev, host_ms_median=host_ms, host_ms_all=t_host, host_over_device=host_ms / dev_ms,
               batch_device_ms_median=batch_ms, batch_device_ms_all=t_batch, search_only_ms_median=search_ms, search_only_ms_all=t_search,
               fold_and_order_ms=dev_ms - search_ms,
               kernels_ms=kernels, kernel_ms_sum=sum(k["ms"] for k in kernels.values()),
               fold=dict(ms=kernels["fold"]["ms"], longest_chain=longest, us_per_merge_on_the_critical_path=kernels["fold"]["ms"] * 1e3 / max(longest, 1)),
               agreement=dict(same_items=bool(same_items), items_with_the_same_codes=same_codes, items_with_the_same_codes_and_score_bytes=same_scores, items=len(host)),
               warmup=1, steps=a.steps, host_steps=a.host_steps,
               not_measured="hardware counters, other N / skews, C above 32 (the workgroup form of the fold), an fp64 model, the greedy assignment (host, "
                            "unchanged), a second box; the per-kind times are event pairs of one extra call that drains the device between groups")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("streaming device %.1f ms (search alone %.1f ms; batch device route %.1f ms)   host %.1f ms   host / device %.1f" % (
        dev_ms, search_ms, batch_ms, host_ms, host_ms / dev_ms))
    for name, k in kernels.items():
        print("  %-20s %3d launches %9.3f ms" % (name, k["launches"], k["ms"]))
    print("fold: longest chain %d, %.3f us per merge on the critical path" % (longest, out["fold"]["us_per_merge_on_the_critical_path"]))
    print("agreement:", out["agreement"])


if __name__ == "__main__":
    main()
