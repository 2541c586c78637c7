#!/usr/bin/env python3
"""Deep-Retrieval M-step path scores at config 5's shape (configs/c5_dr_10m.conf: K, D, L, E and cd.candidate_path_num; 1 M items, fp32
model, Zipf-distributed targets): the device call (Engine.dr_mstep_path_scores: search, aggregation, cut at C, download of the CSR) against
the host route (dr_mstep.batch_path_scores: the same searches, download of every candidate, lexsort, reduceat, a Python loop over the items)
on the same engine and the same inputs, at an N both can hold.  1 warm-up and the median wall time of `--steps` calls for the device route;
the host route takes seconds, so it gets 1 warm-up (the engine's buffers) and the median of `--host-steps`.  Then one device call under
DM_DR_TIME_LAUNCHES=1 for the event times per kind of launch (an event pair around each group drains the device between groups, so that call
is slower than the timed ones and its sum is not their time).

Floor: bytes by count for the aggregation alone (the search is timed by tools/dr_bench.py): every pair written once (key 8 + value 4), the
first sort's passes (12 read twice — histogram and scatter — and written once per 8-bit pass), the probabilities gathered once (8 + the 4-byte
value), at 6.3 TB/s, the streaming rate an MI355X's HBM reaches (8 TB/s on paper).  The call's aggregation time is its wall time minus a
search-only call (Engine.dr_beam_search_dev on the same samples), and the multiple of the floor is stated for that.

Writes profiles/dr_mstep_bench.json (--out).  Not measured: hardware counters, achieved bandwidth per kernel, other N or skews, fp64 models,
the greedy assignment that follows (host, unchanged), more than one box."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dismember_amd import Engine, conf, dr_mstep  # noqa: E402

KINDS = {"search_history_gemm": 0, "pairs": 80, "pair_sort": 81, "segment_heads": 82, "segment_sums": 83, "score_sort": 84, "item_sort": 85, "cut": 86,
         "emit_offsets": 87, "occurrence": 88}
HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dr_mstep_bench.json"))
    ap.add_argument("--conf", default=os.path.join(ROOT, "configs", "c5_dr_10m.conf"))
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    a = ap.parse_args()
    m = conf.read_conf(a.conf, "model")
    cd = conf.read_conf(a.conf, "cd")
    K, D, L, E, C = int(m["num_node"]), int(m["num_layer"]), int(m["seq_len"]), int(m["embed_size"]), int(cd["candidate_path_num"])
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
    dev, t_dev = timed(lambda: eng.dr_mstep_path_scores(seqs, targets, C), 1, a.steps)
    d_seq, d_p, d_pr, d_c = eng.dev_alloc(seqs.nbytes), eng.dev_alloc(N * C * D * 4), eng.dev_alloc(N * C * 8), eng.dev_alloc(N * 4)
    eng.h2d(d_seq, seqs)

    def search_only():
        eng.dr_beam_search_dev(d_seq, N, C, d_p, d_pr, d_c)
        eng.synchronize()
    _, t_search = timed(search_only, 1, a.steps)
    for p in (d_seq, d_p, d_pr, d_c):
        eng.dev_free(p)
    host, t_host = timed(lambda: dr_mstep.batch_path_scores(eng, seqs, targets, C), 1, a.host_steps)
    os.environ["DM_DR_TIME_LAUNCHES"] = "1"
    eng.timing_reset()
    eng.dr_mstep_path_scores(seqs, targets, C)
    os.environ.pop("DM_DR_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}
    layers = [eng.timing_get_kind(kind) for kind in range(10, 30)]             # the sliced search's launches, every layer (EV_DR_*)
    kernels["search_layers"] = dict(launches=sum(n for n, _ in layers), ms=sum(ms for _, ms in layers))
    eng.close()
    # the two routes on the same inputs: the same items, the same paths in the same order wherever the host's sums leave the order alone
    off, codes, scores, occ = dev
    same_items = sorted(host) == np.flatnonzero(np.diff(off)).tolist()
    same_codes = sum(1 for v, (c, _) in host.items() if c.tolist() == codes[off[v]:off[v + 1]].tolist())
    max_rel = max((float(np.max(np.abs(s - scores[off[v]:off[v + 1]]) / s)) for v, (c, s) in host.items()
                   if c.tolist() == codes[off[v]:off[v + 1]].tolist()), default=0.0)
    pairs = N * C
    ibits, cbits = int(items).bit_length(), (K ** D - 1).bit_length()
    passes = (ibits + cbits + 7) // 8
    floor_bytes = pairs * 12 + passes * pairs * 36 + pairs * 12
    floor_ms = floor_bytes / (HBM_TBPS * 1e12) * 1e3
    dev_ms, host_ms, search_ms = float(np.median(t_dev)), float(np.median(t_host)), float(np.median(t_search))
    out = dict(shape=dict(K=K, D=D, L=L, E=E, C=C, num_item=items, N=N, zipf=a.zipf, dtype="float32", pairs=pairs,
                          items_hit=int((occ > 0).sum()), max_occurrence=int(occ.max()), entries=int(len(codes))),
               device_ms_median=dev_ms, device_ms_all=t_dev, host_ms_median=host_ms, host_ms_all=t_host, host_over_device=host_ms / dev_ms,
               search_only_ms_median=search_ms, search_only_ms_all=t_search, aggregation_ms=dev_ms - search_ms,
               floor=dict(bytes=floor_bytes, sort_passes=passes, hbm_tbps=HBM_TBPS, ms=floor_ms, aggregation_over_floor=(dev_ms - search_ms) / floor_ms),
               kernels_ms=kernels, kernel_ms_sum=sum(k["ms"] for k in kernels.values()),
               agreement=dict(same_items=bool(same_items), items_with_the_same_codes=same_codes, items=len(host), max_rel_score_diff_there=max_rel),
               warmup=1, steps=a.steps, host_steps=a.host_steps,
               not_measured="hardware counters, achieved bandwidth per kernel, other N / skews / an fp64 model, the greedy assignment (host, unchanged), "
                            "a second box; the per-kind times are event pairs of one extra call that drains the device between groups")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("device %.1f ms (search alone %.1f ms, aggregation %.1f ms = %.1f x the byte floor %.2f ms)   host %.1f ms   host / device %.1f" % (
        dev_ms, search_ms, dev_ms - search_ms, (dev_ms - search_ms) / floor_ms, floor_ms, host_ms, host_ms / dev_ms))
    for name, k in kernels.items():
        print("  %-20s %3d launches %9.3f ms" % (name, k["launches"], k["ms"]))
    print("agreement:", out["agreement"])


if __name__ == "__main__":
    main()
