#!/usr/bin/env python3
"""Deep-Retrieval M-step, the greedy path assignment at the shape of tools/dr_mstep_bench.py (configs/c5_dr_10m.conf's K,
D, L, E, cd.candidate_path_num, penalty; 1 M items, 262 144 Zipf samples, fp32 model), J = 3 paths per item, three iterations.  The CSR
comes from the device route (Engine.dr_mstep_path_scores) in the same run.  Timed on identical inputs:
  * dr_mstep.assign_paths (host) and Engine.dr_mstep_assign_paths (device), over the hit items only (the CSR re-numbered to them) and
    over all items (the host then draws a numpy path per unhit item and iteration, the device one counter-based path per unhit item);
  * one device call under DM_DR_TIME_LAUNCHES=1 for the event times per kind: the chain's, and that time per item visit
    (iterations x hit items);
  * CoordinateDescent.optimize as a whole: dr_mstep.optimize(path_scores="device", assign="device") — one call, nothing but the result
    leaves the device — against path_scores="device" with the host assignment.
1 warm-up and the median wall time of `--steps` calls for the device routes; a host route runs `--host-steps` times.  The hit items' paths
of the two routes are compared and counted, nothing is asserted.

Writes profiles/dr_mstep_assign_bench.json (--out).  Not measured: hardware counters, other shapes / skews / J / C above 64 (the chain's
wider register forms), the streaming mode's fused call, more than one box."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dismember_amd import Engine, conf, dr_mstep  # noqa: E402

KINDS = {"index": 94, "check": 95, "chain": 96, "random_and_decode": 97}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dr_mstep_assign_bench.json"))
    ap.add_argument("--conf", default=os.path.join(ROOT, "configs", "c5_dr_10m.conf"))
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--paths", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=1)
    a = ap.parse_args()
    m = conf.read_conf(a.conf, "model")
    cd = conf.read_conf(a.conf, "cd")
    K, D, L, E, C = int(m["num_node"]), int(m["num_layer"]), int(m["seq_len"]), int(m["embed_size"]), int(cd["candidate_path_num"])
    pf, p = float(cd["penalty_factor"]), int(cd["penalty_poly_order"])
    N, items, J, T = a.samples, a.items, a.paths, a.iterations
    rng = np.random.default_rng(1)
    eng = Engine(0)
    eng.dr_load_model_synthetic(E, L, K, D, items, seed=3, rerank=False, dtype=np.float32)
    seqs = rng.integers(0, items, size=(N, L)).astype(np.int32)
    seqs[rng.random((N, L)) < 0.1] = -1
    rank = rng.zipf(a.zipf, size=4 * N)
    targets = (rank[rank <= items][:N] - 1).astype(np.int32)
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
    off, codes, scores, occ = eng.dr_mstep_path_scores(seqs, targets, C)
    hit = np.flatnonzero(occ > 0)
    usable = bool((np.diff(off)[hit] >= J).all())          # (an item with fewer than J candidates stops both routes)
    off_h = np.zeros(len(hit) + 1, np.int64)
    np.cumsum(np.diff(off)[hit], out=off_h[1:])
    kw = dict(penalty_factor=pf, penalty_poly_order=p, seed=0)
    dev_all, t_dev_all = timed(lambda: eng.dr_mstep_assign_paths(off, codes, scores, occ, K, D, J, T, **kw), 1, a.steps)
    dev_hit, t_dev_hit = timed(lambda: eng.dr_mstep_assign_paths(off_h, codes, scores, occ[hit], K, D, J, T, **kw), 1, a.steps)
    sc = {int(v): (codes[off[v]:off[v + 1]], scores[off[v]:off[v + 1]]) for v in hit}
    oc = dict(zip(hit.tolist(), occ[hit].tolist()))
    host_hit, t_host_hit = timed(lambda: dr_mstep.assign_paths(sc, oc, hit.tolist(), T, J, K, D, **kw), 0, a.host_steps)
    _, t_host_all = timed(lambda: dr_mstep.assign_paths(sc, oc, range(items), T, J, K, D, **kw), 0, a.host_steps)
    okw = dict(num_iteration=T, path_scores="device", **kw)
    _, t_fused = timed(lambda: dr_mstep.optimize(eng, seqs, targets, range(items), C, J, assign="device", as_array=True, **okw), 1, a.steps)
    _, t_mixed = timed(lambda: dr_mstep.optimize(eng, seqs, targets, range(items), C, J, **okw), 0, a.host_steps)
    os.environ["DM_DR_TIME_LAUNCHES"] = "1"
    eng.timing_reset()
    eng.dr_mstep_assign_paths(off, codes, scores, occ, K, D, J, T, **kw)
    os.environ.pop("DM_DR_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}
    eng.close()
    dec = dr_mstep.decode_codes(dev_all[hit], K, D)
    same = sum(1 for i, v in enumerate(hit.tolist()) if [tuple(r) for r in dec[i].tolist()] == host_hit[v])
    same_sub = bool(np.array_equal(dev_all[hit], dev_hit))
    med = lambda t: float(np.median(t))
    visits = T * len(hit)
    out = dict(shape=dict(K=K, D=D, L=L, E=E, C=C, J=J, iterations=T, penalty_factor=pf, penalty_poly_order=p, num_item=items, N=N, zipf=a.zipf,
                          dtype="float32", items_hit=int(len(hit)), entries=int(len(codes)), every_hit_item_has_J_candidates=usable),
               device_all_items_ms_median=med(t_dev_all), device_all_items_ms_all=t_dev_all,
               device_hit_items_ms_median=med(t_dev_hit), device_hit_items_ms_all=t_dev_hit,
               host_hit_items_ms_median=med(t_host_hit), host_hit_items_ms_all=t_host_hit,
               host_all_items_ms_median=med(t_host_all), host_all_items_ms_all=t_host_all,
               host_over_device_hit_items=med(t_host_hit) / med(t_dev_hit), host_over_device_all_items=med(t_host_all) / med(t_dev_all),
               optimize_fused_ms_median=med(t_fused), optimize_fused_ms_all=t_fused,
               optimize_device_scores_host_assignment_ms_median=med(t_mixed), optimize_device_scores_host_assignment_ms_all=t_mixed,
               kernels_ms=kernels, chain=dict(ms=kernels["chain"]["ms"], item_visits=visits, us_per_item_visit=kernels["chain"]["ms"] * 1e3 / max(visits, 1)),
               agreement=dict(hit_items=int(len(hit)), hit_items_with_the_host_routes_paths=same, hit_only_call_equals_the_all_items_call=same_sub),
               warmup=1, steps=a.steps, host_steps=a.host_steps,
               not_measured="hardware counters, other shapes / skews / J, lists longer than 64 (the chain's wider register forms), the streaming mode's "
                            "fused call, a second box; the per-kind times are event pairs of one extra call that drains the device between groups")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("assignment, hit items only: device %.1f ms   host %.1f ms;   all items: device %.1f ms   host %.1f ms" % (
        med(t_dev_hit), med(t_host_hit), med(t_dev_all), med(t_host_all)))
    print("optimize: fused %.1f ms   device path scores + host assignment %.1f ms" % (med(t_fused), med(t_mixed)))
    for name, k in kernels.items():
        print("  %-20s %3d launches %9.3f ms" % (name, k["launches"], k["ms"]))
    print("chain: %d item visits, %.3f us per visit" % (visits, out["chain"]["us_per_item_visit"]))
    print("agreement:", out["agreement"])


if __name__ == "__main__":
    main()
