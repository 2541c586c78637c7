"""JTM.optimize with the DeepFM scorer at catalogue scale, and the same call with a DIN model on the same tree and catalogue.

  python tools/deepfm_jtm_bench.py [items=1000000] [depth=20] [out=profiles/deepfm_jtm_bench.json]

Shape: n items x 4 training rows, depth-d tree, E = 128, L = 10, gap 2, the fused call (dm_deepfm_jtm_optimize_cached /
dm_jtm_optimize_cached).  2 warm-ups, then the median of 7 runs.  Per run: wall seconds of JTM.optimize, the library's scoring /
re-balance split, and the HIP-event time of the two scorer kernels by kind (42 = dfm_jtm_rows_kernel, 43 = dfm_jtm_pairs_kernel; DIN:
30 = the general-rows kernel).  From those and the shapes: gathered bytes per second of both kernels, and a byte-count floor — the
bytes one gap step cannot avoid moving over 8 TB/s.  No pass mark: nothing ran this path before."""
import datetime
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine, synth
from dismember_amd.jtm import JTM

HBM_PEAK = 8.0e12            # bytes / s (spec)
WARMUP, RUNS = 2, 7


def main():
    items = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "deepfm_jtm_bench.json")
    E, L, nrow, gap = 128, 10, 4, 2
    T, NC = L + 1, 16 * ((L + 2 + 15) // 16)
    ni = (1 << (depth + 1)) - 1
    rng = np.random.default_rng(synth.SEED)
    tree = synth.make_tree(items, depth, rng)
    hist = synth.make_users(tree["leaf_ids"], 4 * 65536, L, np.random.default_rng(1))
    order = np.argsort(tree["leaf_ids"], kind="stable")
    pick = np.random.default_rng(2).integers(0, len(hist), size=items * nrow)
    row_off, row_ids = np.arange(items + 1, dtype=np.int64) * nrow, hist[pick].reshape(-1)
    # what one gap step has to move at least: every history row gathered once, s and aux written and read once, the codes in, the
    # logits out, and every DISTINCT node row of the step's levels once (the chain nodes of a step are at most the nodes of its levels)
    nchain = (2 << gap) - 2
    R, P = items * nrow, items * nrow * nchain
    steps = [(lo, min(depth, lo + gap)) for lo in range(0, depth, gap)]
    floor_bytes = 0
    for lo, hi in steps:
        nodes = sum(min(1 << lv, items) for lv in range(lo + 1, hi + 1))
        pairs = R * ((2 << (hi - lo)) - 2)
        floor_bytes += R * L * E * 4 + 2 * R * (E + NC) * 4 + R * L * 4 + 2 * pairs * 4 + nodes * E * 4
    rows_gather = len(steps) * R * L * E * 4                                   # bytes dfm_jtm_rows_kernel gathers per optimize
    pairs_gather = sum(R * ((2 << (hi - lo)) - 2) for lo, hi in steps) * (2 * E + NC) * 4     # node row + s + aux per pair

    def run(load, kinds):
        eng = Engine(0)
        eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], depth)
        eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
        load(eng)
        jt = JTM.from_arrays(eng, tree["leaf_ids"][order], tree["leaf_codes"][order], depth, row_off, row_ids, gap=gap, seq_len=L)
        rec = []
        proj = None
        for it in range(WARMUP + RUNS):
            tim = {}
            eng.timing_reset()
            t0 = time.perf_counter()
            proj = jt.optimize(timing=tim, as_array=True)
            dt = time.perf_counter() - t0
            if it >= WARMUP:
                rec.append(dict(wall_s=dt, scoring_s=tim["scoring_s"], rebalance_s=tim["rebalance_s"], rows_upload_s=tim["rows_upload_s"],
                                kernels={str(k): dict(zip(("launches", "ms"), eng.timing_get_kind(k))) for k in kinds}))
        ok = bool(np.unique(proj).size == items and int(proj.min()) >= (1 << depth) - 1)
        eng.close()
        med = lambda f: statistics.median(f(r) for r in rec)
        return dict(runs=rec, bijection_onto_leaves=ok, median_wall_s=med(lambda r: r["wall_s"]), median_scoring_s=med(lambda r: r["scoring_s"]),
                    median_rebalance_s=med(lambda r: r["rebalance_s"]),
                    median_kernel_ms={str(k): med(lambda r, k=k: r["kernels"][str(k)]["ms"]) for k in kinds})

    def load_deepfm(eng):
        g = np.random.default_rng(5)
        w = np.empty(ni * E + T * T * E + 2 * T + 1, np.float32)
        for a in range(0, w.size, 1 << 24):
            w[a:a + (1 << 24)] = g.standard_normal(min(1 << 24, w.size - a), dtype=np.float32) * np.float32(0.05)
        eng.load_weights_deepfm(w, E, L, ni)

    deepfm = run(load_deepfm, (42, 43))
    din = run(lambda eng: eng.load_weights_din_synthetic(E, ni, synth.SEED, tree_depth=depth, rho=0.95), (30,))
    k42, k43 = deepfm["median_kernel_ms"]["42"] * 1e-3, deepfm["median_kernel_ms"]["43"] * 1e-3
    res = dict(tool="tools/deepfm_jtm_bench.py", box=socket.gethostname(), date=datetime.date.today().isoformat(),
               shape=dict(items=items, depth=depth, E=E, L=L, rows_per_item=nrow, gap=gap, gap_steps=len(steps), rows=R, pairs_per_full_step=P),
               warmup=WARMUP, runs=RUNS, deepfm=deepfm, din=din,
               deepfm_rows_kernel=dict(seconds=k42, gathered_bytes=rows_gather, gathered_bytes_per_s=rows_gather / k42 if k42 > 0 else None),
               deepfm_pairs_kernel=dict(seconds=k43, gathered_bytes=pairs_gather, gathered_bytes_per_s=pairs_gather / k43 if k43 > 0 else None),
               floor=dict(bytes=floor_bytes, hbm_peak_bytes_per_s=HBM_PEAK, seconds=floor_bytes / HBM_PEAK,
                          kernel_seconds_over_floor=(k42 + k43) / (floor_bytes / HBM_PEAK) if k42 + k43 > 0 else None),
               deepfm_over_din_wall=deepfm["median_wall_s"] / din["median_wall_s"], deepfm_over_din_scoring=deepfm["median_scoring_s"] / din["median_scoring_s"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("deepfm", "din")}))
    print("deepfm: wall %.3f s, scoring %.3f s, re-balance %.3f s; din: wall %.3f s, scoring %.3f s, re-balance %.3f s" % (
        deepfm["median_wall_s"], deepfm["median_scoring_s"], deepfm["median_rebalance_s"], din["median_wall_s"], din["median_scoring_s"],
        din["median_rebalance_s"]))


if __name__ == "__main__":
    main()
