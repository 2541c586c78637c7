"""OTM tree construction's child weights with the DeepFM scorer at catalogue scale: the pair route the library had before against the
one-shot call and the prepared form of csrc/dfm_otm_tree.hip.inc.

  python tools/deepfm_otm_tree_bench.py [items=1000000] [out=profiles/deepfm_otm_tree_bench.json]

Shape: a complete tree whose leaf level is upperLog2(items) (20 at the default), L = 10, gap 2, E = 128 and again E = 16; item of
rank k owns max(1, floor(100000 / k)) history rows (Zipf: a few items with 10^5 rows, most with one).  The gap step measured is the
last one (old_level = leaf level - 2), every item in the ancestor of a random leaf.  Routes, alternating in one session, 2 warm-ups,
then the median of 7:
  1. pairs      Engine.deepfm_pairs_forward on the host-expanded (row, chain node) codes (seq_div = nchain: the histories are not
                replicated) plus the double sums and the chain on the host (numpy): what the library could do before
  2. one_shot   Engine.deepfm_otm_child_weights
  3. prepare    Engine.deepfm_otm_tree_prepare, and  step: one Engine.deepfm_otm_tree_weights on it
and a whole TreeConstruction.run (prepared; 1 warm-up, median of 3).  Per run: wall seconds and the HIP-event milliseconds by launch
kind (42 = per-history set-up, 43 = pair kernel, 44 = unit scores, 45 = segment sums + chain).  From the score kernel's time: the bytes
of S + aux it reads per second against the 9.5 TB/s at which the project's gathers saturate, and the share of tile
rows that are live.  No pass mark."""
import datetime
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine
from dismember_amd.otm_tree import TreeConstruction

GATHER_SATURATION = 9.5e12   # bytes / s
WARMUP, RUNS = 2, 7
KINDS = (42, 43, 44, 45)


def chain_codes(node, gap):
    node = node.astype(np.int64)
    return np.stack([(node << d) + (1 << d) - 1 + c for d in range(1, gap + 1) for c in range(1 << d)], 1).astype(np.int32)


def shape_run(E, items, L=10, gap=2):
    leaf_level = int(np.ceil(np.log(items) / np.log(2)))
    ni = (2 << leaf_level) - 1
    T, NC = L + 1, 16 * ((L + 2 + 15) // 16)
    nchain, nchild = (2 << gap) - 2, 1 << gap
    ntiles = (nchain + 15) // 16
    rng = np.random.default_rng(20)
    counts = np.maximum(1, 100000 // np.arange(1, items + 1)).astype(np.int64)
    counts = counts[rng.permutation(items)]
    row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(row_off[-1])
    rows = rng.integers((1 << leaf_level) - 1, ni, (R, L)).astype(np.int32)
    rows[rng.random((R, L)) < 0.15] = -1
    leaves = ((1 << leaf_level) - 1 + rng.permutation(1 << leaf_level)[:items]).astype(np.int32)
    old_level, level = leaf_level - gap, leaf_level
    node = TreeConstruction.ancestor_at_level(leaves, old_level)
    g = np.random.default_rng(5)
    w = np.empty(ni * E + T * T * E + 2 * T + 1, np.float32)
    for a in range(0, w.size, 1 << 24):
        w[a:a + (1 << 24)] = g.standard_normal(min(1 << 24, w.size - a), dtype=np.float32) * np.float32(0.05)
    eng = Engine(0)
    eng.load_weights_deepfm(w, E, L, ni)
    del w
    item_of_row = np.repeat(np.arange(items), counts)
    has = counts > 0

    def pairs_route():
        codes = chain_codes(node, gap)[item_of_row].reshape(-1)                  # host expansion: [R * nchain]
        lg = eng.deepfm_pairs_forward(codes, rows, seq_div=nchain).reshape(R, nchain).astype(np.float64)
        score = np.add.reduceat(lg, row_off[:-1], 0)
        wts = np.zeros((items, nchild))
        idx = np.arange(nchild)
        for d in range(gap, 0, -1):
            wts += score[:, (1 << d) - 2 + idx]
            idx = idx >> 1
        wts[~has] = -1e6
        return wts

    def timed(fn):
        eng.timing_reset()
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        return r, dict(wall_s=dt, kernels={str(k): dict(zip(("launches", "ms"), eng.timing_get_kind(k))) for k in KINDS})

    rec = {k: [] for k in ("pairs", "one_shot", "prepare", "step")}
    agree = None
    for it in range(WARMUP + RUNS):
        a, ta = timed(pairs_route)
        b, tb = timed(lambda: eng.deepfm_otm_child_weights(row_off, rows, node, old_level, level))
        _, tp = timed(lambda: eng.deepfm_otm_tree_prepare(row_off, rows))
        c, tc_ = timed(lambda: eng.deepfm_otm_tree_weights(node, old_level, level))
        eng.deepfm_otm_tree_release()
        if it == 0:
            agree = dict(one_shot_equals_prepared=bool(b.tobytes() == c.tobytes()),
                         max_rel_diff_to_pairs_route=float((np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()))
        if it >= WARMUP:
            for k, t in (("pairs", ta), ("one_shot", tb), ("prepare", tp), ("step", tc_)):
                rec[k].append(t)
    med = lambda rs, f: statistics.median(f(r) for r in rs)
    routes = {k: dict(runs=v, median_wall_s=med(v, lambda r: r["wall_s"]),
                      median_kernel_ms={str(kk): med(v, lambda r, kk=kk: r["kernels"][str(kk)]["ms"]) for kk in KINDS}) for k, v in rec.items()}
    # a whole construction through the prepared form
    tc = TreeConstruction.__new__(TreeConstruction)
    tc.engine, tc.items, tc.item_leaf, tc.leaf_level = eng, np.arange(1, items + 1, dtype=np.int32), leaves, leaf_level
    tc.gap, tc.L, tc.use_mask, tc.comm, tc.deepfm, tc.row_off, tc.row_codes = gap, L, False, None, True, row_off, rows.reshape(-1)
    whole = []
    for it in range(1 + 3):
        eng.timing_reset()
        t0 = time.perf_counter()
        proj = tc.run()
        dt = time.perf_counter() - t0
        if it >= 1:
            whole.append(dict(wall_s=dt, kernels={str(k): dict(zip(("launches", "ms"), eng.timing_get_kind(k))) for k in KINDS}))
    nodes = np.fromiter(proj.values(), np.int64, len(proj))
    eng.close()
    score_s = routes["step"]["median_kernel_ms"]["44"] * 1e-3
    s_aux = R * ntiles * (E + NC) * 4
    p_wall = routes["pairs"]["median_wall_s"]
    return dict(shape=dict(items=items, leaf_level=leaf_level, E=E, L=L, gap=gap, old_level=old_level, level=level, rows=R, max_rows_per_item=int(counts.max()),
                           items_with_one_row=int((counts == 1).sum()), pairs=R * nchain, chain_tiles=ntiles),
                agreement=agree, routes=routes,
                construction=dict(runs=whole, median_wall_s=med(whole, lambda r: r["wall_s"]), gap_steps=-(-leaf_level // gap),
                                  bijection_onto_leaves=bool(np.unique(nodes).size == items and int(nodes.min()) >= (1 << leaf_level) - 1)),
                score_kernel=dict(seconds=score_s, s_aux_bytes=s_aux, s_aux_bytes_per_s=s_aux / score_s if score_s > 0 else None,
                                  share_of_gather_saturation=(s_aux / score_s) / GATHER_SATURATION if score_s > 0 else None,
                                  live_tile_rows=nchain, tile_rows=16 * ntiles, live_share=nchain / (16.0 * ntiles)),
                ratios_to_pairs_route=dict(one_shot_wall=routes["one_shot"]["median_wall_s"] / p_wall, step_wall=routes["step"]["median_wall_s"] / p_wall,
                                           prepare_wall=routes["prepare"]["median_wall_s"] / p_wall,
                                           step_kernels_over_pair_kernels=(routes["step"]["median_kernel_ms"]["44"] + routes["step"]["median_kernel_ms"]["45"]) /
                                           max(1e-9, routes["pairs"]["median_kernel_ms"]["42"] + routes["pairs"]["median_kernel_ms"]["43"])))


def main():
    items = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "deepfm_otm_tree_bench.json")
    res = dict(tool="tools/deepfm_otm_tree_bench.py", box=socket.gethostname(), date=datetime.date.today().isoformat(), warmup=WARMUP, runs=RUNS,
               shapes=[shape_run(E, items) for E in (128, 16)])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for s in res["shapes"]:
        print(json.dumps({k: v for k, v in s.items() if k not in ("routes", "construction")}))
        print("E = %d: pairs %.4f s, one-shot %.4f s, prepare %.4f s, step %.4f s, construction %.3f s" % (
            s["shape"]["E"], s["routes"]["pairs"]["median_wall_s"], s["routes"]["one_shot"]["median_wall_s"], s["routes"]["prepare"]["median_wall_s"],
            s["routes"]["step"]["median_wall_s"], s["construction"]["median_wall_s"]))


if __name__ == "__main__":
    main()
