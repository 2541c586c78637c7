#!/usr/bin/env python3
"""Times TDMClusterTree on a synthetic table and writes profiles/cluster_bench.json (a measurement tool, not a gate).

    python tools/cluster_bench.py [--items N --embed E --restarts R --rho 0.8 --out profiles/cluster_bench.json]

The table is dm_fill_tree_normal's (row(c) = rho * row(parent) + noise: a hierarchy to find) and the items sit on its leaves under a
random permutation; the rows are gathered on the device (dm_cluster_tree_model).  Recorded: seconds per phase, Lloyd passes, bytes
streamed, GB/s of the streaming passes, and per level the fraction of the built tree's nodes whose item set is a planted node's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dismember_amd import Engine  # noqa: E402


def recovery(codes, planted_leaf, depth, level):
    codes = codes.astype(np.int64)
    d = np.floor(np.log2(codes + 1.0)).astype(np.int64)
    node = ((codes + 1) >> np.maximum(d - level, 0)) - 1
    grp = planted_leaf >> (depth - level)
    pairs = np.unique(np.stack([node, grp], axis=1), axis=0, return_counts=True)
    nodes, per_node = np.unique(pairs[0][:, 0], return_counts=True)
    gsize = np.bincount(grp)
    pure = dict(zip(nodes[per_node == 1].tolist(), [True] * int((per_node == 1).sum())))
    hit = sum(1 for (nd, g), c in zip(pairs[0].tolist(), pairs[1].tolist()) if nd in pure and c == gsize[g])
    return hit / float(1 << level)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=10_000_000)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--restarts", type=int, default=10)
    ap.add_argument("--rho", type=float, default=0.8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    a = ap.parse_args()
    n, E = a.items, a.embed
    depth = max(1, int(n - 1).bit_length())
    ni = (1 << (depth + 1)) - 1
    eng = Engine(0)
    eng.load_weights_din_synthetic(E, ni, a.seed, tree_depth=depth, rho=a.rho)
    leaf = np.random.default_rng(a.seed).permutation(1 << depth)[:n].astype(np.int64)
    ids = np.arange(1, n + 1, dtype=np.int32)
    eng.load_id_maps(ids, ((1 << depth) - 1 + leaf).astype(np.int32))
    t0 = time.perf_counter()
    codes, st, _ = eng.cluster_tree(item_ids=ids, restarts=a.restarts, seed=a.seed)
    wall = time.perf_counter() - t0
    stream_s = st["seeding_s"] + st["lloyd_s"] + st["split_s"]
    res = dict(items=n, embed=E, restarts=a.restarts, rho=a.rho, wall_s=wall, stats=st,
               streaming_GBps=(st["bytes_streamed"] - n * eng.E * 4) / 1e9 / stream_s if stream_s > 0 else None,
               recovery={str(l): recovery(codes, leaf, depth, l) for l in range(1, min(depth, 8) + 1)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    eng.close()


if __name__ == "__main__":
    main()
