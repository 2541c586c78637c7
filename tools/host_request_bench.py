#!/usr/bin/env python3
"""The host-side figures of bench.py that the host-request layer (csrc/host_request.hip.inc) can move, one library against another.

    python tools/host_request_bench.py --libs parent=/path/to/libdismember_hip.so new=dismember_amd/libdismember_hip.so --rounds 3 --out FILE.json

Every round of every library is a fresh child process (DM_LIB_PATH names the library), the libraries alternate, and the raw figure of
every round is written.  The workloads and the protocols are bench.py's own:
  tdm_host_buffer_users_per_s   the headline workload (10M-item depth-24 tree, E = 128, beam = topk = 200, L = 10, 131 072 users per step)
                                through dm_tdm_beam_search, 3 timed steps after one untimed (bench.py: host_buffer_users_per_s)
  otm_host_buffer_users_per_s   OTM serving on the same table, 32 768 users, one timed call after one untimed (extra_otm.host_buffer_users_per_s)
  tdm_recommend_ms              TDM.recommend on the bundled trained model, one user per call: 10 warm-up calls, median of five blocks of 100
  otm_recommend_ms              OTM.recommend on the bundled DIN[Double]: 10 + 100 calls
  dr_recommend_ms               DeepRetrieval.recommend, synthetic fp64 model over the bundled item -> path mapping: 10 + 100 calls
`verdict` compares, per figure, the new library's rounds with the range the parent's rounds span."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIGURES = ("tdm_host_buffer_users_per_s", "otm_host_buffer_users_per_s", "tdm_recommend_ms", "otm_recommend_ms", "dr_recommend_ms")


def one_round():
    from dismember_amd import OTM, TDM, DeepRetrieval, Engine, synth
    E, L, depth, beam, topk, U, Uo = 128, 10, 24, 200, 200, 131072, 32768
    out = {}
    tree = synth.make_tree(10_000_000, depth, np.random.default_rng(synth.SEED))
    shards = [synth.make_users(tree["leaf_ids"], U, L, np.random.default_rng(synth.SEED + 1 + 1000 * k)) for k in range(3)]
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], depth)
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_din_synthetic(E, (1 << (depth + 1)) - 1, synth.SEED, tree_depth=depth, rho=0.95)
    hout = (np.empty((U, topk), np.int32), np.empty((U, topk), np.float32), np.empty(U, np.int32))
    eng.tdm_beam_search(shards[0], beam, topk, out=hout)
    eng.synchronize()
    t0 = time.perf_counter()
    for k in range(3):
        eng.tdm_beam_search(shards[k], beam, topk, out=hout)
    eng.synchronize()
    out["tdm_host_buffer_users_per_s"] = U * 3 / (time.perf_counter() - t0)
    lut = np.zeros(int(tree["leaf_ids"].max()) + 1, np.int32)
    lut[tree["leaf_ids"]] = tree["leaf_codes"]
    seqs = shards[0][:Uo]
    ocodes = np.where(seqs > 0, lut[np.clip(seqs, 0, lut.size - 1)], -1).astype(np.int32)
    oout = (np.empty((Uo, 2 * beam), np.int32), np.empty((Uo, 2 * beam), np.float32), np.empty(Uo, np.int32))
    eng.otm_beam_search(ocodes, beam, depth, out=oout)
    t0 = time.perf_counter()
    eng.otm_beam_search(ocodes, beam, depth, out=oout)
    out["otm_host_buffer_users_per_s"] = Uo / (time.perf_counter() - t0)
    eng.close()

    def per_call(model, query, blocks):
        for _ in range(10):
            model.recommend(query, 10, 20)
        ts = []
        for _ in range(blocks):
            t0 = time.perf_counter()
            for _ in range(100):
                model.recommend(query, 10, 20)
            ts.append((time.perf_counter() - t0) / 100)
        return float(np.median(ts)) * 1e3

    g = os.path.join(ROOT, "tests", "golden")
    t1 = np.load(os.path.join(g, "tdm_tree.npz"))
    e1 = Engine(0)
    e1.load_tree(t1["codes"], t1["ids"], t1["is_leaf"], int(t1["max_level"]))
    e1.load_id_maps(t1["leaf_ids"], t1["leaf_codes"])
    e1.load_weights_din(np.load(os.path.join(g, "din_f32.npy")), 16, 8191)
    out["tdm_recommend_ms"] = per_call(TDM(e1, "din"), np.array([0, 0, 2126, 204, 3257, 3439, 996, 1681, 3438, 1882], np.int32), 5)
    e1.close()
    om = np.load(os.path.join(g, "otm_mapping.npy"))
    e2 = Engine(0)
    e2.load_weights_din(np.load(os.path.join(g, "din_f64.npy")), 16, 8191)
    out["otm_recommend_ms"] = per_call(OTM(e2, {int(a): int(b) for a, b in om}), [int(x) for x in om[:10, 0]], 1)
    e2.close()
    dm = np.load(os.path.join(g, "dr_mapping.npz"))
    nit = int(dm["ids"].max()) + 1
    ip = np.zeros((nit, dm["paths"].shape[1], 3), np.int32)
    ip[dm["ids"]] = dm["paths"]
    e3 = Engine(0)
    e3.dr_load_model(synth.make_dr_model(nit, 100, 3, 10, 16, np.random.default_rng(11), scale=0.3), 16, 10, 100, 3, nit, dtype=np.float64)
    e3.dr_load_path_items(*synth.dr_path_items(ip))
    out["dr_recommend_ms"] = per_call(DeepRetrieval(e3, {int(i): int(d) for i, d in zip(dm["items"], dm["ids"])}), [int(x) for x in dm["items"][:10]], 1)
    e3.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", metavar="NAME=PATH", help="the libraries to compare, the reference first")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--round", action="store_true", help=argparse.SUPPRESS)          # a child: one round of the library DM_LIB_PATH names
    a = ap.parse_args()
    if a.round:
        print("ROUND " + json.dumps(one_round()))
        return
    libs = [s.split("=", 1) for s in a.libs]
    rounds = {name: [] for name, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ, DM_LIB_PATH=os.path.abspath(path))
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--round"], env=env, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                sys.exit("round %d of %s failed (exit %d):\n%s" % (r, name, done.returncode, done.stdout[-2000:] + done.stderr[-2000:]))
            rounds[name].append(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("ROUND ")][-1][6:]))
            print(name, r, rounds[name][-1], flush=True)
    ref = libs[0][0]
    verdict = {}
    for name, _ in libs[1:]:
        for f in FIGURES:
            lo, hi = min(x[f] for x in rounds[ref]), max(x[f] for x in rounds[ref])
            vals = [x[f] for x in rounds[name]]
            verdict["%s.%s" % (name, f)] = {"%s_range" % ref: [lo, hi], "%s_range" % name: [min(vals), max(vals)], "rounds_inside": sum(lo <= v <= hi for v in vals),
                                            "rounds": len(vals)}
    res = {"what": __doc__.split("\n\n")[0], "order": "alternating, %s first, %d rounds each, one process per round" % (ref, a.rounds),
           "rounds": rounds, "verdict": verdict}
    print(json.dumps(res["verdict"], indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
