#!/usr/bin/env python3
"""DeepFM serving benchmark: TDM beam search through the level pipeline with the DeepFM scorer (csrc/deepfm.hip.inc).

    python tools/deepfm_bench.py [--out profiles/deepfm_bench.json] [--users 16384] [--beam 200] [--repeats 7]

Shape: 1 M-item tree of depth 20, E = 128, L = 10, beam 200, top-k 200, device-resident request (dm_tdm_beam_search_dev).
Reported: users/s (wall clock around the call + synchronize, median of the repeats after warm-up), kernel time per kind through
dm_kernel_timing_get_kind (40 = dfm_user_kernel, 41 = dfm_level_kernel), the level kernel's gathered bytes per second
(scored rows x E x 4 / its time) beside the rate at which DESIGN.md §7 says this project's gathers saturate, and — the only
like-for-like figure the DIN side offers — the DIN model on the same tree forced through the same level pipeline at L = 17
(DM_LONG_PIPELINE=1).  One box, one run: the JSON says so.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATHER_SATURATION_TBS = 9.5


def timed_search(eng, d_seq, U, L, beam, topk, bufs, warmup, repeats, kinds=()):
    d_ids, d_sc, d_cnt = bufs
    for _ in range(warmup):
        eng.tdm_beam_search_dev(d_seq, U, L, beam, topk, d_ids, d_sc, d_cnt, use_mask=False)
        eng.synchronize()
    wall, per_kind = [], {k: [] for k in kinds}
    for _ in range(repeats):
        eng.timing_reset()
        eng.synchronize()
        t0 = time.perf_counter()
        eng.tdm_beam_search_dev(d_seq, U, L, beam, topk, d_ids, d_sc, d_cnt, use_mask=False)
        eng.synchronize()
        wall.append(time.perf_counter() - t0)
        for k in kinds:
            per_kind[k].append(eng.timing_get_kind(k))
    return wall, per_kind


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfm_bench.json"))
    ap.add_argument("--users", type=int, default=16384)
    ap.add_argument("--beam", type=int, default=200)
    ap.add_argument("--topk", type=int, default=200)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()

    from dismember_amd import Engine, synth
    E, L, depth, U = a.embed, a.seq_len, a.depth, a.users
    num_index = (1 << (depth + 1)) - 1
    rng = np.random.default_rng(synth.SEED)
    tree = synth.make_tree(a.items, depth, rng)
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], depth)
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    bufs = (eng.dev_alloc(U * a.topk * 4), eng.dev_alloc(U * a.topk * 4), eng.dev_alloc(U * 4))
    res = dict(note="one box, one run", shape=dict(items=a.items, depth=depth, E=E, beam=a.beam, topk=a.topk, users=U),
               warmup=a.warmup, repeats=a.repeats)

    # ---- DeepFM, L = seq_len
    T = L + 1
    n = num_index * E + T * T * E + 2 * T + 1
    w = np.empty(n, np.float32)
    w[:] = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)
    eng.load_weights_deepfm(w, E, L, num_index)
    del w
    seqs = synth.make_users(tree["leaf_ids"], U, L, np.random.default_rng(synth.SEED + 1))
    d_seq = eng.dev_alloc(U * L * 4)
    eng.h2d(d_seq, seqs)
    wall, kinds = timed_search(eng, d_seq, U, L, a.beam, a.topk, bufs, a.warmup, a.repeats, kinds=(40, 41))
    rows = eng.last_scored_rows()
    level_ms = [ms for _, ms in kinds[41]]
    user_ms = [ms for _, ms in kinds[40]]
    gather_tbs = rows * E * 4 / (statistics.median(level_ms) * 1e-3) / 1e12
    res["deepfm"] = dict(L=L, kernel=eng.last_beam_kernel(), wall_s=summary(wall), users_per_s=U / statistics.median(wall),
                         scored_rows=rows, dfm_user_kernel_ms=summary(user_ms), dfm_level_kernel_ms=summary(level_ms),
                         level_launches=kinds[41][0][0], user_launches=kinds[40][0][0],
                         level_gather_TB_per_s=gather_tbs, gather_saturation_TB_per_s=GATHER_SATURATION_TBS,
                         level_fraction_of_saturation=gather_tbs / GATHER_SATURATION_TBS,
                         kernels_fraction_of_wall=(statistics.median(level_ms) + statistics.median(user_ms)) * 1e-3 / statistics.median(wall))
    eng.dev_free(d_seq)

    # ---- DIN on the same tree through the same level pipeline (L = 17, DM_LONG_PIPELINE=1)
    Ld = 17
    eng.load_weights_din_synthetic(E, num_index, synth.SEED)
    eng.set_scorer_mode("f32")
    seqs = synth.make_users(tree["leaf_ids"], U, Ld, np.random.default_rng(synth.SEED + 2))
    d_seq = eng.dev_alloc(U * Ld * 4)
    eng.h2d(d_seq, seqs)
    os.environ["DM_LONG_PIPELINE"] = "1"
    try:
        wall, _ = timed_search(eng, d_seq, U, Ld, a.beam, a.topk, bufs, a.warmup, a.repeats)
    finally:
        del os.environ["DM_LONG_PIPELINE"]
    res["din_level_pipeline"] = dict(L=Ld, kernel=eng.last_beam_kernel(), wall_s=summary(wall), users_per_s=U / statistics.median(wall),
                                     scored_rows=eng.last_scored_rows())
    res["deepfm_over_din_pipeline_users_per_s"] = res["deepfm"]["users_per_s"] / res["din_level_pipeline"]["users_per_s"]
    eng.dev_free(d_seq)
    for b in bufs:
        eng.dev_free(b)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
