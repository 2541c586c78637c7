#!/usr/bin/env python3
"""OTM with the DeepFM scorer: the fused beam kernel against the TDM level pipeline, and one training iteration's phase split.

    python tools/deepfm_otm_bench.py [--out profiles/deepfm_otm_bench.json] [--users 16384] [--beam 200] [--repeats 7]

Search.  Complete tree of leaf level 20, E = 128, L = 10, beam 200, 16 384 users, device-resident request
(dm_deepfm_otm_beam_search_dev).  Protocol of tools/deepfm_bench.py: 2 warm-up calls, median of 7, wall clock around the call +
synchronize; kernel time through dm_kernel_timing_get_kind (42 = dfm_otm_beam_kernel), scored rows through dm_last_scored_rows, the
kernel's gathered bytes per second (scored rows x E x 4 / its time) beside the rate at which DESIGN.md §7 says this project's gathers
saturate.  Baseline: dm_tdm_beam_search_dev with the same DeepFM weights on a TDM tree of the same depth with every node present and
the same beam — the only other route that scores these rows (tdm_pl_fold + dfm_user_kernel / dfm_level_kernel).  The two are measured
in one session, alternating, `--rounds` times each; the figure compared is time per scored row.

Training.  One dm_deepfm_otm_train_batch at the reference conf's shape (8 192 users, beam 20, E = 16, leaf level 12): the
dm_otm_train_stats split, and the DM_DFM_TIME_LAUNCHES split (70 = rows kernel, 71 = l1.W product, 72 = embedding gradient, 73 = Adam)
of ONE level's step on a batch of the level's size.  The baseline of the user-grouped step.  One box, one run.
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


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def timed(eng, call, warmup, repeats, kinds):
    for _ in range(warmup):
        call()
        eng.synchronize()
    wall, per_kind = [], {k: [] for k in kinds}
    for _ in range(repeats):
        eng.timing_reset()
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        eng.synchronize()
        wall.append(time.perf_counter() - t0)
        for k in kinds:
            per_kind[k].append(eng.timing_get_kind(k))
    return wall, per_kind


def deepfm_weights(rng, E, L, num_index, std=0.05):
    T = L + 1
    n = num_index * E + T * T * E + 2 * T + 1
    w = np.empty(n, np.float32)
    chunk = 1 << 24
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        w[o:o + m] = rng.standard_normal(m, dtype=np.float32) * np.float32(std)
    return w


def search_part(a):
    from dismember_amd import Engine, synth
    E, L, depth, U, beam = a.embed, a.seq_len, a.depth, a.users, a.beam
    ni = (1 << (depth + 1)) - 1
    rng = np.random.default_rng(synth.SEED)
    tree = synth.make_tree(1 << depth, depth, rng)                  # every node present
    assert tree["codes"].size == ni
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], depth)
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_deepfm(deepfm_weights(rng, E, L, ni), E, L, ni)
    seqs = synth.make_users(tree["leaf_ids"], U, L, np.random.default_rng(synth.SEED + 1))        # item ids, 0 = padding
    code_of = np.full(int(tree["leaf_ids"].max()) + 1, -1, np.int32)
    code_of[tree["leaf_ids"]] = tree["leaf_codes"]
    codes = code_of[seqs]                                           # the same histories as node codes, -1 = padding
    d_items, d_codes = eng.dev_alloc(seqs.nbytes), eng.dev_alloc(codes.nbytes)
    eng.h2d(d_items, seqs); eng.h2d(d_codes, codes)
    stride = 2 * beam
    bufs = (eng.dev_alloc(U * stride * 4), eng.dev_alloc(U * stride * 4), eng.dev_alloc(U * 4))
    otm = lambda: eng.otm_beam_search_dev(d_codes, U, L, beam, depth, *bufs)
    tdm = lambda: eng.tdm_beam_search_dev(d_items, U, L, beam, stride, *bufs, use_mask=False)
    rounds = {"otm": [], "tdm": []}
    for r in range(a.rounds):                                       # alternating: both routes see the same box state
        for name, call, kinds in (("otm", otm, (42,)), ("tdm", tdm, (40, 41))):
            wall, per_kind = timed(eng, call, a.warmup, a.repeats, kinds)
            rows = eng.last_scored_rows()
            d = dict(kernel=eng.last_beam_kernel(), wall_s=summary(wall), users_per_s=U / statistics.median(wall), scored_rows=rows,
                     ns_per_scored_row=statistics.median(wall) * 1e9 / rows)
            for k in kinds:
                d["kind_%d_ms" % k] = summary([ms for _, ms in per_kind[k]])
                d["kind_%d_launches" % k] = per_kind[k][0][0]
            if name == "otm":
                ms = d["kind_42_ms"]["median"]
                d["gather_TB_per_s"] = rows * E * 4 / (ms * 1e-3) / 1e12
                d["fraction_of_gather_saturation"] = d["gather_TB_per_s"] / GATHER_SATURATION_TBS
                d["kernel_ns_per_scored_row"] = ms * 1e6 / rows
            else:
                d["kernels_ns_per_scored_row"] = (d["kind_40_ms"]["median"] + d["kind_41_ms"]["median"]) * 1e6 / rows
            rounds[name].append(d)
    med = lambda name, key: statistics.median(d[key] for d in rounds[name])
    out = dict(shape=dict(leaf_level=depth, E=E, L=L, beam=beam, users=U, num_index=ni), rounds=rounds,
               otm_ns_per_scored_row=med("otm", "ns_per_scored_row"), tdm_ns_per_scored_row=med("tdm", "ns_per_scored_row"),
               otm_users_per_s=med("otm", "users_per_s"), tdm_users_per_s=med("tdm", "users_per_s"),
               gather_saturation_TB_per_s=GATHER_SATURATION_TBS)
    out["tdm_over_otm_time_per_row"] = out["tdm_ns_per_scored_row"] / out["otm_ns_per_scored_row"]
    for p in (d_items, d_codes) + bufs:
        eng.dev_free(p)
    eng.close()
    return out


def train_part(a):
    from dismember_amd import Engine
    from dismember_amd.otm_train import OTMTrainer
    E, L, leaf, beam, U = 16, 10, 12, 20, a.train_users
    ni = (1 << (leaf + 1)) - 1
    rng = np.random.default_rng(7)
    eng = Engine(0)
    eng.load_weights_deepfm(deepfm_weights(rng, E, L, ni), E, L, ni)
    seqs = rng.integers((1 << leaf) - 1, ni, (U, L)).astype(np.int32)
    seqs[rng.random((U, L)) < 0.15] = -1
    targets = [rng.integers((1 << leaf) - 1, ni, 1 + int(k)).tolist() for k in rng.integers(0, 4, U)]
    tr = OTMTrainer(eng, leaf_level=leaf, beam=beam, seq_len=L)
    tr.train_batch(seqs, targets)                                   # warm-up: buffers grow here
    losses = tr.train_batch(seqs, targets)
    out = dict(shape=dict(users=U, beam=beam, E=E, L=L, leaf_level=leaf), level_losses=losses, stats=tr.last_stats())
    # one level's step, launch by launch
    B = U * 2 * beam
    codes = rng.integers(0, ni, B).astype(np.int32)
    rows = np.repeat(seqs, 2 * beam, axis=0)
    labels = (rng.random(B) < 0.02).astype(np.float32)
    os.environ["DM_DFM_TIME_LAUNCHES"] = "1"
    try:
        eng.deepfm_train_forward_backward(codes, rows, labels); eng.deepfm_adam_step()
        eng.timing_reset()
        eng.deepfm_train_forward_backward(codes, rows, labels); eng.deepfm_adam_step()
        eng.synchronize()
        names = {70: "rows_kernel", 71: "l1w_product", 72: "embedding_gradient", 73: "adam"}
        out["one_level_step"] = dict(rows=B, **{names[k]: dict(zip(("launches", "ms"), eng.timing_get_kind(k))) for k in names})
    finally:
        del os.environ["DM_DFM_TIME_LAUNCHES"]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfm_otm_bench.json"))
    ap.add_argument("--users", type=int, default=16384)
    ap.add_argument("--beam", type=int, default=200)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-users", type=int, default=8192)
    a = ap.parse_args()
    res = dict(note="one box, one run", warmup=a.warmup, repeats=a.repeats, search=search_part(a), training=train_part(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
