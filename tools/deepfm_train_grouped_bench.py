#!/usr/bin/env python3
"""User-grouped DeepFM training step (dm_deepfm_train_forward_backward_grouped_dev; csrc/dfm_train_grouped.hip.inc)
against the row step (dm_deepfm_train_forward_backward_dev) on the same batch.

    python tools/deepfm_train_grouped_bench.py [--out profiles/deepfm_train_grouped_bench.json]

Shapes: DESIGN.md §15's OTM level (8 192 users x 40 rows, E = 16, L = 10, leaf level 12) and 16 384 x 400 at E = 128, L = 10 (leaf level
20).  A shape whose U R exceeds the 4 194 240 rows both steps accept is run with U halved until it fits; `requested` and `ran` say so.
Protocol: one session, the same device-resident inputs for both steps (the row step's histories are the users' repeated R times),
`--rounds` rounds (at least three) that alternate row step / grouped step; in a round each step gets two warm-up calls and then
`--repeats` timed calls, each ending in a stream synchronise; a round's figure is the median of its calls.  No Adam step in between: the
weights and hence the work stay the same.  Then one further call of each under DM_DFM_TIME_LAUNCHES=1 for the per-kind event times
(kinds 70 .. 76; host work between the launches is in the step time and in none of them).
Then one whole dm_deepfm_otm_train_batch (8 192 users, beam 20, E = 16, leaf level 12) with and without DM_DFM_TRAIN_GROUPED=1,
alternating over the same rounds, one warm-up call each; dm_otm_train_stats' forward/backward seconds beside the wall time.
One box, one run; not profiled: hardware counters, occupancy, achieved memory traffic."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_ROWS = 65535 * 64
KINDS = {"rows_kernel": 70, "l1w_products": 71, "embedding_gradient": 72, "grouped_user_setup": 74, "grouped_rows_kernel": 75,
         "grouped_user_backward": 76}


def deepfm_weights(rng, E, L, ni):
    T = L + 1
    n = ni * E + T * T * E + 2 * T + 1
    w = np.empty(n, np.float32)
    w[:] = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)
    return w


def timed(call, sync, warmup, repeats):
    for _ in range(warmup):
        call(); sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call(); sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def spread(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def step_part(a, U_req, R, E, L, leaf):
    from dismember_amd import Engine
    U = U_req
    while U * R > MAX_ROWS:
        U //= 2
    ni = (1 << (leaf + 1)) - 1
    rng = np.random.default_rng(7)
    eng = Engine(0)
    eng.load_weights_deepfm(deepfm_weights(rng, E, L, ni), E, L, ni)
    eng.deepfm_train_init(lr=1e-3)
    seq = rng.integers((1 << leaf) - 1, ni, (U, L)).astype(np.int32)
    seq[rng.random((U, L)) < 0.15] = -1
    B = U * R
    codes = rng.integers(0, ni, B).astype(np.int32)
    lab = (rng.random(B) < 0.02).astype(np.float32)
    d_seq, d_codes, d_lab, d_rows = eng.dev_alloc(U * L * 4), eng.dev_alloc(B * 4), eng.dev_alloc(B * 4), eng.dev_alloc(B * L * 4)
    eng.h2d(d_seq, seq); eng.h2d(d_codes, codes); eng.h2d(d_lab, lab); eng.h2d(d_rows, np.repeat(seq, R, axis=0))
    loss = {}

    def row():
        loss["row"] = eng.deepfm_train_forward_backward_dev(d_codes, d_rows, d_lab, B, L)

    def grouped():
        loss["grouped"] = eng.deepfm_train_forward_backward_grouped_dev(d_seq, d_codes, d_lab, U, R, L)
    rounds = []
    for _ in range(a.rounds):
        r = dict(row_ms=spread(timed(row, eng.synchronize, 2, a.repeats)), grouped_ms=spread(timed(grouped, eng.synchronize, 2, a.repeats)))
        r["row_over_grouped"] = r["row_ms"]["median"] / r["grouped_ms"]["median"]
        rounds.append(r)
    kinds = {}
    os.environ["DM_DFM_TIME_LAUNCHES"] = "1"
    try:
        for name, call in (("row", row), ("grouped", grouped)):
            eng.timing_reset()
            call(); eng.synchronize()
            kinds[name] = {k: dict(zip(("launches", "ms"), eng.timing_get_kind(v))) for k, v in KINDS.items() if eng.timing_get_kind(v)[0]}
    finally:
        del os.environ["DM_DFM_TIME_LAUNCHES"]
    for p in (d_seq, d_codes, d_lab, d_rows):
        eng.dev_free(p)
    eng.close()
    return dict(requested=dict(users=U_req, rows_per_user=R), ran=dict(users=U, rows_per_user=R, rows=B, E=E, L=L, leaf_level=leaf, slots_row=B * (L + 1),
                                                                          slots_grouped=B + U * L),
                rounds=rounds, grouped_faster_in_every_round=all(r["row_over_grouped"] > 1 for r in rounds),
                row_over_grouped=spread([r["row_over_grouped"] for r in rounds]), loss=loss, kinds_ms_one_call=kinds)


def otm_part(a):
    from dismember_amd import Engine
    from dismember_amd.otm_train import OTMTrainer
    E, L, leaf, beam, U = 16, 10, 12, 20, a.train_users
    ni = (1 << (leaf + 1)) - 1
    rng = np.random.default_rng(7)
    w = deepfm_weights(rng, E, L, ni)
    seqs = rng.integers((1 << leaf) - 1, ni, (U, L)).astype(np.int32)
    seqs[rng.random((U, L)) < 0.15] = -1
    targets = [rng.integers((1 << leaf) - 1, ni, 1 + int(k)).tolist() for k in rng.integers(0, 4, U)]
    eng = Engine(0)
    rounds = []
    for _ in range(a.rounds):
        r = {}
        for name, env in (("row", None), ("grouped", "1")):
            if env:
                os.environ["DM_DFM_TRAIN_GROUPED"] = env
            try:
                eng.load_weights_deepfm(w, E, L, ni)                 # the same weights for every timed iteration
                tr = OTMTrainer(eng, leaf_level=leaf, beam=beam, seq_len=L)
                tr.train_batch(seqs, targets)                        # warm-up: buffers grow here
                eng.load_weights_deepfm(w, E, L, ni)
                tr = OTMTrainer(eng, leaf_level=leaf, beam=beam, seq_len=L)
                t0 = time.perf_counter()
                losses = tr.train_batch(seqs, targets)
                r[name] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, stats=tr.last_stats(), first_level_loss=losses[0], last_level_loss=losses[-1])
            finally:
                os.environ.pop("DM_DFM_TRAIN_GROUPED", None)
        rounds.append(r)
    eng.close()
    return dict(shape=dict(users=U, beam=beam, E=E, L=L, leaf_level=leaf), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfm_train_grouped_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train-users", type=int, default=8192)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    assert a.rounds >= 3
    res = dict(note="one box, one run", rounds=a.rounds, repeats=a.repeats, warmup=2, otm_level=step_part(a, 8192, 40, 16, 10, 12))
    if not a.skip_large:
        res["large"] = step_part(a, 16384, 400, 128, 10, 20)
    res["otm_train_batch"] = otm_part(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
