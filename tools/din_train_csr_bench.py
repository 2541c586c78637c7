#!/usr/bin/env python3
"""Ragged (CSR) user-grouped DIN training path of an f32 model (dm_tdm_sample_train_batch_csr_dev + dm_train_forward_backward_csr_dev;
csrc/train_grouped_csr.hip.inc) against the row path (dm_tdm_sample_train_batch_dev + dm_train_forward_backward_dev) on
the TDM sampler's own batch, use_mask on.

    python tools/din_train_csr_bench.py [--out profiles/din_train_csr_bench.json]

Batch: `--targets` targets (16 384) drawn from a tree whose leaves lie on two levels (complete down to level `--depth` - 1, the first
half of that level's nodes have both children on level `--depth`), negatives per level min(2^l - 1, 6), L = 10, at E = 16 and E = 128.
One target in 64 is padding (no rows).  A batch whose row bound exceeds the 4 194 240 rows both steps accept is run with the targets
halved until it fits; `requested` and `ran` say so.
Protocol (that of tools/deepfm_train_csr_bench.py): one session, the same device-resident item ids and targets for both paths,
`--rounds` rounds (at least three) that alternate row path / CSR path; in a round every figure gets two warm-up calls and then `--repeats`
timed calls, each ending in a stream synchronise; a round's figure is the median of its calls.  Two figures per path: sampler plus
forward/backward, and forward/backward alone on the batch the sampler left in the buffers.  Both steps ADD to the gradient and no Adam
step runs in between: the weights and hence the work stay the same.  Then one further CSR forward/backward under DM_TRAIN_TIME_LAUNCHES=1
for the per-kind event times (kinds 56 .. 59 and 68; the offset check, the index and tile lists and host work between the launches are in
the step time and in none of them; the row step records no kinds).
Then one whole TDMTrainer.step (upload of ids, sampler, step, Adam) with din_grouped=False and din_grouped=True, alternating over the same
rounds.
One box, one run; not profiled: hardware counters, occupancy, achieved memory traffic."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_ROWS = 65535 * 64
L = 10
KINDS = {"user_setup": 56, "rows_kernel": 57, "user_backward": 58, "dense_gradients": 59, "embedding_gradient": 68}


def din_weights(rng, E, ni):
    n = ni * E + 3 * E * E + 2 * E + 1
    return rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)


def two_level_tree(depth):
    """leaves on levels depth - 1 and depth: (dict for load_tree / load_id_maps, number of items)"""
    lo = (1 << (depth - 1)) - 1                                   # first code of level depth - 1
    half = 1 << (depth - 2)
    leaf_codes = np.concatenate([np.arange((1 << depth) - 1, (1 << depth) - 1 + 2 * half), np.arange(lo + half, lo + 2 * half)]).astype(np.int32)
    n = leaf_codes.size
    leaf_ids = (np.random.default_rng(5).permutation(n) + 1).astype(np.int32)
    codes = np.concatenate([np.arange(0, lo + half), np.sort(leaf_codes)]).astype(np.int32)
    ids = codes + (n + 1)
    order = np.argsort(leaf_codes)
    pos = np.searchsorted(codes, leaf_codes[order])
    ids[pos] = leaf_ids[order]
    is_leaf = np.zeros(codes.size, np.uint8)
    is_leaf[pos] = 1
    return dict(codes=codes, ids=ids.astype(np.int32), is_leaf=is_leaf, leaf_ids=leaf_ids, leaf_codes=leaf_codes, max_level=depth), n


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


def make_engine(E, depth, tree, rng):
    from dismember_amd import Engine
    ni = (1 << (depth + 1)) - 1
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_din(din_weights(rng, E, ni), E, ni)
    return eng


def inputs(rng, tree, T):
    seq = rng.choice(tree["leaf_ids"], (T, L)).astype(np.int32)
    seq[rng.random((T, L)) < 0.15] = 0
    tgt = rng.choice(tree["leaf_ids"], T).astype(np.int32)
    tgt[::64] = 0
    return seq, tgt


def step_part(a, E):
    from dismember_amd import _native as N
    depth = a.depth
    tree, _ = two_level_tree(depth)
    neg = np.array([min((1 << l) - 1, 6) for l in range(depth + 1)], np.int32)
    per = int(sum(1 + neg[l] for l in range(1, depth + 1)))
    T = a.targets
    while T * per > MAX_ROWS:
        T //= 2
    rng = np.random.default_rng(7)
    eng = make_engine(E, depth, tree, rng)
    eng.train_init(lr=1e-3)
    seq, tgt = inputs(rng, tree, T)
    cap = T * per
    lib, o = N.lib(), N.SampleOpts(1, 0, 20, 1, 11)
    negp = neg.ctypes.data_as(N.i32p)
    bufs = dict(seq=T * L * 4, tgt=T * 4, codes=cap * 4, lab=cap * 4, rows=cap * L * 4, rmask=cap * 4, sc=T * L * 4, um=T * 4, off=(T + 1) * 8)
    d = {k: eng.dev_alloc(v) for k, v in bufs.items()}
    eng.h2d(d["seq"], seq); eng.h2d(d["tgt"], tgt)
    n, loss, out = C.c_int64(0), C.c_float(0), {}

    def chk(rc):
        if rc != 0:
            raise RuntimeError("rc %d: %s" % (rc, lib.dm_last_error(eng._h)))

    def sample_row():
        chk(lib.dm_tdm_sample_train_batch_dev(eng._h, d["seq"], d["tgt"], T, L, negp, neg.size, C.byref(o), d["codes"], d["rows"], d["rmask"], d["lab"], cap,
                                              C.byref(n)))

    def sample_csr():
        chk(lib.dm_tdm_sample_train_batch_csr_dev(eng._h, d["seq"], d["tgt"], T, L, negp, neg.size, C.byref(o), d["codes"], d["sc"], d["um"], d["off"], d["lab"],
                                                  cap, C.byref(n)))

    def fb_row():
        chk(lib.dm_train_forward_backward_dev(eng._h, d["codes"], d["rows"], d["rmask"], d["lab"], n.value, L, C.byref(loss)))
        out["row"] = loss.value

    def fb_csr():
        chk(lib.dm_train_forward_backward_csr_dev(eng._h, d["sc"], d["um"], d["off"], d["codes"], d["lab"], T, n.value, L, C.byref(loss)))
        out["csr"] = loss.value

    def both_row():
        sample_row(); fb_row()

    def both_csr():
        sample_csr(); fb_csr()
    sample_row(); sample_csr()
    B = n.value
    rounds = []
    for _ in range(a.rounds):
        r = dict(row_sampler_and_step_ms=spread(timed(both_row, eng.synchronize, 2, a.repeats)),
                 csr_sampler_and_step_ms=spread(timed(both_csr, eng.synchronize, 2, a.repeats)),
                 row_step_ms=spread(timed(fb_row, eng.synchronize, 2, a.repeats)),
                 csr_step_ms=spread(timed(fb_csr, eng.synchronize, 2, a.repeats)))
        r["row_over_csr_sampler_and_step"] = r["row_sampler_and_step_ms"]["median"] / r["csr_sampler_and_step_ms"]["median"]
        r["row_over_csr_step"] = r["row_step_ms"]["median"] / r["csr_step_ms"]["median"]
        rounds.append(r)
    kinds = {}
    os.environ["DM_TRAIN_TIME_LAUNCHES"] = "1"
    try:
        for name, call in (("csr", fb_csr),):
            eng.timing_reset()
            call(); eng.synchronize()
            kinds[name] = {k: dict(zip(("launches", "ms"), eng.timing_get_kind(v))) for k, v in KINDS.items() if eng.timing_get_kind(v)[0]}
    finally:
        del os.environ["DM_TRAIN_TIME_LAUNCHES"]
    for p in d.values():
        eng.dev_free(p)
    eng.close()
    return dict(requested=dict(targets=a.targets), ran=dict(targets=T, rows=B, row_bound=cap, rows_per_target=sorted({per, per - 1 - int(neg[depth])}), E=E, L=L,
                                                            depth=depth, slots_row=B * (L + 1), slots_csr=B + T * L),
                rounds=rounds, csr_faster_in_every_round=all(r["row_over_csr_sampler_and_step"] > 1 and r["row_over_csr_step"] > 1 for r in rounds),
                row_over_csr_sampler_and_step=spread([r["row_over_csr_sampler_and_step"] for r in rounds]),
                row_over_csr_step=spread([r["row_over_csr_step"] for r in rounds]), loss=out, kinds_ms_one_call=kinds)


def trainer_part(a, E):
    from dismember_amd.trainer import TDMTrainer
    depth = a.depth
    tree, _ = two_level_tree(depth)
    neg = np.array([min((1 << l) - 1, 6) for l in range(depth + 1)], np.int32)
    per = int(sum(1 + neg[l] for l in range(1, depth + 1)))
    T = a.targets
    while T * per > MAX_ROWS:
        T //= 2
    rng = np.random.default_rng(7)
    seq, tgt = inputs(rng, tree, T)
    engs = {g: make_engine(E, depth, tree, np.random.default_rng(7)) for g in (False, True)}
    trs = {g: TDMTrainer(engs[g], neg, 1, lr=1e-3, use_mask=True, din_grouped=g) for g in (False, True)}
    rounds = []
    for _ in range(a.rounds):
        r = {}
        for g, name in ((False, "row"), (True, "grouped")):
            r[name + "_ms"] = spread(timed(lambda: trs[g].step(seq, tgt), engs[g].synchronize, 2, a.repeats))
        r["row_over_grouped"] = r["row_ms"]["median"] / r["grouped_ms"]["median"]
        rounds.append(r)
    for e in engs.values():
        e.close()
    return dict(shape=dict(targets=T, E=E, L=L, depth=depth), rounds=rounds, grouped_faster_in_every_round=all(r["row_over_grouped"] > 1 for r in rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "din_train_csr_bench.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--targets", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=16)
    a = ap.parse_args()
    assert a.rounds >= 3 and a.depth >= 4
    res = dict(note="one box, one run; not measured: hardware counters, occupancy, achieved memory traffic, other batch shapes, L > 10, more than one GPU", rounds=a.rounds, repeats=a.repeats, warmup=2)
    for E in (16, 128):
        res["E%d" % E] = step_part(a, E)
    res["trainer_step"] = {"E%d" % E: trainer_part(a, E) for E in (16, 128)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
