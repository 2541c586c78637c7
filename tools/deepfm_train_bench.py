#!/usr/bin/env python3
"""DeepFM training step (dm_deepfm_train_forward_backward_dev + dm_deepfm_adam_step; csrc/dfm_train.hip.inc) on sampled rows.

    python tools/deepfm_train_bench.py [--out profiles/deepfm_train_bench.json] [--rows 16384]

Shape: 1 M-item tree of depth 20, E = 128, L = 10, about 16 384 rows drawn by the device sampler (dm_deepfm_sample_train_batch_dev) for
as many targets as that takes.  One box; 2 warm-up steps, then the median wall time of 7 steps (each ends in a stream synchronize), then
one more step under DM_DFM_TIME_LAUNCHES=1 for the per-kernel event times (kinds 70 .. 73; host work between the groups is in the step
time and in none of them) — tools/dr_train_bench.py's protocol.
Beside it a byte floor BY COUNT against the 9.5 TB/s at which this project's gathers saturate: X gathered twice by the
rows kernel and once by the l1.W product (non-padding slots x E x 4 bytes each), dX written once and read once, the sort of the B T
slots (per slot: 12 bytes written by the pairs kernel; per 8-bit pass 8 read by the histogram, 12 read and 12 written by the scatter;
12 read by the segment kernel), and Adam over the distinct rows of the batch (4 vectors read and written).  The ratio step / floor is
reported.  Context only: the DIN step (dm_train_forward_backward_dev + dm_adam_step) on the same rows of the same tree.
Not profiled: hardware counters, occupancy, achieved memory traffic, L2 hit rates of the fragment reads."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATHER_SATURATION_TBS = 9.5
KINDS = {"rows": 70, "l1W_l1b": 71, "emb_grad": 72, "adam": 73}


def median_step(step, sync, warmup, steps):
    for _ in range(warmup):
        step(); sync()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step(); sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfm_train_bench.json"))
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()

    from dismember_amd import Engine, _native as N, synth
    E, L, depth = a.embed, a.seq_len, a.depth
    T = L + 1
    num_index = (1 << (depth + 1)) - 1
    rng = np.random.default_rng(synth.SEED)
    tree = synth.make_tree(a.items, depth, rng)
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], depth)
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    n = num_index * E + T * T * E + 2 * T + 1
    w = np.empty(n, np.float32)
    w[:] = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)
    eng.load_weights_deepfm(w, E, L, num_index)
    del w
    neg = np.array([0, 1, 2, 3] + [4] * (depth - 3), np.int32)
    per = int(sum(1 + int(v) for v in neg[1:]))
    n_tgt = -(-a.rows // per)
    seqs = synth.make_users(tree["leaf_ids"], n_tgt, L, np.random.default_rng(synth.SEED + 1))
    tgt = np.random.default_rng(synth.SEED + 2).choice(tree["leaf_ids"], n_tgt).astype(np.int32)
    eng.deepfm_train_init(lr=1e-3)
    first_loss, (codes, hist, lab) = eng.deepfm_train_step_sampled(seqs, tgt, neg, 1, seed=1, return_rows=True)
    B = codes.size
    d_codes, d_seqs, d_lab, d_mask = eng.dev_alloc(B * 4), eng.dev_alloc(B * L * 4), eng.dev_alloc(B * 4), eng.dev_alloc(B * 4)
    eng.h2d(d_codes, codes); eng.h2d(d_seqs, hist); eng.h2d(d_lab, lab); eng.h2d(d_mask, np.zeros(B, np.uint32))
    losses = []

    def step():
        losses.append(eng.deepfm_train_forward_backward_dev(d_codes, d_seqs, d_lab, B, L))
        eng.deepfm_adam_step(1.0)
    ms, times = median_step(step, eng.synchronize, a.warmup, a.steps)
    os.environ["DM_DFM_TIME_LAUNCHES"] = "1"
    eng.timing_reset()
    step(); eng.synchronize()
    os.environ.pop("DM_DFM_TIME_LAUNCHES")
    kernels = {name: dict(zip(("launches", "ms"), eng.timing_get_kind(kind))) for name, kind in KINDS.items()}

    ids = np.concatenate([codes[:, None], hist], axis=1)
    slots, live, distinct = ids.size, int((ids >= 0).sum()), int(np.unique(ids[ids >= 0]).size)
    passes = -(-int(num_index).bit_length() // 8)
    floor_bytes = dict(x_gathers=3 * live * E * 4, dX=2 * slots * E * 4, sort=slots * (12 + passes * 32 + 12), adam=distinct * E * 4 * 8)
    floor_ms = sum(floor_bytes.values()) / (GATHER_SATURATION_TBS * 1e12) * 1e3
    res = dict(note="one box, one run", shape=dict(items=a.items, depth=depth, E=E, L=L, targets=n_tgt, rows=B), warmup=a.warmup, steps=a.steps,
               deepfm=dict(step_ms_median=ms, step_ms_all=times, kernels_ms=kernels, kernel_ms_sum=sum(k["ms"] for k in kernels.values()),
                           first_loss=first_loss, last_loss=losses[-1], slots=slots, non_padding_slots=live, distinct_rows=distinct,
                           floor_bytes=floor_bytes, floor_ms_at_gather_saturation=floor_ms, gather_saturation_TB_per_s=GATHER_SATURATION_TBS,
                           step_over_floor=ms / floor_ms),
               not_profiled="hardware counters, occupancy, achieved memory traffic, L2 hit rates of the fragment reads; the per-kernel "
                            "times are event pairs of one extra step")

    # ---- context only: the DIN step on the same rows (nothing masked)
    eng.load_weights_din_synthetic(E, num_index, synth.SEED)
    eng.train_init(lr=1e-3)
    lf = C.c_float(0)

    def din_step():
        eng._chk(N.lib().dm_train_forward_backward_dev(eng._h, d_codes, d_seqs, d_mask, d_lab, B, L, C.byref(lf)))
        eng.adam_step(1.0)
    din_ms, din_times = median_step(din_step, eng.synchronize, a.warmup, a.steps)
    res["din_same_rows_context_only"] = dict(step_ms_median=din_ms, step_ms_all=din_times, last_loss=float(lf.value))
    for p in (d_codes, d_seqs, d_lab, d_mask):
        eng.dev_free(p)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
