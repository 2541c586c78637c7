#!/usr/bin/env python3
"""DeepFM gradient exchange (dm_deepfm_train_sync_gradients; csrc/dfm_train_sync.hip.inc) at the training bench's shape.

    python tools/deepfm_train_sync_bench.py [--out profiles/deepfm_train_sync_bench.json] [--rows 16384] [--workers 2]

Shape: tools/deepfm_train_bench.py's — 1 M-item tree of depth 20, E = 128, L = 10, about 16 384 rows per rank drawn by the device
sampler for the rank's own targets.  W worker processes share ONE GPU over the host transport (RCCL refuses two ranks per device): the
wire is TCP through host memory and says nothing about xGMI, so NO exchange time is reported.  What is reported, per rank, from steps
under DM_DFM_TIME_LAUNCHES=1 after 2 warm-up steps: the event times of the two device halves — kind 77 (unique rows, compaction, block
pack) and kind 78 (tails, own rows cleared, every rank's rows added in rank order, bookkeeping) — the bytes a rank sends and receives,
its rows, and the host synchronisations per exchange.  Beside them, for scale, the single-rank step (forward/backward + Adam, no
communicator: the code of the commit before the exchange existed) on rank 0's rows, median wall time.
RCCL with more than one rank has not executed anywhere: a one-GPU box cannot hold two RCCL ranks."""
import argparse
import json
import multiprocessing as mp
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, STEPS = 2, 5


def setup(a, rank):
    from dismember_amd import Engine, synth
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
    w[:] = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)      # the same weights on every rank
    eng.load_weights_deepfm(w, E, L, num_index)
    del w
    neg = np.array([0, 1, 2, 3] + [4] * (depth - 3), np.int32)
    per = int(sum(1 + int(v) for v in neg[1:]))
    n_tgt = -(-a.rows // per)
    seqs = synth.make_users(tree["leaf_ids"], n_tgt, L, np.random.default_rng(synth.SEED + 1 + 10 * rank))
    tgt = np.random.default_rng(synth.SEED + 2 + 10 * rank).choice(tree["leaf_ids"], n_tgt).astype(np.int32)
    return eng, neg, seqs, tgt


def worker(rank, world, port, q, a):
    try:
        from dismember_amd.comm import Comm
        eng, neg, seqs, tgt = setup(a, rank)
        eng.deepfm_train_init(lr=1e-3)
        comm = Comm(world, rank, "127.0.0.1", port, transport="host")
        eng.attach_comm(comm)
        os.environ["DM_DFM_TIME_LAUNCHES"] = "1"
        per_step = []
        for it in range(WARMUP + STEPS):
            eng.deepfm_train_step_sampled(seqs, tgt, neg, 1, seed=1 + it)
            eng.timing_reset()
            eng.deepfm_train_sync_gradients()
            pack, rebuild = eng.timing_get_kind(77), eng.timing_get_kind(78)
            eng.deepfm_adam_step(1.0 / world)
            if it >= WARMUP:
                per_step.append(dict(pack_launches=pack[0], pack_ms=pack[1], rebuild_launches=rebuild[0], rebuild_ms=rebuild[1], **eng.train_sync_stats()))
        weights_crc = int(np.frombuffer(eng.deepfm_train_download("weights").tobytes(), np.uint32).sum(dtype=np.uint64))
        q.put((rank, "ok", dict(per_step=per_step, weights_checksum=weights_crc)))
        comm.barrier()
        eng.attach_comm(None)
        eng.close(); comm.close()
    except BaseException:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise


def single_rank_step(a):
    """forward/backward + Adam without a communicator on rank 0's rows: median wall milliseconds"""
    eng, neg, seqs, tgt = setup(a, 0)
    eng.deepfm_train_init(lr=1e-3)
    _, (codes, hist, lab) = eng.deepfm_train_step_sampled(seqs, tgt, neg, 1, seed=1, return_rows=True)
    B, L = codes.size, hist.shape[1]
    d_codes, d_seqs, d_lab = eng.dev_alloc(B * 4), eng.dev_alloc(B * L * 4), eng.dev_alloc(B * 4)
    eng.h2d(d_codes, codes); eng.h2d(d_seqs, hist); eng.h2d(d_lab, lab)
    times = []
    for it in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        eng.deepfm_train_forward_backward_dev(d_codes, d_seqs, d_lab, B, L)
        eng.deepfm_adam_step(1.0)
        eng.synchronize()
        if it >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
    for p in (d_codes, d_seqs, d_lab):
        eng.dev_free(p)
    eng.close()
    return dict(rows=int(B), step_ms_median=float(np.median(times)), step_ms_all=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfm_train_sync_bench.json"))
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--workers", type=int, default=2)
    a = ap.parse_args()
    world = a.workers
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q, a)) for r in range(world)]
    out = {}
    try:
        [p.start() for p in procs]
        for _ in range(world):
            rank, status, res = q.get(timeout=900)
            if status != "ok":
                raise SystemExit("rank %d failed:\n%s" % (rank, res))
            out[rank] = res
        [p.join(120) for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    med = lambda r, k: float(np.median([s[k] for s in out[r]["per_step"]]))
    res = dict(note="one box, one run; W processes on ONE GPU over the host transport (TCP through host memory): no exchange time is reported, "
                    "the wire says nothing about xGMI.  RCCL with more than one rank has not executed anywhere.",
               shape=dict(items=a.items, depth=a.depth, E=a.embed, L=a.seq_len, rows_per_rank_requested=a.rows, workers=world), warmup=WARMUP, steps=STEPS,
               replicas_bit_identical=len({out[r]["weights_checksum"] for r in out}) == 1,
               ranks=[dict(rank=r, pack_ms_median=med(r, "pack_ms"), rebuild_ms_median=med(r, "rebuild_ms"), pack_launch_groups=out[r]["per_step"][-1]["pack_launches"],
                           rebuild_launch_groups=out[r]["per_step"][-1]["rebuild_launches"], rows_mine=out[r]["per_step"][-1]["rows_mine"],
                           rows_total=out[r]["per_step"][-1]["rows_total"], bytes_sent=out[r]["per_step"][-1]["bytes_sent"],
                           bytes_recv=out[r]["per_step"][-1]["bytes_recv"], host_syncs_per_exchange=out[r]["per_step"][-1]["host_syncs"],
                           per_step=out[r]["per_step"]) for r in sorted(out)],
               single_rank_step_for_scale=single_rank_step(a),
               not_measured="the exchange's wall time on a real multi-GPU wire (xGMI, RCCL), hardware counters; the event times are pairs around "
                            "launches on one GPU that W processes share")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "ranks"} | {"ranks": [{k: v for k, v in r.items() if k != "per_step"} for r in res["ranks"]]}, sort_keys=True))


if __name__ == "__main__":
    main()
