#!/usr/bin/env python3
"""Deep-Retrieval gradient exchange (dm_dr_train_sync_gradients; csrc/dr_train_sync.hip.inc) at the training bench's shape.

    python tools/dr_train_sync_bench.py [--out profiles/dr_train_sync_bench.json] [--rows 16384] [--workers 2]

Shape: tools/dr_train_bench.py's — K = 1000, D = 3, L = 10, E = 128, 1 M items; every rank trains its own --rows / W rows of one batch.
W worker processes share ONE GPU over the host transport (RCCL refuses two ranks per device): the wire is TCP through host memory and
says nothing about xGMI, so NO exchange time is reported.  What is reported, per dtype and rank, from steps under DM_DR_TIME_LAUNCHES=1
after 2 warm-up steps: the event times of the two device halves — kind 79 (unique rows, compaction, block pack) and kind 93 (tails copied
and added, own rows cleared, every rank's rows added in rank order, bookkeeping) — the rows and bytes a rank sends and receives and the
waits on the stream per exchange.  Beside them, for scale, the single-rank step (forward/backward + Adam, no communicator) on the whole
batch in the same run, median wall time.
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
K, D, L, E = 1000, 3, 10, 128
DTYPES = {"float64": np.float64, "float32": np.float32}


def setup(a, dtype):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.dr_load_model_synthetic(E, L, K, D, a.items, seed=3, rerank=False, dtype=DTYPES[dtype])      # the same weights on every rank
    eng.dr_train_init(lr=1e-3)
    rng = np.random.default_rng(1)
    seq = rng.integers(0, a.items, size=(a.rows, L)).astype(np.int32)
    seq[rng.random((a.rows, L)) < 0.1] = -1
    return eng, seq, rng.integers(0, K, size=(a.rows, D)).astype(np.int32)


def worker(rank, world, port, q, a):
    try:
        from dismember_amd.comm import Comm
        from dismember_amd.dr_train import layer_slices
        comm = Comm(world, rank, "127.0.0.1", port, transport="host")
        res = {}
        for dtype in DTYPES:
            eng, seq, paths = setup(a, dtype)
            eng.attach_comm(comm)
            lo, n = layer_slices(a.rows, world)[0][rank]
            os.environ["DM_DR_TIME_LAUNCHES"] = "1"
            per_step = []
            for it in range(WARMUP + STEPS):
                eng.dr_train_forward_backward(seq[lo:lo + n], paths[lo:lo + n])
                eng.timing_reset()
                eng.dr_train_sync_gradients()
                pack, rebuild = eng.timing_get_kind(79), eng.timing_get_kind(93)
                eng.dr_adam_step(1.0 / world)
                if it >= WARMUP:
                    per_step.append(dict(pack_launches=pack[0], pack_ms=pack[1], rebuild_launches=rebuild[0], rebuild_ms=rebuild[1], **eng.train_sync_stats()))
            del os.environ["DM_DR_TIME_LAUNCHES"]
            crc = int(np.frombuffer(eng.dr_train_download("weights").tobytes(), np.uint32).sum(dtype=np.uint64))
            res[dtype] = dict(per_step=per_step, weights_checksum=crc)
            eng.attach_comm(None)
            eng.close()
        q.put((rank, "ok", res))
        comm.barrier()
        comm.close()
    except BaseException:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise


def single_rank_step(a, dtype):
    """forward/backward + Adam without a communicator on the whole batch: median wall milliseconds"""
    eng, seq, paths = setup(a, dtype)
    d_seq, d_paths = eng.dev_alloc(seq.nbytes), eng.dev_alloc(paths.nbytes)
    eng.h2d(d_seq, seq); eng.h2d(d_paths, paths)
    times = []
    for it in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        eng.dr_train_forward_backward_dev(d_seq, d_paths, a.rows)
        eng.dr_adam_step(1.0)
        eng.synchronize()
        if it >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
    for p in (d_seq, d_paths):
        eng.dev_free(p)
    eng.close()
    return dict(rows=int(a.rows), step_ms_median=float(np.median(times)), step_ms_all=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dr_train_sync_bench.json"))
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--items", type=int, default=1_000_000)
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
    res = dict(note="one box, one run; W processes on ONE GPU over the host transport (TCP through host memory): no exchange time is reported, "
                    "the wire says nothing about xGMI.  RCCL with more than one rank has not executed anywhere.",
               shape=dict(items=a.items, K=K, D=D, L=L, E=E, rows_per_batch=a.rows, workers=world), warmup=WARMUP, steps=STEPS, dtypes={},
               not_measured="the exchange's wall time on a real multi-GPU wire (xGMI, RCCL), hardware counters, other shapes; the event times are "
                            "pairs around launches on one GPU that W processes share")
    for dtype in DTYPES:
        med = lambda r, k: float(np.median([s[k] for s in out[r][dtype]["per_step"]]))
        last = lambda r: out[r][dtype]["per_step"][-1]
        res["dtypes"][dtype] = dict(
            replicas_bit_identical=len({out[r][dtype]["weights_checksum"] for r in out}) == 1,
            ranks=[dict(rank=r, pack_ms_median=med(r, "pack_ms"), rebuild_ms_median=med(r, "rebuild_ms"), pack_launch_groups=last(r)["pack_launches"],
                        rebuild_launch_groups=last(r)["rebuild_launches"], rows_mine=last(r)["rows_mine"], rows_total=last(r)["rows_total"],
                        bytes_sent=last(r)["bytes_sent"], bytes_recv=last(r)["bytes_recv"], host_syncs_per_exchange=last(r)["host_syncs"],
                        per_step=out[r][dtype]["per_step"]) for r in sorted(out)],
            single_rank_step_for_scale=single_rank_step(a, dtype))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    brief = {dt: {"replicas_bit_identical": v["replicas_bit_identical"], "single_rank_step_ms": v["single_rank_step_for_scale"]["step_ms_median"],
                  "ranks": [{k: x for k, x in r.items() if k != "per_step"} for r in v["ranks"]]} for dt, v in res["dtypes"].items()}
    print(json.dumps(brief, sort_keys=True))


if __name__ == "__main__":
    main()
