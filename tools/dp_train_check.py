"""Data-parallel training check with the library's own gradient exchange (dm_train_sync_gradients =
LocalOptimizer.syncGradients, tdm/.../optim/LocalOptimizer.scala:164-187): W worker processes share ONE GPU over the
host transport (RCCL refuses two ranks per device; same entry point and kernels, only the wire differs).  After three
TDMTrainer steps (device-side negative sampling, sync, Adam) every replica must hold bit-identical weights, and they
must equal a single worker that sees all W slices with the gradient formed in rank order.
Prints one JSON line; the driver-side copy is kept as profiles/<round>_dp_train_check.json.
  usage: python tools/dp_train_check.py [workers] [--deepfm | --dr]
--deepfm: the same check through the DeepFM trainer (dm_deepfm_train_sync_gradients).  A DeepFM step REPLACES the
gradient, so a single worker cannot accumulate the W slices; instead every worker also hands back its local and its exchanged gradient
of every step, and the exchanged one must equal the float32 numpy sum of the local ones in rank order, bit for bit.
--dr: the Deep-Retrieval layer model through DRTrainer(comm=...) (dm_dr_train_sync_gradients), fp64: every worker gets
the same global batch, trains its slice, and hands back local and exchanged gradients of every step (the same bit-for-bit criterion, in
float64) and its weights and moments."""
import json, multiprocessing as mp, os, socket, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEG = np.arange(13, dtype=np.int32)
STEPS = 3


def data(world):
    from dismember_amd import synth
    t = np.load(os.path.join(GOLDEN, "tdm_tree.npz"))
    rng = np.random.default_rng(0)
    seqs = synth.make_users(t["leaf_ids"], 32 * world, 10, rng)
    tgt = rng.choice(t["leaf_ids"], 32 * world).astype(np.int32)
    return t, seqs, tgt


def deepfm_weights():
    rng = np.random.default_rng(5)
    n = 8191 * 16 + 11 * 11 * 16 + 2 * 11 + 1
    return (rng.standard_normal(n) * 0.05).astype(np.float32)


def engine(t, deepfm=False):
    from dismember_amd import Engine
    e = Engine(0)
    e.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"])); e.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    if deepfm:
        e.load_weights_deepfm(deepfm_weights(), 16, 10, 8191)
        return e
    e.load_weights_din(np.load(os.path.join(GOLDEN, "din_f32.npy")) * np.float32(0.3), 16, 8191)
    return e


def deepfm_worker(rank, world, port, q):
    """TDMTrainer.step taken apart so that the gradients can be read: local step, exchange, Adam"""
    from dismember_amd import sharding
    from dismember_amd.comm import Comm
    from dismember_amd.trainer import TDMTrainer
    t, seqs, tgt = data(world)
    eng = engine(t, deepfm=True)
    comm = Comm(world, rank, "127.0.0.1", port, transport="host")
    tr = TDMTrainer(eng, NEG, lr=1e-3, comm=comm, seed=77, sampler="device")
    lo, hi = sharding.shard_range(len(seqs), rank, world)
    losses, grads = [], []
    for it in range(STEPS):
        loss = eng.deepfm_train_step_sampled(seqs[lo:hi], tgt[lo:hi], NEG, 1, seed=77 + 1000003 * it + rank)
        local = eng.deepfm_train_download("grad")
        eng.deepfm_train_sync_gradients()
        grads.append((local, eng.deepfm_train_download("grad")))
        eng.deepfm_adam_step(1.0 / world)
        losses.append(comm.allreduce(float(loss)) / world)
    # ... and the trainer's own step on top, so that its wiring runs too
    losses.append(float(tr.step(seqs[lo:hi], tgt[lo:hi])))
    q.put((rank, losses, eng.deepfm_train_download("weights"), grads))
    comm.barrier()
    eng.close(); comm.close()


def dr_problem():
    from dismember_amd import synth
    K, D, L, E, NI, J, B = 32, 3, 8, 32, 2000, 2, 96
    rng = np.random.default_rng(9)
    weights = synth.make_dr_model(NI, K, D, L, E, rng)
    item_paths = synth.make_dr_paths(NI, K, D, J, rng)
    seqs = rng.integers(0, NI, (STEPS + 1, B, L)).astype(np.int32)
    seqs[rng.random(seqs.shape) < 0.1] = -1
    return (E, L, K, D, NI), weights, item_paths, seqs, rng.integers(0, NI, (STEPS + 1, B))


def dr_worker(rank, world, port, q):
    """DRTrainer's parallel layer step taken apart so that the gradients can be read, then the trainer's own step"""
    from dismember_amd import Engine
    from dismember_amd.comm import Comm
    from dismember_amd.dr_train import DRTrainer, expand_batch, layer_slices
    (E, L, K, D, NI), weights, item_paths, seqs, targets = dr_problem()
    eng = Engine(0)
    eng.dr_load_model(weights, E, L, K, D, NI, dtype=np.float64)
    comm = Comm(world, rank, "127.0.0.1", port, transport="host")
    tr = DRTrainer(eng, item_paths, lr=1e-3, comm=comm)
    losses, grads = [], []
    for it in range(STEPS):
        slices, P = layer_slices(len(targets[it]), world)
        lo, n = slices[rank]
        loss = np.zeros(D)
        if n:
            loss = eng.dr_train_forward_backward(*expand_batch(seqs[it][lo:lo + n], targets[it][lo:lo + n], item_paths))
        local = eng.dr_train_download("grad")
        eng.dr_train_sync_gradients()
        grads.append((local, eng.dr_train_download("grad")))
        eng.dr_adam_step(1.0 / P)
        losses.append((comm.allreduce(loss) / P).tolist())
    losses.append(np.asarray(tr.step(seqs[STEPS], targets[STEPS])).tolist())
    q.put((rank, losses, np.concatenate([eng.dr_train_download(k) for k in ("weights", "s", "r")]), grads))
    comm.barrier()
    eng.close(); comm.close()


def worker(rank, world, port, q):
    from dismember_amd import sharding
    from dismember_amd.comm import Comm
    from dismember_amd.trainer import TDMTrainer
    t, seqs, tgt = data(world)
    eng = engine(t)
    comm = Comm(world, rank, "127.0.0.1", port, transport="host")
    tr = TDMTrainer(eng, NEG, lr=1e-3, comm=comm, seed=77, sampler="device")
    lo, hi = sharding.shard_range(len(seqs), rank, world)
    losses = [float(tr.step(seqs[lo:hi], tgt[lo:hi])) for _ in range(STEPS)]
    q.put((rank, losses, eng.train_download("weights")))
    comm.barrier()
    eng.close(); comm.close()


def main():
    args = [v for v in sys.argv[1:] if v not in ("--deepfm", "--dr")]
    deepfm, dr = "--deepfm" in sys.argv[1:], "--dr" in sys.argv[1:]
    world = int(args[0]) if args else 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=dr_worker if dr else deepfm_worker if deepfm else worker, args=(r, world, port, q)) for r in range(world)]
    try:
        [p.start() for p in procs]
        out = sorted((q.get(timeout=600) for _ in range(world)), key=lambda x: x[0])
        [p.join(120) for p in procs]
    finally:
        for p in procs:                     # a rank that failed leaves its peers inside a collective: end them
            if p.is_alive():
                p.terminate()
    w0 = out[0][2]
    if deepfm or dr:
        exact = True
        for it in range(STEPS):
            want = np.zeros_like(out[0][3][it][0])
            for r in range(world):
                want = want + out[r][3][it][0]          # the model's dtype, rank order
            exact = exact and all(np.array_equal(out[r][3][it][1], want) for r in range(world))
    if dr:
        from dismember_amd.dr_train import pack_params
        print(json.dumps({"workers": world, "steps": STEPS + 1, "model": "deep-retrieval layer model, fp64", "transport": "host (W processes on one GPU)",
                          "replicas_bit_identical": bool(all(np.array_equal(w0, o[2]) for o in out[1:])),
                          "exchange_equals_rank_ordered_numpy_sum": bool(exact), "losses_per_worker": [o[1] for o in out],
                          "weights_changed": bool(not np.array_equal(w0[:w0.size // 3], pack_params(dr_problem()[1]))),
                          "exit_codes": [p.exitcode for p in procs]}))
        return
    if deepfm:
        print(json.dumps({"workers": world, "steps": STEPS + 1, "scorer": "deepfm", "transport": "host (W processes on one GPU)",
                          "replicas_bit_identical": bool(all(np.array_equal(w0, o[2]) for o in out[1:])),
                          "exchange_equals_rank_ordered_numpy_sum": bool(exact), "losses_per_worker": [o[1] for o in out],
                          "weights_changed": bool(not np.array_equal(w0, deepfm_weights())), "exit_codes": [p.exitcode for p in procs]}))
        return
    rec = {"workers": world, "steps": STEPS, "transport": "host (W processes on one GPU)",
           "replicas_bit_identical": bool(all(np.array_equal(w0, o[2]) for o in out[1:])),
           "losses_per_worker": [o[1] for o in out],
           "weights_changed": bool(not np.array_equal(w0, np.load(os.path.join(GOLDEN, "din_f32.npy")) * np.float32(0.3))),
           "exit_codes": [p.exitcode for p in procs]}
    # single worker holding every slice: the same sampled rows (same seeds), gradients summed in rank order, one Adam step
    from dismember_amd import sharding
    t, seqs, tgt = data(world)
    ref = engine(t)
    ref.train_init(lr=1e-3)
    for it in range(STEPS):
        for r in range(world):
            lo, hi = sharding.shard_range(len(seqs), r, world)
            ref.train_step_sampled(seqs[lo:hi], tgt[lo:hi], NEG, 1, seed=77 + 1000003 * it + r, use_mask=True)   # gradients accumulate until the Adam step
        ref.adam_step(1.0 / world)
    wr = ref.train_download("weights")
    rec["max_abs_diff_vs_single_worker"] = float(np.abs(wr.astype(np.float64) - w0).max())
    rec["max_abs_weight_update"] = float(np.abs(w0.astype(np.float64) - np.load(os.path.join(GOLDEN, "din_f32.npy")) * np.float32(0.3)).max())
    rec["note_single_worker"] = ("the single worker adds worker r's rows onto the running gradient one by one, a worker sums its own rows first: "
                                 "same terms, different fp32 association, so agreement is to rounding, not bit for bit")
    ref.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
