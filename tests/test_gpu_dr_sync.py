"""The Deep-Retrieval gradient exchange behind the C ABI (dm_dr_train_sync_gradients = LocalOptimizer.syncGradients,
deep-retrieval/src/main/scala/com/mass/dr/optim/LocalOptimizer.scala:167-194, minus the division) on real engines:
dismember_amd/csrc/dr_train_sync.hip.inc, and DRTrainer(comm=...) on top of it.

A GPU box has ONE device and RCCL refuses two ranks per device, so the multi-worker protocol runs as W spawned processes sharing the GPU
over the library's host transport (same entry point, same kernels; only the wire differs), as tests/test_gpu_deepfm_sync.py does.  A
failing rank reports its traceback and ends the test: nobody waits longer than the queue's timeout, and stragglers are terminated.  Every
gradient comparison is np.array_equal against the numpy sum in rank order and in the model's dtype (tests/dr_sync_ref.py): exact IEEE
adds in a fixed order.  All cases of one world size share one set of worker processes."""
import ctypes as C
import functools
import multiprocessing as mp
import os
import socket
import traceback

import numpy as np
import pytest

import dr_sync_ref as S
import dr_train_ref as R
from dismember_amd.dr_train import expand_batch, layer_slices, pack_params, param_sections, split_params

pytestmark = pytest.mark.gpu
EV_PACK, EV_SUM = 79, 93
ERR_STATE = -3
LR = 1e-2
STATE = ("weights", "s", "r")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def live_allocs():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


def _engine(c, dtype=None, dims=None, train=True):
    from dismember_amd import Engine
    dims = dims or c["dims"]
    E, L, K, D, NI = dims
    eng = Engine(0)
    eng.dr_load_model(split_params(c["w"], *dims), E, L, K, D, NI, dtype=S.NP[dtype or c["dtype"]])
    if train:
        eng.dr_train_init(lr=LR)
    return eng


def _fb(eng, batch):
    """the local step; an idle rank runs nothing"""
    seq, paths = batch
    return eng.dr_train_forward_backward(seq, paths) if len(seq) else None


def _refused(call):
    from dismember_amd import DismemberError
    try:
        call()
    except DismemberError as e:
        return e.code, str(e)
    return 0, ""


def _state(eng):
    return tuple(eng.dr_train_download(k) for k in STATE)


# --------------------------------------------------------------------------- what a rank runs (module level: spawn imports this file)
def _case_run(rank, comm, name):
    c = S.case(name)
    os.environ.update(c["env"])
    try:
        eng = _engine(c)
        eng.attach_comm(comm)
        _fb(eng, c["batches"][rank])
        out = dict(local=eng.dr_train_download("grad"))
        eng.dr_train_sync_gradients()
        out["summed"], out["stats"] = eng.dr_train_download("grad"), eng.train_sync_stats()
        eng.dr_adam_step(1.0 / c["P"])
        out["state"] = _state(eng)
        out["cleared"] = not eng.dr_train_download("grad").any()
        eng.close()
    finally:
        for k in c["env"]:
            del os.environ[k]
    return out


def _sc_cases(rank, world, comm, _):
    return {name: _case_run(rank, comm, name) for name in S.CASES if S.case(name)["W"] == world}


def _sc_protocol(rank, world, comm, name):
    """second exchange, launch kinds, allocations; then two steps with disjoint item rows"""
    c = S.case(name)
    batch = c["batches"][rank]
    base = live_allocs()
    eng = _engine(c)
    _fb(eng, batch)
    eng.dr_train_free()
    loaded = live_allocs()                                          # the model and what a step derives from it, no training state
    eng.dr_train_init(lr=LR)
    eng.attach_comm(comm)
    _fb(eng, batch)
    eng.timing_reset()
    eng.dr_train_sync_gradients()
    silent = (eng.timing_get_kind(EV_PACK)[0], eng.timing_get_kind(EV_SUM)[0])
    summed = eng.dr_train_download("grad")
    again = _refused(eng.dr_train_sync_gradients)                   # no step in between: refused on every rank, before any collective
    still = eng.dr_train_download("grad")
    eng.dr_adam_step(1.0 / world)
    w1 = eng.dr_train_download("weights")
    # step 2: the rows received in step 1 are in `prev` (this step's zeroGradParameters clears them) — the gradient is exactly the one a
    # fresh engine loaded with w1 computes on this rank's batch, zero on the other rank's item rows
    os.environ["DM_DR_TIME_LAUNCHES"] = "1"
    try:
        _fb(eng, batch)
        g2 = eng.dr_train_download("grad")
        before = live_allocs()
        eng.timing_reset()
        eng.dr_train_sync_gradients()                               # (a good call after the refusal, and a warm one)
        warm = live_allocs() == before
        timed = (eng.timing_get_kind(EV_PACK)[0], eng.timing_get_kind(EV_SUM)[0])
    finally:
        del os.environ["DM_DR_TIME_LAUNCHES"]
    summed2 = eng.dr_train_download("grad")
    eng.dr_adam_step(1.0 / world)
    w2 = eng.dr_train_download("weights")
    fresh = _engine(dict(c, w=w1.astype(np.float64)))
    _fb(fresh, batch)
    g2_fresh = fresh.dr_train_download("grad")
    fresh.close()
    eng.attach_comm(None)
    eng.dr_train_free()
    freed = live_allocs() == loaded
    eng.close()
    return dict(summed=summed, again=again, still=still, w1=w1, w2=w2, g2=g2, g2_fresh=g2_fresh, summed2=summed2, silent=silent, timed=timed, warm=warm,
                freed=freed, closed=live_allocs() == base)


def _sc_mismatch(rank, world, comm, what):
    from dismember_amd.comm import Comm
    c = S.case("shared_w2_f64")
    E, L, K, D, NI = c["dims"]
    if what == "dtype":                                             # rank 1 holds an f32 model
        eng = _engine(c, dtype="f32" if rank else "f64")
    else:                                                           # rank 1 has 8 items more
        dims = (E, L, K, D, NI + 8 * rank)
        n = param_sections(*dims)["b%d" % (D - 1)][1]
        eng = _engine(dict(c, w=np.random.default_rng(3).standard_normal(n) * 0.3), dims=dims)
    eng.attach_comm(comm)
    _fb(eng, c["batches"][rank])
    local = eng.dr_train_download("grad")
    out = dict(refusal=_refused(eng.dr_train_sync_gradients), untouched=eng.dr_train_download("grad").tobytes() == local.tobytes())
    one = Comm(1, 0, "127.0.0.1", _free_port(), transport="host")  # the handle is usable: a good call on a communicator of one, a step
    eng.attach_comm(one)
    eng.dr_train_sync_gradients()
    out["after"] = (eng.train_sync_stats()["nranks"], eng.dr_train_download("grad").tobytes() == local.tobytes())
    eng.dr_adam_step(1.0)
    out["stepped"] = not eng.dr_train_download("grad").any()
    eng.attach_comm(None)
    one.close()
    eng.close()
    return out


def _problem():
    p = R.learning_problem()
    return p, pack_params(p["weights"])


def _trainer_engine(p):
    from dismember_amd import Engine
    E, L, K, D, NI = p["dims"]
    eng = Engine(0)
    eng.dr_load_model(p["weights"], E, L, K, D, NI, dtype=np.float64)
    return eng


def _sc_trainer(rank, world, comm, arg):
    from dismember_amd.dr_train import DRTrainer
    B, rerank = arg
    p, _ = _problem()
    seqs, targets = p["seqs"][:B], p["targets"][:B]
    kw = dict(rerank=True, num_sampled=8, seed=5) if rerank else {}
    eng = _trainer_engine(p)
    tr = DRTrainer(eng, p["item_paths"], lr=p["lr"], comm=comm, **kw)
    (lo, n), P = layer_slices(B, world)[0][rank], layer_slices(B, world)[1]
    local = eng.dr_train_forward_backward(*expand_batch(seqs[lo:lo + n], targets[lo:lo + n], p["item_paths"])) if n else None
    steps = [tr.step(seqs, targets) for _ in range(3)]
    out = dict(local=local, P=P, losses=[s[0] if rerank else s for s in steps], state=_state(eng), sync_calls=tr.sync_calls, sync_s=tr.sync_s,
               stats=eng.train_sync_stats())
    if rerank:
        out["rr_losses"] = [s[1] for s in steps]
        out["rr"] = tuple(eng.dr_rerank_download(v, k) for v in ("graph", "softmax") for k in STATE)
    if rank == 0:
        # the handle that trained data-parallel serves what a fresh handle loaded from its downloaded weights serves
        fresh = _trainer_engine(dict(p, weights=dict(p["weights"], **tr.weights())))
        out["search"] = tuple(b"".join(a.tobytes() for a in e.dr_beam_search(p["seqs"][:16], 4)) for e in (eng, fresh))
        out["found"] = int(eng.dr_beam_search(p["seqs"][:16], 4)[2].sum())
        fresh.close()
        if rerank:                                                  # the rerank half is unsplit: a single worker's bytes
            solo_eng = _trainer_engine(p)
            solo = DRTrainer(solo_eng, p["item_paths"], lr=p["lr"], **kw)
            out["solo_rr_losses"] = [solo.step(seqs, targets)[1] for _ in range(3)]
            out["solo_rr"] = tuple(solo_eng.dr_rerank_download(v, k) for v in ("graph", "softmax") for k in STATE)
            solo_eng.close()
    eng.attach_comm(None)
    eng.close()
    return out


def _sc_seeds(rank, world, comm, _):
    from dismember_amd.dr_train import DRTrainer
    p, _ = _problem()
    eng = _trainer_engine(p)
    try:
        DRTrainer(eng, p["item_paths"], lr=p["lr"], comm=comm, rerank=True, num_sampled=8, seed=5 + rank)
        return "no error"
    except ValueError as e:
        return str(e)
    finally:
        eng.close()


SCENARIOS = {"cases": _sc_cases, "protocol": _sc_protocol, "mismatch": _sc_mismatch, "trainer": _sc_trainer, "seeds": _sc_seeds}


def _worker(rank, world, port, q, scenario, arg):
    try:
        from dismember_amd.comm import Comm
        comm = Comm(world, rank, "127.0.0.1", port, transport="host")
        out = SCENARIOS[scenario](rank, world, comm, arg)
        q.put((rank, "ok", out))
        comm.barrier()
        comm.close()
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
        raise


def _run_ranks(world, scenario, arg=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, scenario, arg)) for r in range(world)]
    try:
        [p.start() for p in procs]
        out = {}
        for _ in range(world):
            rank, status, res = q.get(timeout=120)
            assert status == "ok", "rank %d failed:\n%s" % (rank, res)
            out[rank] = res
        [p.join(30) for p in procs]
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        return [out[r] for r in range(world)]
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(5)


@functools.lru_cache(maxsize=None)
def _run_once(world, scenario, arg=None):
    """a run several tests read: made once"""
    return _run_ranks(world, scenario, arg)


# --------------------------------------------------------------------------- the exchange, case by case
@pytest.mark.parametrize("name", S.CASES)
def test_exchange_equals_the_rank_ordered_sum(name):
    c = S.case(name)
    W, dims, dt, T = c["W"], c["dims"], c["dtype"], S.NP[c["dtype"]]
    out = [o[name] for o in _run_once(W, "cases")]
    E, NR = dims[0], S.num_rows(dims)
    want = S.dense_sum([o["local"] for o in out])
    rows = [S.batch_rows(seq, paths, dims) for seq, paths in c["batches"]]
    union, acc, tail = S.exchange([S.split(o["local"], rows[r], dims) for r, o in enumerate(out)], dims, dt)
    assert want.dtype == T and np.array_equal(S.assemble(union, acc, tail, dims), want)      # (no gradient outside the batch's rows)
    for r, o in enumerate(out):
        assert o["local"].dtype == T and o["summed"].dtype == T
        assert o["local"].any() == bool(len(c["batches"][r][0]))                             # an idle rank holds zeros
        assert np.array_equal(o["summed"], want), r
        st = o["stats"]
        assert (st["nranks"], st["transport"], st["rows_mine"], st["rows_total"]) == (W, "host", rows[r].size, sum(x.size for x in rows)), st
        assert st["bytes_sent"] == S.block_bytes(rows[r].size, dims, dt) and st["bytes_recv"] == sum(S.block_bytes(x.size, dims, dt) for x in rows), st
        assert 1 <= st["host_syncs"] <= 5, st                        # row count, staging down and up, end; one more when the key list grows
    if W == 3 and name.startswith("shared"):
        assert not np.array_equal(S.dense_sum([o["local"] for o in out][::-1]), want)        # the order is visible in these bytes
    # ---- after dr_adam_step(1 / P): identical replicas, and the criterion of test_gpu_dr_train.py::test_adam_wiring against the sum
    gs = T(np.float32(1.0 / c["P"]))                                 # (grad_scale crosses the ABI as a float)
    sg = gs * want
    touched = np.zeros(NR, bool)
    touched[union] = True
    w0 = c["w"].astype(T)
    emb = lambda v: v[:NR * E].reshape(NR, E)
    for o in out:
        w1, s1, r1 = o["state"]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], out[0]["state"]))
        assert o["cleared"]
        assert emb(w0)[~touched].tobytes() == emb(w1)[~touched].tobytes()
        live = np.abs(emb(want)).sum(1) > 0                          # (K = 16: no all-zero gradient rows among the touched ones in practice)
        assert (emb(w0)[live] != emb(w1)[live]).any(axis=1).all() and live.sum() > 0
        for got, exp in ((s1, T(1 - 0.9) * sg), (r1, T(1 - 0.999) * (sg * sg))):
            assert (np.abs(got - exp) <= 2 * np.spacing(np.abs(exp))).all()
    if name in S.TWIN:                                               # DM_ADAM_DENSE=1 after an exchange: the bytes of the rows path
        assert 4 * union.size < NR
        for o, t in zip(out, (x[S.TWIN[name]] for x in _run_once(W, "cases"))):
            assert np.array_equal(o["summed"], t["summed"]) and all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], t["state"]))
    if name.startswith("idle"):
        idle = [r for r in range(W) if not len(c["batches"][r][0])][0]
        assert out[idle]["stats"]["rows_mine"] == 0 and not out[idle]["local"].any()


# --------------------------------------------------------------------------- protocol
def test_second_exchange_events_memory_and_two_steps_with_disjoint_rows():
    name = "disjoint_items_f64"
    c, out = S.case(name), _run_ranks(2, "protocol", name)
    dims = c["dims"]
    NI, E = dims[4], dims[0]
    items = lambda g: g[:NI * E].reshape(NI, E)
    mine = [np.unique(seq[seq >= 0]) for seq, _ in c["batches"]]
    assert np.intersect1d(mine[0], mine[1]).size == 0
    for r, o in enumerate(out):
        code, msg = o["again"]
        assert code == ERR_STATE and "already exchanged" in msg, o["again"]
        assert np.array_equal(o["still"], o["summed"])              # the refusal left the sum alone
        assert o["silent"] == (0, 0)                                # no DM_DR_TIME_LAUNCHES: the two kinds record nothing
        assert o["timed"] == (2, 1), o["timed"]                     # with it: rows + block, and one pair around the rebuild
        assert o["warm"] and o["freed"] and o["closed"]             # no allocation in a warm call; dr_train_free returns everything
        assert o["summed"].tobytes() == out[0]["summed"].tobytes() and o["summed2"].tobytes() == out[0]["summed2"].tobytes()
        assert o["w1"].tobytes() == out[0]["w1"].tobytes() and o["w2"].tobytes() == out[0]["w2"].tobytes()
        assert o["w2"].tobytes() != o["w1"].tobytes()
        # step 1 moved the other rank's item rows here too: received rows are active
        other = mine[1 - r]
        assert (items(o["w1"])[other] != items(c["w"])[other]).any(axis=1).all()
        # step 2's local gradient: exact, and nothing left of the rows received in step 1
        assert np.array_equal(o["g2"], o["g2_fresh"])
        assert items(o["summed"])[other].any() and not items(o["g2"])[other].any()
    assert np.array_equal(out[0]["summed2"], S.dense_sum([o["g2"] for o in out]))


@pytest.mark.parametrize("what", ["dtype", "num_item"])
def test_disagreement_fails_every_rank(what):
    out = _run_ranks(2, "mismatch", what)
    for o in out:
        code, msg = o["refusal"]
        assert code == ERR_STATE and "another shape" in msg, o["refusal"]
        assert o["untouched"] and o["after"] == (1, True) and o["stepped"]


def test_single_process_refusals_and_one_rank_communicators():
    """every refusal before any collective, each followed by a good call; both one-rank transports (RCCL: ncclCommInitRank on the real
    device) move nothing and say who was there"""
    import threading
    from dismember_amd import Engine, _native as N
    from dismember_amd.comm import Comm
    c = S.case("shared_w2_f64")
    eng, bare = _engine(c, train=False), Engine(0)
    one, comms = None, [None, None]
    try:
        eng.dr_train_init(lr=LR)
        _fb(eng, c["batches"][0])
        eng.dr_train_free()
        base = live_allocs()                                        # the model and what a step derives from it, no training state
        one = Comm(1, 0, "127.0.0.1", _free_port(), transport="host")
        port = _free_port()

        def make(r):
            comms[r] = Comm(2, r, "127.0.0.1", port, transport="host")
        th = [threading.Thread(target=make, args=(r,)) for r in range(2)]
        [t.start() for t in th]; [t.join(60) for t in th]
        assert comms[0] is not None and comms[1] is not None

        def good():
            eng.attach_comm(one)
            g = eng.dr_train_download("grad")
            eng.dr_train_sync_gradients()
            assert eng.train_sync_stats()["nranks"] == 1 and eng.dr_train_download("grad").tobytes() == g.tobytes()
            eng.attach_comm(None)

        def refused(e, word):
            got, msg = _refused(e.dr_train_sync_gradients)
            assert got == ERR_STATE and word in msg, (got, msg)
        # no Deep-Retrieval model; no training state, with and without a communicator (two ranks: refused before any collective)
        refused(bare, "not loaded")
        refused(eng, "dm_dr_train_init")
        eng.attach_comm(comms[0])
        refused(eng, "dm_dr_train_init")
        eng.attach_comm(None)
        eng.dr_train_init(lr=LR)
        _fb(eng, c["batches"][0])
        good()
        refused(eng, "no communicator")
        good()
        # the other two exchanges keep refusing a Deep-Retrieval handle
        eng.attach_comm(one)
        assert N.lib().dm_train_sync_gradients(eng._h) != 0 and N.lib().dm_deepfm_train_sync_gradients(eng._h) != 0
        eng.attach_comm(None)
        good()
        g = eng.dr_train_download("grad")
        for transport in ("host", "rccl"):
            cm = Comm(1, 0, "127.0.0.1", _free_port(), transport=transport, device_id=0)
            eng.attach_comm(cm)
            before = live_allocs()
            for _ in range(2):                                      # (no "already exchanged" on a communicator of one: nothing was summed)
                eng.dr_train_sync_gradients()
            st = eng.train_sync_stats()
            assert (st["nranks"], st["transport"], st["rows_total"], st["bytes_sent"], st["host_syncs"]) == (1, transport, 0, 0, 0), st
            assert eng.dr_train_download("grad").tobytes() == g.tobytes() and live_allocs() == before
            eng.attach_comm(None)
            cm.close()
        eng.dr_adam_step(1.0)
        assert eng.dr_train_download("weights").tobytes() != c["w"].tobytes()
        eng.dr_train_free()
        assert live_allocs() == base
    finally:
        eng.close(); bare.close()
        for cm in [one] + comms:
            if cm is not None:
                cm.close()


# --------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("B", [64, 5, 1])
def test_trainer_replicas_loss_and_serving(B):
    W = 2
    out = _run_once(W, "trainer", (B, False))
    _, w0 = _problem()
    P = layer_slices(B, W)[1]
    assert P == (1 if B == 1 else 2) and all(o["P"] == P for o in out)
    for o in out:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], out[0]["state"]))
        assert o["state"][0].tobytes() != w0.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(o["losses"], out[0]["losses"])) and len(o["losses"]) == 3
        assert o["losses"][2].sum() < o["losses"][0].sum()          # it learns
        assert o["sync_calls"] == 3 and o["sync_s"] > 0 and o["stats"]["nranks"] == 2 and o["stats"]["rows_total"] > 0
    local = [o["local"] for o in out if o["local"] is not None]
    assert len(local) == P and (B > 1 or out[1]["local"] is None)
    assert np.array_equal(out[0]["losses"][0], S.dense_sum(local) / P)
    got, want = out[0]["search"]
    assert got == want and out[0]["found"] > 0


def test_trainer_with_the_rerank_model():
    out = _run_once(2, "trainer", (64, True))
    for o in out:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], out[0]["state"]))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["rr"], out[0]["rr"]))
        assert all(np.array_equal(a, b) for a, b in zip(o["rr"], out[0]["solo_rr"]))          # the rerank half is unsplit
        assert o["rr_losses"] == out[0]["solo_rr_losses"] and all(np.isfinite(o["rr_losses"]))
    g_w = out[0]["rr"][0]
    assert np.abs(out[0]["rr"][1]).max() > 0 and g_w.size > 0       # it trained: a first moment that is not zero
    got, want = out[0]["search"]
    assert got == want


def test_mismatched_seeds_raise():
    for msg in _run_ranks(2, "seeds"):
        assert "same seed" in msg, msg
