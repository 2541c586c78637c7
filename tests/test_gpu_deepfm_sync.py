"""The DeepFM gradient exchange behind the C ABI (dm_deepfm_train_sync_gradients = LocalOptimizer.syncGradients,
tdm/src/main/scala/com/mass/tdm/optim/LocalOptimizer.scala:164-187, minus the division) on real engines: dismember_amd/csrc/dfm_train_sync.hip.inc.

A GPU box has ONE device and RCCL refuses two ranks per device, so the multi-worker protocol runs as W spawned processes sharing the GPU
over the library's host transport (same entry point, same kernels; only the wire differs), as tests/test_gpu_comm.py does.  A failing rank
reports its traceback and ends the test: nobody waits longer than the queue's timeout, and stragglers are terminated.  Every gradient
comparison is np.array_equal against the float32 numpy sum in rank order (tests/deepfm_sync_ref.py): exact IEEE adds in a fixed order.

The two launch kinds of the exchange and the "already exchanged" refusal need an exchange that moved something, hence more than one rank:
they are checked inside the two-rank run, not in the single-process tests."""
import ctypes as C
import functools
import multiprocessing as mp
import os
import socket
import threading
import traceback

import numpy as np
import pytest

import deepfm_ref as R
import deepfm_sync_ref as S
import deepfm_train_ref as T

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NEG = np.arange(13, dtype=np.int32)
EV_PACK, EV_SUM = 77, 78
ERR_STATE, ERR_UNSUPPORTED = -3, -5


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


def padded_view(eng, what):
    """the device's own (padded) vector through the debug view, not in the public header"""
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_deepfm_train_padded
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, N.f32p, N.i64p]
    n = C.c_int64(0)
    assert fn(eng._h, what, None, C.byref(n)) == 0
    out = np.empty(n.value, np.float32)
    assert fn(eng._h, what, out.ctypes.data_as(N.f32p), C.byref(n)) == 0
    return out


def _ulps(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.float32(1e-45)).astype(np.float64)


def _engine(c):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_weights_deepfm(c["w"], c["E"], c["L"], c["NI"])
    return eng


def _fb(eng, batch):
    """the local step; a rank whose batch is empty runs nothing (as TDMTrainer does when the sampler drew no rows)"""
    codes, seqs, y = batch
    return eng.deepfm_train_forward_backward(codes, seqs, y) if codes.size else 0.0


def _refused(call):
    from dismember_amd import DismemberError
    try:
        call()
    except DismemberError as e:
        return e.code, str(e)
    return 0, ""


# --------------------------------------------------------------------------- what a rank runs (module level: spawn imports this file)
def _sc_sum(rank, world, comm, name):
    """one exchange checked from every side, then a warm second one with the launch kinds on"""
    c = S.case(name)
    eng = _engine(c)
    base = live_allocs()
    eng.deepfm_train_init(lr=1e-3)
    eng.attach_comm(comm)
    _fb(eng, c["batches"][rank])
    local = eng.deepfm_train_download("grad")
    eng.timing_reset()
    eng.deepfm_train_sync_gradients()
    silent = (eng.timing_get_kind(EV_PACK)[0], eng.timing_get_kind(EV_SUM)[0])
    summed, stats = eng.deepfm_train_download("grad"), eng.train_sync_stats()
    again = _refused(eng.deepfm_train_sync_gradients)               # no step in between: refused on every rank, before any collective
    still = eng.deepfm_train_download("grad")
    eng.deepfm_adam_step(1.0 / world)
    state = tuple(eng.deepfm_train_download(k) for k in ("weights", "s", "r"))
    os.environ["DM_DFM_TIME_LAUNCHES"] = "1"
    try:
        _fb(eng, c["batches"][rank])
        before = live_allocs()
        eng.timing_reset()
        eng.deepfm_train_sync_gradients()
        warm = live_allocs() == before
        timed = (eng.timing_get_kind(EV_PACK)[0], eng.timing_get_kind(EV_SUM)[0])
    finally:
        del os.environ["DM_DFM_TIME_LAUNCHES"]
    eng.deepfm_adam_step(1.0 / world)
    w2 = eng.deepfm_train_download("weights")
    eng.attach_comm(None)
    eng.deepfm_train_free()
    freed = live_allocs() == base
    eng.close()
    return dict(local=local, summed=summed, stats=stats, again=again, still=still, state=state, silent=silent, timed=timed, warm=warm, w2=w2, freed=freed)


def _sc_disjoint(rank, world, comm, name):
    c = S.case(name)
    eng = _engine(c)
    eng.deepfm_train_init(lr=1e-3)
    eng.attach_comm(comm)
    batch = c["batches"][rank]
    _fb(eng, batch)
    local = eng.deepfm_train_download("grad")
    eng.deepfm_train_sync_gradients()
    summed = eng.deepfm_train_download("grad")
    eng.deepfm_adam_step(1.0 / world)
    w1 = eng.deepfm_train_download("weights")
    # step 2, with a detour: forward/backward -> exchange -> forward/backward on the same batch is the local gradient again
    _fb(eng, batch)
    g_a = eng.deepfm_train_download("grad")
    eng.deepfm_train_sync_gradients()
    _fb(eng, batch)
    g_b = eng.deepfm_train_download("grad")
    eng.deepfm_train_sync_gradients()
    eng.deepfm_adam_step(1.0 / world)
    w2 = eng.deepfm_train_download("weights")
    eng.close()
    return dict(local=local, summed=summed, w1=w1, w2=w2, again_local=g_a.tobytes() == g_b.tobytes(), moved=g_a.tobytes() != local.tobytes())


def _edge_run(rank, world, comm, c, padded):
    eng = _engine(c)
    eng.deepfm_train_init(lr=1e-3)
    eng.attach_comm(comm)
    _fb(eng, c["batches"][rank])
    out = dict(local=eng.deepfm_train_download("grad"))
    eng.deepfm_train_sync_gradients()
    out["summed"], out["stats"] = eng.deepfm_train_download("grad"), eng.train_sync_stats()
    if padded:
        out["padded"] = padded_view(eng, 1)
    eng.deepfm_adam_step(1.0 / world)
    out["state"] = tuple(eng.deepfm_train_download(k) for k in ("weights", "s", "r"))
    eng.close()
    return out


def _sc_edges(rank, world, comm, _):
    out = {name: _edge_run(rank, world, comm, S.case(name), name == "embed_24") for name in S.EDGES}
    os.environ["DM_ADAM_DENSE"] = "1"                               # the dense stream against the rows path, after an exchange
    try:
        out["embed_24_dense"] = _edge_run(rank, world, comm, S.case("embed_24"), False)
    finally:
        del os.environ["DM_ADAM_DENSE"]
    return out


def _tdm_world(world):
    from dismember_amd import synth
    t = np.load(os.path.join(GOLDEN, "tdm_tree.npz"))
    rng = np.random.default_rng(0)
    seqs = synth.make_users(t["leaf_ids"], 32 * world, 10, rng)
    tgt = rng.choice(t["leaf_ids"], 32 * world).astype(np.int32)
    w = R.random_deepfm_weights(np.random.default_rng(5), 16, 10, 8191)
    return t, seqs, tgt, w


def _tdm_engine(t, w):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_deepfm(w, 16, 10, 8191)
    return eng


def _search_dev(eng, seqs, beam, topk):
    U, L = seqs.shape
    d_seq, d_ids, d_sc, d_cnt = eng.dev_alloc(U * L * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * 4)
    try:
        eng.h2d(d_seq, np.ascontiguousarray(seqs, np.int32))
        eng.tdm_beam_search_dev(d_seq, U, L, beam, topk, d_ids, d_sc, d_cnt, use_mask=False)
        eng.synchronize()
        ids, sc, cnt = np.empty((U, topk), np.int32), np.empty((U, topk), np.float32), np.empty(U, np.int32)
        eng.d2h(ids, d_ids); eng.d2h(sc, d_sc); eng.d2h(cnt, d_cnt)
    finally:
        for p in (d_seq, d_ids, d_sc, d_cnt):
            eng.dev_free(p)
    m = np.arange(topk)[None, :] < cnt[:, None]
    return ids[m].tobytes() + sc[m].tobytes() + cnt.tobytes(), int(cnt.sum())


def _sc_trainer(rank, world, comm, form):
    from dismember_amd import sharding
    from dismember_amd.trainer import TDMTrainer
    t, seqs, tgt, w = _tdm_world(world)
    eng = _tdm_engine(t, w)
    tr = TDMTrainer(eng, NEG, lr=1e-3, comm=comm, seed=77, sampler="host" if form == "host" else "device", grouped=form == "grouped")
    lo, hi = sharding.shard_range(len(seqs), rank, world)
    losses = [float(tr.step(seqs[lo:hi], tgt[lo:hi])) for _ in range(3)]
    out = dict(losses=losses, weights=eng.deepfm_train_download("weights"), sync_calls=tr.sync_calls, stats=eng.train_sync_stats())
    if rank == 0 and form == "device":
        # the handle that trained data-parallel serves what a fresh handle loaded from its downloaded weights serves
        fresh = _tdm_engine(t, out["weights"])
        codes, hist, _ = eng.deepfm_make_train_batch(seqs[:8], tgt[:8], NEG, 1, seed=99)
        out["rows"] = int(codes.size)
        out["forward"] = (eng.deepfm_forward(codes, hist).tobytes(), fresh.deepfm_forward(codes, hist).tobytes())
        out["search"] = (_search_dev(eng, seqs[:16], 8, 5), _search_dev(fresh, seqs[:16], 8, 5))
        fresh.close()
    eng.attach_comm(None)
    eng.close()
    return out


def _sc_mismatch(rank, world, comm, _):
    from dismember_amd.comm import Comm
    c = S.case("shared_w2")
    L = c["L"] - rank                                               # rank 1 trains seq_len 9
    rng = np.random.default_rng(33 + rank)
    eng = _engine(dict(c, L=L, w=R.random_deepfm_weights(rng, c["E"], L, c["NI"])))
    eng.deepfm_train_init(lr=1e-3)
    eng.attach_comm(comm)
    codes, seqs, y = c["batches"][rank]
    eng.deepfm_train_forward_backward(codes, np.ascontiguousarray(seqs[:, :L]), y)
    local = eng.deepfm_train_download("grad")
    out = dict(refusal=_refused(eng.deepfm_train_sync_gradients), untouched=eng.deepfm_train_download("grad").tobytes() == local.tobytes())
    if rank == 0:                                                   # the handle is usable: a good call on a communicator of one
        one = Comm(1, 0, "127.0.0.1", _free_port(), transport="host")
        eng.attach_comm(one)
        eng.deepfm_train_sync_gradients()
        out["after"] = (eng.train_sync_stats()["nranks"], eng.deepfm_train_download("grad").tobytes() == local.tobytes())
        eng.attach_comm(None)
        one.close()
    eng.close()
    return out


SCENARIOS = {"sum": _sc_sum, "disjoint": _sc_disjoint, "edges": _sc_edges, "trainer": _sc_trainer, "mismatch": _sc_mismatch}


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


def _check_sum(c, out, W):
    E, L, NI = c["E"], c["L"], c["NI"]
    want = S.dense_sum([o["local"] for o in out])
    rows = [S.batch_rows(b[0], b[1], NI) for b in c["batches"]]
    union, acc, tail = S.exchange([S.split(o["local"], rows[r], E, NI) for r, o in enumerate(out)], E, NI)
    assert np.array_equal(S.assemble(union, acc, tail, E, NI), want)         # (no gradient outside the batch's rows: the restatement's form)
    for r, o in enumerate(out):
        assert np.array_equal(o["summed"], want), r
        st = o["stats"]
        assert (st["nranks"], st["transport"], st["rows_mine"], st["rows_total"]) == (W, "host", rows[r].size, sum(x.size for x in rows)), st
        words = lambda n: 4 * (n + n * ((E + 15) // 16 * 16) + (L + 1) * (L + 1) * ((E + 15) // 16 * 16) + 2 * (L + 1) + 1)
        assert st["bytes_sent"] == words(rows[r].size) and st["bytes_recv"] == sum(words(x.size) for x in rows), st
        assert 1 <= st["host_syncs"] <= 5, st                        # row count, staging down and up, end; one more when the key list grows
    return want


# --------------------------------------------------------------------------- the exchange
@pytest.mark.parametrize("world", [2, 3])
def test_exchange_equals_the_rank_ordered_sum(world):
    name = "shared_w%d" % world
    c, out = S.case(name), _run_once(world, "sum", name)
    want = _check_sum(c, out, world)
    E, NI = c["E"], c["NI"]
    assert (np.abs(want[:NI * E]).reshape(NI, E).sum(1) > 0).sum() > 300
    if world == 3:
        assert not np.array_equal(S.dense_sum([o["local"] for o in out][::-1]), want)      # the order is visible in these bytes
    wn, sn, rn = c["w"].copy(), np.zeros_like(c["w"]), np.zeros_like(c["w"])
    T.adam_update(wn, want, sn, rn, 1, 1e-3, grad_scale=1.0 / world)
    for o in out:
        w1, s1, r1 = o["state"]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], out[0]["state"]))
        assert w1.tobytes() != c["w"].tobytes()
        assert np.abs(sn).max() > 0 and _ulps(s1, sn).max() <= 2 and _ulps(r1, rn).max() <= 2
        assert np.allclose(w1, wn, rtol=1e-5, atol=1e-7)
        assert o["w2"].tobytes() == out[0]["w2"].tobytes() and o["w2"].tobytes() != w1.tobytes()


def test_second_exchange_is_refused_events_and_memory():
    for o in _run_once(2, "sum", "shared_w2"):
        code, msg = o["again"]
        assert code == ERR_STATE and "already exchanged" in msg, o["again"]
        assert np.array_equal(o["still"], o["summed"])              # the refusal left the sum alone
        assert o["silent"] == (0, 0)                                # no DM_DFM_TIME_LAUNCHES: the two kinds record nothing
        assert o["timed"] == (2, 1), o["timed"]                     # with it: rows + block, and one pair around the rebuild
        assert o["warm"] and o["freed"]                             # no allocation in a warm call; deepfm_train_free returns everything


def test_repeatability():
    a = _run_once(2, "sum", "shared_w2")
    b = _run_ranks(2, "sum", "shared_w2")
    for x, y in zip(a, b):
        for k in ("local", "summed", "w2"):
            assert x[k].tobytes() == y[k].tobytes(), k
        assert all(u.tobytes() == v.tobytes() for u, v in zip(x["state"], y["state"]))


def test_disjoint_rows_two_steps():
    c, out = S.case("disjoint"), _run_ranks(2, "disjoint", "disjoint")
    want = S.dense_sum([o["local"] for o in out])
    E, NI = c["E"], c["NI"]
    emb = lambda g: np.asarray(g[:NI * E]).reshape(NI, E)
    mine = [np.flatnonzero(np.abs(emb(o["local"])).sum(1) > 0) for o in out]
    assert np.intersect1d(mine[0], mine[1]).size == 0 and mine[0].size > 500 and mine[1].size > 500
    for o in out:
        assert np.array_equal(o["summed"], want)
        assert o["w1"].tobytes() == out[0]["w1"].tobytes() and o["w2"].tobytes() == out[0]["w2"].tobytes()      # received rows are active
        assert o["w2"].tobytes() != o["w1"].tobytes() != c["w"].tobytes()
        assert o["moved"] and o["again_local"]                      # received rows are cleared by the next step: they are in `prev`
    # every row either rank reached moved on both replicas
    w1 = emb(out[0]["w1"])
    assert (w1[np.concatenate(mine)] != emb(c["w"])[np.concatenate(mine)]).any(axis=1).all()


def test_edges():
    out = _run_ranks(2, "edges")
    for name in S.EDGES:
        c = S.case(name)
        res = [o[name] for o in out]
        _check_sum(c, res, 2)
        for o in res:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], res[0]["state"])), name
            assert o["state"][0].tobytes() != c["w"].tobytes(), name
    # the empty rank sent no rows and a zero tail, and holds rank 0's gradient
    e = [o["empty_rank"] for o in out]
    assert not e[1]["local"].any() and e[1]["stats"]["rows_mine"] == 0 and np.array_equal(e[1]["summed"], e[0]["local"])
    # E = 24 lives padded to 32 on the device: the padded columns of the exchanged gradient are exact zeros
    c = S.case("embed_24")
    E, Ep, NI, Tt = 24, 32, c["NI"], c["L"] + 1
    for o in (x["embed_24"] for x in out):
        blocks = o["padded"][:NI * Ep + Tt * Tt * Ep].reshape(-1, Ep)
        assert not blocks[:, E:].any() and blocks[:, :E].any()
        assert np.array_equal(np.concatenate([blocks[:, :E].ravel(), o["padded"][NI * Ep + Tt * Tt * Ep:]]), o["summed"])
    # DM_ADAM_DENSE=1 after an exchange: the bytes of the rows path
    for o in out:
        assert np.array_equal(o["embed_24_dense"]["summed"], o["embed_24"]["summed"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["embed_24_dense"]["state"], o["embed_24"]["state"]))
    st = [o["tile_4095_4097"]["stats"] for o in out]
    assert [s["rows_mine"] for s in st] == [4095, 4097]


# --------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("form", ["device", "grouped", "host"])
def test_trainer_every_step_form(form):
    out = _run_once(2, "trainer", form)
    w0 = _tdm_world(2)[3]
    for o in out:
        assert o["weights"].tobytes() == out[0]["weights"].tobytes()
        assert o["losses"] == out[0]["losses"] and len(o["losses"]) == 3 and all(np.isfinite(o["losses"])) and all(v > 0 for v in o["losses"])
        assert o["weights"].tobytes() != w0.tobytes()
        assert o["sync_calls"] == 3 and o["stats"]["nranks"] == 2 and o["stats"]["rows_total"] > 0


def test_serving_after_data_parallel_training():
    o = _run_once(2, "trainer", "device")[0]
    assert o["rows"] > 0 and o["forward"][0] == o["forward"][1]
    (got, n_got), (want, n_want) = o["search"]
    assert n_got == n_want > 0 and got == want


# --------------------------------------------------------------------------- refusals
def test_shape_disagreement_fails_every_rank():
    out = _run_ranks(2, "mismatch")
    for o in out:
        code, msg = o["refusal"]
        assert code == ERR_STATE and "another shape" in msg, o["refusal"]
        assert o["untouched"]
    assert out[0]["after"] == (1, True)


def test_single_process_refusals_and_one_rank_communicators():
    from dismember_amd import Engine, _native as N
    from dismember_amd.comm import Comm
    c = S.case("shared_w2")
    eng, din = _engine(c), Engine(0)
    one, comms, clone = None, [None, None], None
    try:
        din.load_weights_din(np.load(os.path.join(GOLDEN, "din_f32.npy")), 16, 8191)
        din.train_init()
        base = live_allocs()
        one = Comm(1, 0, "127.0.0.1", _free_port(), transport="host")
        port = _free_port()

        def make(r):
            comms[r] = Comm(2, r, "127.0.0.1", port, transport="host")
        th = [threading.Thread(target=make, args=(r,)) for r in range(2)]
        [t.start() for t in th]; [t.join(60) for t in th]
        assert comms[0] is not None and comms[1] is not None

        def good():
            """a call that works: the one-rank communicator, gradient untouched"""
            eng.attach_comm(one)
            g = eng.deepfm_train_download("grad")
            eng.deepfm_train_sync_gradients()
            assert eng.train_sync_stats()["nranks"] == 1 and eng.deepfm_train_download("grad").tobytes() == g.tobytes()
            eng.attach_comm(None)

        def refused(e, word, code=ERR_STATE):
            got, msg = _refused(e.deepfm_train_sync_gradients)
            assert got == code and word in msg, (got, msg)
        # no training state, with and without a communicator (two ranks: refused before any collective)
        refused(eng, "dm_deepfm_train_init")
        eng.attach_comm(comms[0])
        refused(eng, "dm_deepfm_train_init")
        eng.attach_comm(None)
        eng.deepfm_train_init(lr=1e-3)
        _fb(eng, c["batches"][0])
        good()
        # no communicator
        refused(eng, "no communicator")
        good()
        # a DIN model; and the DIN entry point keeps refusing a DeepFM model
        din.attach_comm(one)
        refused(din, "the loaded scorer is DIN")
        din.train_sync_gradients()                                  # (its own exchange still works on that handle)
        din.attach_comm(None)
        eng.attach_comm(one)
        assert N.lib().dm_train_sync_gradients(eng._h) == ERR_UNSUPPORTED
        eng.attach_comm(None)
        good()
        # a clone, with the two-rank communicator on the owner
        eng.attach_comm(comms[0])
        clone = eng.clone()
        refused(clone, "clone")
        clone.close(); clone = None
        eng.attach_comm(None)
        good()
        eng.deepfm_adam_step(1.0)
        assert eng.deepfm_train_download("weights").tobytes() != c["w"].tobytes()
        eng.deepfm_train_free()
        assert live_allocs() == base
    finally:
        if clone is not None:
            clone.close()
        eng.close(); din.close()
        for cm in [one] + comms:
            if cm is not None:
                cm.close()


def test_one_rank_communicators_are_a_no_op():
    """both transports (RCCL: ncclCommInitRank on the real device): nothing moves, the stats say who was there"""
    from dismember_amd.comm import Comm
    c = S.case("shared_w2")
    eng = _engine(c)
    try:
        base = live_allocs()
        eng.deepfm_train_init(lr=1e-3)
        _fb(eng, c["batches"][0])
        g = eng.deepfm_train_download("grad")
        for transport in ("host", "rccl"):
            cm = Comm(1, 0, "127.0.0.1", _free_port(), transport=transport, device_id=0)
            eng.attach_comm(cm)
            before = live_allocs()
            for _ in range(2):                                      # (no "already exchanged" on a communicator of one: nothing was summed)
                eng.deepfm_train_sync_gradients()
            st = eng.train_sync_stats()
            assert (st["nranks"], st["transport"], st["rows_total"], st["bytes_sent"], st["host_syncs"]) == (1, transport, 0, 0, 0), st
            assert eng.deepfm_train_download("grad").tobytes() == g.tobytes() and live_allocs() == before
            eng.attach_comm(None)
            cm.close()
        eng.deepfm_train_free()
        assert live_allocs() == base
    finally:
        eng.close()
