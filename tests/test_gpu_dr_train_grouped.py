"""GPU tests of the sample-grouped Deep-Retrieval training step and the eval loss (dm_dr_train_forward_backward_grouped*,
dm_dr_layer_loss) against tests/dr_train_ref.py on the EXPANDED batch (tests/dr_train_grouped_ref.py builds the cases).

H1 gradient and loss per case within |gpu - ref| <= k[tensor] eps_T A (k: tests/golden/dr_train_grouped_tolerances.json, measured on the
CPU), H2 reproducibility, H3 row and grouped steps in turn, H4 Adam wiring and the search's derived copies, H5 dr_layer_loss, H6 the
trainer and evaluate_dr, H7 data-parallel, H8 refusals."""
import ctypes as C
import functools
import json
import multiprocessing as mp
import os
import socket
import traceback

import numpy as np
import pytest

import dr_sync_ref as SY
import dr_train_grouped_ref as G
import dr_train_ref as R
from dismember_amd import synth
from dismember_amd.dr_train import DRTrainer, layer_slices, param_sections, split_params

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = json.load(open(os.path.join(GOLDEN, "dr_train_grouped_tolerances.json")))
OK, INVALID, STATE, INDEX, UNSUPPORTED = 0, -1, -3, -4, -5
MAX_ROWS = 65535 * 64


def engine_for(weights, dims, dtype, train=True, **adam):
    from dismember_amd import Engine
    E, L, K, D, NI = dims
    eng = Engine(0)
    eng.dr_load_model(weights, E, L, K, D, NI, dtype=dtype)
    if train:
        eng.dr_train_init(**adam)
    return eng


def case_engine(name, train=True, **adam):
    c = G.make_case(name)
    return c, engine_for(split_params(c["w"], *c["dims"]), c["dims"], R.NP[c["dtype"]], train=train, **adam)


def check_against(name, c, ref, loss, g):
    dt, K = c["dtype"], c["dims"][2]
    eps, k = R.EPS[dt], TOL[dt]["k"]
    ratios, zeros_exact = R.class_ratios(g.astype(np.float64), ref, eps, c["dims"])
    lr = G.loss_ratio(loss, ref, eps)
    print("%s: ratio / bound  %s  loss %.3g / %.3g" % (name, "  ".join("%s %.3g / %.3g" % (t, ratios[t], k[t]) for t in R.CLASSES), lr, k["loss"]))
    assert zeros_exact                      # what received nothing is exactly zero (padding, rows nobody named)
    if K == 1:
        assert (g == 0).all() and (loss == 0).all()
    for t in R.CLASSES:
        assert ratios[t] <= k[t], (t, ratios[t], k[t])
    assert lr <= k["loss"], (loss, ref["loss"])


# ------------------------------------------------------------------------------------------------------------------------ H1
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_gradient_and_loss_against_the_row_restatement(name):
    c, eng = case_engine(name)
    loss = eng.dr_train_forward_backward_grouped(c["seq"], c["paths"])
    g = eng.dr_train_download("grad")
    eng.close()
    check_against(name, c, G.reference(name), loss, g)


def test_device_arrays_give_the_host_entry_bytes():
    c, eng = case_engine("j-3-f32")
    eng.dr_train_forward_backward_grouped(c["seq"], c["paths"])
    g = eng.dr_train_download("grad")
    d_seq, d_pa = eng.dev_alloc(c["seq"].nbytes), eng.dev_alloc(c["paths"].nbytes)
    eng.h2d(d_seq, c["seq"]); eng.h2d(d_pa, c["paths"])
    loss = eng.dr_train_forward_backward_grouped_dev(d_seq, d_pa, c["S"], c["J"])
    assert eng.dr_train_download("grad").tobytes() == g.tobytes() and np.isfinite(loss).all()
    eng.dev_free(d_seq); eng.dev_free(d_pa)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ H2
@pytest.mark.parametrize("name", ["cache-13-f32", "same-sample-f64", "rows-513-f32", "row-1025-f64"])
def test_three_steps_are_reproducible_to_the_byte(name):
    c = G.make_case(name)
    rng = np.random.default_rng(7)
    E, L, K, D, _ = c["dims"]
    batches = [(c["seq"], c["paths"])] + [G.make_batch(rng, K, D, L, c["S"], c["J"], "pad") for _ in range(2)]
    runs = []
    for _ in range(2):
        _, eng = case_engine(name, lr=1e-2)
        for seq, paths in batches:
            l1 = eng.dr_train_forward_backward_grouped(seq, paths)
            g = eng.dr_train_download("grad")
            l2 = eng.dr_train_forward_backward_grouped(seq, paths)                       # one call repeated: the same bytes
            assert eng.dr_train_download("grad").tobytes() == g.tobytes() and l1.tobytes() == l2.tobytes()
            eng.dr_adam_step(1.0)
        runs.append([g.tobytes()] + [eng.dr_train_download(w).tobytes() for w in ("weights", "grad", "s", "r")])
        eng.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------------------ H3
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_row_and_grouped_steps_in_turn_clear_each_others_rows(dt):
    """each step's zeroGradParameters clears the rows the OTHER kind of step remembered: every gradient is its own reference's"""
    c, eng = case_engine("all-pad-sample-" + dt)
    dims = c["dims"]
    rng = np.random.default_rng(17)
    E, L, K, D, _ = dims
    seq2, paths2 = G.make_batch(rng, K, D, L, 21, 2, "pad")                              # other rows than the case's
    row2 = G.expand(seq2, paths2)
    ref1, ref2 = G.reference("all-pad-sample-" + dt), R.step(c["w"], dims, *row2)
    for first_grouped in (True, False):
        if first_grouped:
            eng.dr_train_forward_backward_grouped(c["seq"], c["paths"])
            loss = eng.dr_train_forward_backward(*row2)
            want = ref2
        else:
            eng.dr_train_forward_backward(*row2)
            loss = eng.dr_train_forward_backward_grouped(c["seq"], c["paths"])
            want = ref1
        check_against("in-turn", c, want, loss, eng.dr_train_download("grad"))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ H4
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_adam_after_a_grouped_step(dt):
    K, D, L, E, NI, S, J = 7, 3, 4, 16, R.NUM_ITEM, 4, 2
    dims, T = (E, L, K, D, NI), R.NP[dt]
    rng = np.random.default_rng(11)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    seq, paths = G.make_batch(rng, K, D, L, S, J, "pad")
    out = {}
    for mode in ("rows", "dense"):
        eng = engine_for(wd, dims, T, lr=1e-2)
        w0 = eng.dr_train_download("weights")
        eng.dr_train_forward_backward_grouped(seq, paths)
        if mode == "dense":
            os.environ["DM_ADAM_DENSE"] = "1"
        try:
            eng.dr_adam_step(0.5)
        finally:
            os.environ.pop("DM_ADAM_DENSE", None)
        out[mode] = [eng.dr_train_download(w) for w in ("weights", "s", "r")]
        assert (eng.dr_train_download("grad") == 0).all()
        eng.close()
    w1 = out["rows"][0]
    sec = param_sections(*dims)
    touched = R.touched_rows(dict(dims=dims, seq=seq, paths=paths.reshape(-1, D)))
    assert 4 * touched.sum() < len(touched)                                 # few enough rows for the active-rows path
    emb0, emb1 = (v[slice(*sec["emb"])].reshape(-1, E) for v in (w0, w1))
    assert emb0[~touched].tobytes() == emb1[~touched].tobytes()             # untouched rows do not move
    assert (emb0[touched] != emb1[touched]).any(axis=1).all()
    for a, b in zip(out["rows"], out["dense"]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dt,E", [("f64", 16), ("f32", 64)])
def test_derived_copies_follow_the_weights_trained_by_grouped_steps(dt, E):
    K, D, L, NI, S, J, beam = 40, 3, 5, 300, 48, 2, 8
    dims, T = (E, L, K, D, NI), R.NP[dt]
    rng = np.random.default_rng(21)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    wd = {k: ([a.astype(T) for a in v] if isinstance(v, list) else v.astype(T)) for k, v in wd.items()}
    users = rng.integers(0, NI, size=(24, L)).astype(np.int32)
    users[rng.random(users.shape) < 0.2] = -1
    a = engine_for(wd, dims, T, lr=5e-2)
    before = a.dr_beam_search(users, beam)
    for _ in range(3):
        a.dr_train_forward_backward_grouped(*G.make_batch(rng, K, D, L, S, J, "pad", num_item=NI))
        a.dr_adam_step(1.0)
    trained = split_params(a.dr_train_download("weights"), *dims)
    b = engine_for(dict(wd, **trained), dims, T, train=False)
    sa, sb = a.dr_beam_search(users, beam), b.dr_beam_search(users, beam)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert not all(np.array_equal(x, y) for x, y in zip(sa, before))          # the search saw the new weights
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------------ H5
@pytest.mark.parametrize("name", ["j-3-f32", "j-3-f64", "row-1025-f32", "row-1025-f64", "cache-13-f64", "tiny-f32"])
def test_layer_loss_against_the_restatement(name):
    c, eng = case_engine(name, train=False)                                    # no dr_train_init
    ref = R.step(c["w"], c["dims"], *G.expand(c["seq"], c["paths"]), loss_only=True)
    dt = c["dtype"]
    loss = eng.dr_layer_loss(c["seq"], c["paths"])
    lr = G.loss_ratio(loss, ref, R.EPS[dt])
    print("%s: layer loss ratio %.3g / %.3g" % (name, lr, TOL[dt]["k"]["loss"]))
    assert lr <= TOL[dt]["k"]["loss"]
    os.environ["DM_DR_LAYER_LOSS_ROWS"] = "3"                                  # chunks of 3 samples, the last one shorter
    try:
        chunked = eng.dr_layer_loss(c["seq"], c["paths"])
    finally:
        del os.environ["DM_DR_LAYER_LOSS_ROWS"]
    assert G.loss_ratio(chunked, ref, R.EPS[dt]) <= TOL[dt]["k"]["loss"]
    eng.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_layer_loss_leaves_the_training_state_alone(dt):
    """forward/backward, dr_layer_loss, Adam, a second step: the bytes of the same sequence without the loss call"""
    name = "j-2-" + dt
    c = G.make_case(name)
    E, L, K, D, _ = c["dims"]
    other = G.make_batch(np.random.default_rng(3), K, D, L, 9, 3, "pad")
    runs = []
    for with_loss in (False, True):
        _, eng = case_engine(name, lr=1e-2)
        eng.dr_train_forward_backward_grouped(c["seq"], c["paths"])
        if with_loss:
            eng.dr_layer_loss(*other)
        g = eng.dr_train_download("grad")
        eng.dr_adam_step(1.0)
        if with_loss:
            eng.dr_layer_loss(*other)
        eng.dr_train_forward_backward_grouped(*other)
        runs.append([g.tobytes()] + [eng.dr_train_download(w).tobytes() for w in ("weights", "grad", "s", "r")])
        eng.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------------------ H6
def _trainer(p, **kw):
    eng = engine_for(p["weights"], p["dims"], np.float64, train=False)
    return eng, DRTrainer(eng, p["item_paths"], lr=p["lr"], **kw)


def test_grouped_trainer_learns():
    p = R.learning_problem()
    eng, tr = _trainer(p, grouped=True)
    assert tr.grouped
    for _ in range(p["steps"]):
        tr.step(p["seqs"], p["targets"])
    first, last = tr.losses[0], tr.losses[-1]
    print("losses", first, last)
    assert (last < 0.8 * first).all()
    eng.close()


def test_grouped_trainer_follows_the_row_trainer_with_two_paths_per_item():
    """J = 2: the first step's loss within the loss bound of the row trainer's; the environment switch selects the grouped step"""
    p = R.learning_problem()
    rng = np.random.default_rng(4)
    K = p["dims"][2]
    paths2 = np.concatenate([p["item_paths"], rng.integers(0, K, size=p["item_paths"].shape).astype(np.int32)], axis=1)
    os.environ["DM_DR_TRAIN_GROUPED"] = "1"
    try:
        eng_g, tg = _trainer(dict(p, item_paths=paths2))
    finally:
        del os.environ["DM_DR_TRAIN_GROUPED"]
    eng_r, trw = _trainer(dict(p, item_paths=paths2))
    assert tg.grouped and not trw.grouped
    lg, lrw = tg.step(p["seqs"], p["targets"]), trw.step(p["seqs"], p["targets"])
    # both lie within k_loss eps64 A_loss (k_loss about 10, A_loss about 5 x the loss here) of the same restatement: 2 x 10 x 1.1e-16 x 5
    np.testing.assert_allclose(lg, lrw, rtol=1e-13)
    eng_g.close(); eng_r.close()


def test_evaluate_dr_reports_the_layer_losses():
    from dismember_amd.evaluation import evaluate_dr
    K, D, L, E, NI, J, N = 12, 2, 4, 16, 80, 2, 40
    rng = np.random.default_rng(9)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    item_paths = synth.make_dr_paths(NI, K, D, J, rng)
    eng = engine_for(wd, (E, L, K, D, NI), np.float64, train=False)
    eng.dr_load_path_items(*synth.dr_path_items(item_paths))
    tr = DRTrainer(eng, item_paths, lr=1e-2, grouped=True)
    seqs = rng.integers(0, NI, size=(N, L)).astype(np.int32)
    targets = rng.integers(0, NI, size=N)
    tr.step(seqs, targets)
    want = tr.evaluate_layer(seqs, targets)
    assert want.shape == (D,) and (want > 0).all()
    labels = [[int(t)] for t in targets]
    res = evaluate_dr(eng, seqs, labels, np.arange(N), {u: [] for u in range(N)}, 5, 4, batch_size=N, loss_fn=tr.eval_loss_fn(seqs, targets))
    assert res.count == 1 and np.array_equal(np.asarray(res.layer_loss), want) and res.rerank_loss == 0.0
    halves = evaluate_dr(eng, seqs, labels, np.arange(N), {u: [] for u in range(N)}, 5, 4, batch_size=N // 2, loss_fn=tr.eval_loss_fn(seqs, targets))
    assert halves.count == 2
    np.testing.assert_allclose(np.asarray(halves.mean_metrics().layer_loss), want, rtol=1e-12)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ H7
# W = 2 spawned processes on one GPU over the host transport: the pattern of tests/test_gpu_dr_sync.py, its helpers copied
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sc_grouped(rank, world, comm, name):
    c, eng = case_engine(name, lr=1e-2)
    eng.attach_comm(comm)
    lo, n = layer_slices(c["S"], world)[0][rank]
    eng.dr_train_forward_backward_grouped(c["seq"][lo:lo + n], c["paths"][lo:lo + n])
    out = dict(local=eng.dr_train_download("grad"))
    eng.dr_train_sync_gradients()
    out["summed"] = eng.dr_train_download("grad")
    eng.dr_adam_step(1.0 / world)
    out["state"] = tuple(eng.dr_train_download(k) for k in ("weights", "s", "r"))
    eng.attach_comm(None)
    eng.close()
    return out


def _worker(rank, world, port, q, arg):
    try:
        from dismember_amd.comm import Comm
        comm = Comm(world, rank, "127.0.0.1", port, transport="host")
        out = _sc_grouped(rank, world, comm, arg)
        q.put((rank, "ok", out))
        comm.barrier()
        comm.close()
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
        raise


def _run_ranks(world, arg=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, arg)) for r in range(world)]
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


def test_data_parallel_grouped_steps_exchange_and_stay_identical():
    name = "j-2-f64"
    c = G.make_case(name)
    out = _run_ranks(2, name)
    want = SY.dense_sum([o["local"] for o in out])
    # a rank's local gradient is the grouped step's on its slice: the single-process bytes
    _, eng = case_engine(name)
    for r, o in enumerate(out):
        lo, n = layer_slices(c["S"], 2)[0][r]
        eng.dr_train_forward_backward_grouped(c["seq"][lo:lo + n], c["paths"][lo:lo + n])
        assert np.array_equal(eng.dr_train_download("grad"), o["local"]) and o["local"].any()
        assert np.array_equal(o["summed"], want)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o["state"], out[0]["state"]))
    eng.close()
    assert out[0]["state"][0].tobytes() != c["w"].tobytes()


# ------------------------------------------------------------------------------------------------------------------------ H8
def test_refusals_each_followed_by_a_good_call():
    from dismember_amd import Engine, _native as N
    lib = N.lib()
    K, D, L, E, NI, S, J = 7, 2, 3, 16, 50, 4, 2
    rng = np.random.default_rng(2)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    seq, paths = G.make_batch(rng, K, D, L, S, J, "pad", num_item=NI)
    out = np.empty(D, np.float64)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    i32 = lambda a: None if a is None else a.ctypes.data_as(N.i32p)
    fb = lambda e, s, p, n, j: lib.dm_dr_train_forward_backward_grouped(e._h, i32(s), i32(p), n, j, None)
    ll = lambda e, s, p, n, j: lib.dm_dr_layer_loss(e._h, i32(s), i32(p), n, j, dp)
    eng = Engine(0)
    assert fb(eng, seq, paths, S, J) == STATE and ll(eng, seq, paths, S, J) == STATE          # no model
    assert b"not loaded" in lib.dm_last_error(eng._h)
    eng.dr_load_model(wd, E, L, K, D, NI, dtype=np.float64)
    assert fb(eng, seq, paths, S, J) == STATE                                                 # no training state
    assert b"dm_dr_train_init" in lib.dm_last_error(eng._h)
    d_small = eng.dev_alloc(256)
    assert lib.dm_dr_train_forward_backward_grouped_dev(eng._h, d_small, d_small, S, J, None) == STATE
    assert ll(eng, seq, paths, S, J) == OK                                                    # the loss needs none
    eng.dr_train_init()
    good = lambda: fb(eng, seq, paths, S, J) == OK and ll(eng, seq, paths, S, J) == OK
    assert good()
    for call in (fb, ll):
        bad = paths.copy(); bad[1, 1, 1] = K
        assert call(eng, seq, bad, S, J) == INDEX and good()
        bad = paths.copy(); bad[0, 0, 0] = -1
        assert call(eng, seq, bad, S, J) == INDEX and good()
        bad = seq.copy(); bad[2, 0] = NI
        assert call(eng, bad, paths, S, J) == INDEX and good()
        bad = seq.copy(); bad[2, 0] = -2
        assert call(eng, bad, paths, S, J) == INDEX and good()
        assert call(eng, seq, paths, 0, J) == INVALID and call(eng, seq, paths, -3, J) == INVALID and good()
        assert call(eng, seq, paths, S, 0) == INVALID and call(eng, seq, paths, S, -1) == INVALID and good()
        assert call(eng, None, paths, S, J) == INVALID and call(eng, seq, None, S, J) == INVALID and good()
    assert lib.dm_dr_layer_loss(eng._h, i32(seq), i32(paths), S, J, None) == INVALID and good()
    # more rows than the launches' grids can number, more slots than 32-bit sort values: refused by name before anything is read
    dev = lambda n, j: lib.dm_dr_train_forward_backward_grouped_dev(eng._h, d_small, d_small, n, j, None)
    assert dev(MAX_ROWS // 2 + 1, 2) == UNSUPPORTED and b"batch too large" in lib.dm_last_error(eng._h) and good()
    assert dev(1, MAX_ROWS + 1) == UNSUPPORTED and dev(MAX_ROWS + 1, 1) == UNSUPPORTED and good()
    assert fb(eng, seq, paths, MAX_ROWS + 1, 1) == UNSUPPORTED and good()                     # (the host twin, before it reads an id)
    assert ll(eng, seq, paths, 1, MAX_ROWS + 1) == UNSUPPORTED and good()
    assert dev(0, J) == INVALID and dev(S, 0) == INVALID and good()
    assert lib.dm_dr_train_forward_backward_grouped_dev(eng._h, None, d_small, S, J, None) == INVALID and good()
    eng.dev_free(d_small)
    # a clone neither trains nor evaluates
    cl = eng.clone()
    assert fb(cl, seq, paths, S, J) == STATE and b"clone" in lib.dm_last_error(cl._h)
    assert ll(cl, seq, paths, S, J) == STATE and b"clone" in lib.dm_last_error(cl._h)
    cl.close()
    assert good()
    eng.close()


def test_slot_count_at_two_to_the_31_is_refused():
    """S L + S J (D - 1) >= 2^31 with S J within the row limit: L = 1024, so 2 097 152 samples of one path give 2^31 + 2^21 slots"""
    from dismember_amd import _native as N
    lib = N.lib()
    K, D, L, E, NI = 3, 2, 1024, 16, 8
    wd = synth.make_dr_model(NI, K, D, L, E, np.random.default_rng(0))
    eng = engine_for(wd, (E, L, K, D, NI), np.float32)
    d_small = eng.dev_alloc(256)
    assert lib.dm_dr_train_forward_backward_grouped_dev(eng._h, d_small, d_small, 1 << 21, 1, None) == UNSUPPORTED
    assert b"2^31" in lib.dm_last_error(eng._h)
    eng.dev_free(d_small)
    seq, paths = G.make_batch(np.random.default_rng(1), K, D, L, 2, 2, "pad", num_item=NI)
    assert np.isfinite(eng.dr_train_forward_backward_grouped(seq, paths)).all()
    eng.close()
