"""GPU tests of the Deep-Retrieval training step (dm_dr_train_*, dm_dr_adam_step) against tests/dr_train_ref.py.

G1 gradient and loss per case within |gpu - ref| <= k[tensor] eps_T A (k: tests/golden/dr_train_tolerances.json, measured on the CPU),
G2 reproducibility, G3 Adam wiring, G4 the search's derived copies after training, G5 it learns, G6 refusals, G7 one E/M round."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dr_train_ref as R
from dismember_amd import synth
from dismember_amd.dr_train import DRTrainer, expand_batch, pack_params, param_sections, split_params

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = json.load(open(os.path.join(GOLDEN, "dr_train_tolerances.json")))
OK, INVALID, STATE, INDEX, UNSUPPORTED = 0, -1, -3, -4, -5


def engine_for(weights, dims, dtype, train=True, **adam):
    from dismember_amd import Engine
    E, L, K, D, NI = dims
    eng = Engine(0)
    eng.dr_load_model(weights, E, L, K, D, NI, dtype=dtype)
    if train:
        eng.dr_train_init(**adam)
    return eng


def case_engine(name, **adam):
    c = R.make_case(name)
    return c, engine_for(split_params(c["w"], *c["dims"]), c["dims"], R.NP[c["dtype"]], **adam)


# ------------------------------------------------------------------------------------------------------------------------ G1
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gradient_and_loss_against_the_restatement(name):
    c, eng = case_engine(name)
    ref = R.reference(name)
    dt, D, K = c["dtype"], c["dims"][3], c["dims"][2]
    eps, k = R.EPS[dt], TOL[dt]["k"]
    loss = eng.dr_train_forward_backward(c["seq"], c["paths"])
    g = eng.dr_train_download("grad")
    eng.close()
    ratios, zeros_exact = R.class_ratios(g.astype(np.float64), ref, eps, c["dims"])
    loss_ratio = float((np.abs(loss - ref["loss"]) / np.where(ref["A_loss"] > 0, eps * D * ref["A_loss"], 1.0)).max())
    print("%s: ratio / bound  %s  loss %.3g / %.3g" % (name, "  ".join("%s %.3g / %.3g" % (t, ratios[t], k[t]) for t in R.CLASSES), loss_ratio, k["loss"]))
    assert zeros_exact                      # what received nothing is exactly zero (padding, rows nobody named)
    if K == 1:
        assert (g == 0).all() and (loss == 0).all()
    for t in R.CLASSES:
        assert ratios[t] <= k[t], (t, ratios[t], k[t])
    assert loss_ratio <= k["loss"], (loss, ref["loss"])


def test_forward_backward_replaces_the_gradient():
    """zeroGradParameters: a second batch's gradient does not contain the first's"""
    c, eng = case_engine("all-pad-row-f64")
    other = R.make_case("above-tile-f64")
    seq2 = other["seq"][:, :1].repeat(c["dims"][1], axis=1)[:40]
    paths2 = np.ascontiguousarray(c["paths"][:40][::-1])
    eng.dr_train_forward_backward(c["seq"], c["paths"])
    eng.dr_train_forward_backward(seq2, paths2)
    g2 = eng.dr_train_download("grad")
    fresh = engine_for(split_params(c["w"], *c["dims"]), c["dims"], np.float64)
    fresh.dr_train_forward_backward(seq2, paths2)
    assert g2.tobytes() == fresh.dr_train_download("grad").tobytes()


# ------------------------------------------------------------------------------------------------------------------------ G2
@pytest.mark.parametrize("name", ["cache-13-f32", "same-row-f64", "slab-513-f32"])
def test_three_steps_are_reproducible_to_the_byte(name):
    c = R.make_case(name)
    rng = np.random.default_rng(7)
    K, D, L = c["dims"][2], c["dims"][3], c["dims"][1]
    batches = [(c["seq"], c["paths"])] + [R.make_batch(rng, K, D, L, c["B"], "pad") for _ in range(2)]
    runs = []
    for _ in range(2):
        _, eng = case_engine(name, lr=1e-2)
        for seq, paths in batches:
            eng.dr_train_forward_backward(seq, paths)
            g = eng.dr_train_download("grad")
            eng.dr_adam_step(1.0)
        runs.append([g.tobytes()] + [eng.dr_train_download(w).tobytes() for w in ("weights", "grad", "s", "r")])
        eng.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------------------ G3
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_adam_wiring(dt):
    K, D, L, E, NI, B = 7, 3, 4, 16, R.NUM_ITEM, 8
    dims, T = (E, L, K, D, NI), R.NP[dt]
    rng = np.random.default_rng(11)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    seq, paths = R.make_batch(rng, K, D, L, B, "pad")
    b1, b2, gs = 0.9, 0.999, 0.5
    out = {}
    for mode in ("rows", "dense"):
        eng = engine_for(wd, dims, T, lr=1e-2, beta1=b1, beta2=b2)
        w0 = eng.dr_train_download("weights")
        eng.dr_train_forward_backward(seq, paths)
        g = eng.dr_train_download("grad")
        if mode == "dense":
            os.environ["DM_ADAM_DENSE"] = "1"
        try:
            eng.dr_adam_step(gs)
        finally:
            os.environ.pop("DM_ADAM_DENSE", None)
        out[mode] = [eng.dr_train_download(w) for w in ("weights", "s", "r")]
        assert (eng.dr_train_download("grad") == 0).all()
        eng.close()
    w1, s, r = out["rows"]
    sec = param_sections(*dims)
    case = dict(dims=dims, seq=seq, paths=paths)
    touched = R.touched_rows(case)
    assert 4 * touched.sum() < len(touched)                                 # few enough rows for the active-rows path
    emb0, emb1 = (v[slice(*sec["emb"])].reshape(-1, E) for v in (w0, w1))
    assert emb0[~touched].tobytes() == emb1[~touched].tobytes()
    assert (emb0[touched] != emb1[touched]).any(axis=1).all()
    sg = T(gs) * g
    for got, exp in ((s, T(1 - b1) * sg), (r, T(1 - b2) * (sg * sg))):
        assert (np.abs(got - exp) <= 2 * np.spacing(np.abs(exp))).all()
    for a, b in zip(out["rows"], out["dense"]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_reinit_resets_the_optimizer_state(dt):
    """dm_dr_train_init on a handle that has trained: gradient, both moments, the time step, the active rows and the remembered rows of
    the last batch all start over.  Two steps, init again, one step on the FIRST batch (rows the old run had listed): every buffer
    equals, byte for byte, a fresh engine's that was loaded with the weights at re-init; and a fresh engine's under DM_ADAM_DENSE=1 —
    a list that kept its bits but lost its count would leave those rows out of the rows path."""
    K, D, L, E, NI, B = 7, 3, 4, 16, R.NUM_ITEM, 8
    dims, T = (E, L, K, D, NI), R.NP[dt]
    rng = np.random.default_rng(13)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    batches = [R.make_batch(rng, K, D, L, B, "pad") for _ in range(2)]
    adam = dict(lr=1e-2, lr_decay=0.5)
    assert 4 * R.touched_rows(dict(dims=dims, seq=batches[0][0], paths=batches[0][1])).sum() < NI + K * (D - 1)      # the rows path

    def one_step(eng, dense=False):
        eng.dr_train_forward_backward(*batches[0])
        g = eng.dr_train_download("grad").tobytes()
        if dense:
            os.environ["DM_ADAM_DENSE"] = "1"
        try:
            eng.dr_adam_step(1.0)
        finally:
            os.environ.pop("DM_ADAM_DENSE", None)
        return [g] + [eng.dr_train_download(w).tobytes() for w in ("weights", "grad", "s", "r")]

    eng = engine_for(wd, dims, T, **adam)
    for seq, paths in batches:
        eng.dr_train_forward_backward(seq, paths)
        eng.dr_adam_step(1.0)
    eng.dr_train_forward_backward(*batches[1])                               # a gradient and remembered rows the new run must not see
    w_at = eng.dr_train_download("weights")
    eng.dr_train_init(**adam)
    assert eng.dr_train_download("weights").tobytes() == w_at.tobytes()
    assert all((eng.dr_train_download(w) == 0).all() for w in ("grad", "s", "r"))
    got = one_step(eng)
    eng.close()
    for dense in (False, True):
        fresh = engine_for(split_params(w_at, *dims), dims, T, **adam)
        want = one_step(fresh, dense)
        fresh.close()
        assert got == want, "dense twin" if dense else "fresh engine"


# ------------------------------------------------------------------------------------------------------------------------ G4
@pytest.fixture(params=["one_kernel", "sliced"])
def search_path(request):
    if request.param == "sliced":
        os.environ["DM_DR_SLICED_MIN_USERS"] = "1"                       # read at model load
    yield request.param
    os.environ.pop("DM_DR_SLICED_MIN_USERS", None)


@pytest.mark.parametrize("dt,E", [("f64", 16), ("f32", 64)])
def test_derived_copies_follow_the_trained_weights(search_path, dt, E):
    K, D, L, NI, B, beam, topk = 40, 3, 5, 300, 96, 8, 10
    dims, T = (E, L, K, D, NI), R.NP[dt]
    rng = np.random.default_rng(21)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    wd = {k: ([a.astype(T) for a in v] if isinstance(v, list) else v.astype(T)) for k, v in wd.items()}
    pi = synth.dr_path_items(synth.make_dr_paths(NI, K, D, 2, rng))
    users = rng.integers(0, NI, size=(24, L)).astype(np.int32)
    users[rng.random(users.shape) < 0.2] = -1
    users[0] = -1
    a = engine_for(wd, dims, T, lr=5e-2)
    a.dr_load_path_items(*pi)
    before = a.dr_beam_search(users, beam)
    for _ in range(3):
        a.dr_train_forward_backward(*R.make_batch(rng, K, D, L, B, "pad", num_item=NI))
        a.dr_adam_step(1.0)
    trained = split_params(a.dr_train_download("weights"), *dims)
    assert any((x != y).any() for x, y in zip(trained["layer_w"], wd["layer_w"]))
    new = dict(wd, **trained)
    b = engine_for(new, dims, T, train=False)
    b.dr_load_path_items(*pi)
    sa, sb = a.dr_beam_search(users, beam), b.dr_beam_search(users, beam)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(sa, sb))
    assert not all(x.tobytes() == y.tobytes() for x, y in zip(sa, before))          # the search saw the new weights
    ra, rb = a.dr_recommend(users, beam, topk), b.dr_recommend(users, beam, topk)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
    if dt == "f64":
        from oracle import pyoracle as po
        orc = po.DeepRetrieval(new, E, L, K, D, NI, path_items=pi)
        for u in range(len(users)):
            op, ov = orc.beam_search(users[u], beam)
            assert sa[0][u, :sa[2][u]].tolist() == op.tolist(), u
            np.testing.assert_allclose(sa[1][u, :sa[2][u]], ov, rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------------------------------ G5
def test_it_learns():
    p = R.learning_problem()
    eng = engine_for(p["weights"], p["dims"], np.float64, train=False)
    tr = DRTrainer(eng, p["item_paths"], lr=p["lr"])
    for _ in range(p["steps"]):
        tr.step(p["seqs"], p["targets"])
    first, last = tr.losses[0], tr.losses[-1]
    print("losses", first, last)
    assert (last < 0.9 * first).all()


# ------------------------------------------------------------------------------------------------------------------------ G6
def test_refusals():
    from dismember_amd import Engine, _native as N
    lib = N.lib()
    K, D, L, E, NI, B = 7, 2, 3, 16, 50, 4
    dims = (E, L, K, D, NI)
    rng = np.random.default_rng(2)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    seq, paths = R.make_batch(rng, K, D, L, B, "pad", num_item=NI)
    opts = N.AdamOpts(1e-3, 0.0, 0.9, 0.999, 1e-8)
    i32 = lambda a: a.ctypes.data_as(N.i32p)
    fb = lambda e, s, p, n: lib.dm_dr_train_forward_backward(e._h, None if s is None else i32(s), None if p is None else i32(p), n, None)
    eng = Engine(0)
    assert lib.dm_dr_train_init(eng._h, C.byref(opts)) == STATE                       # no model yet
    eng.dr_load_model(wd, E, L, K, D, NI, dtype=np.float64)
    assert fb(eng, seq, paths, B) == STATE                                            # no training state yet
    assert lib.dm_dr_adam_step(eng._h, 1.0) == STATE
    assert lib.dm_dr_train_init(eng._h, None) == INVALID
    eng.dr_train_init()
    assert fb(eng, seq, paths, B) == OK
    bad = paths.copy(); bad[1, 1] = K
    assert fb(eng, seq, bad, B) == INDEX
    bad = paths.copy(); bad[0, 0] = -1
    assert fb(eng, seq, bad, B) == INDEX
    bad = seq.copy(); bad[2, 0] = NI
    assert fb(eng, bad, paths, B) == INDEX
    bad = seq.copy(); bad[2, 0] = -2
    assert fb(eng, bad, paths, B) == INDEX
    assert fb(eng, seq, paths, 0) == INVALID and fb(eng, seq, paths, -3) == INVALID
    assert fb(eng, None, paths, B) == INVALID and fb(eng, seq, None, B) == INVALID
    # more rows than the launches' grids can number: refused by name before anything is read (the arrays here are far too short)
    d_small = eng.dev_alloc(256)
    assert lib.dm_dr_train_forward_backward_dev(eng._h, d_small, d_small, 65535 * 64 + 1, None) == UNSUPPORTED
    assert b"batch too large" in lib.dm_last_error(eng._h)
    eng.dev_free(d_small)
    n = eng.dr_train_param_count()
    assert n == list(param_sections(*dims).values())[-1][1]
    buf = np.empty(n + 1, np.float64)
    assert lib.dm_dr_train_download(eng._h, 1, buf.ctypes.data_as(C.c_void_p), n + 1) == INVALID
    assert lib.dm_dr_train_download(eng._h, 1, buf.ctypes.data_as(C.c_void_p), n - 1) == INVALID
    assert lib.dm_dr_train_download(eng._h, 1, None, n) == INVALID
    assert lib.dm_dr_train_download(eng._h, 1, buf.ctypes.data_as(C.c_void_p), n) == OK
    # a clone neither trains nor initialises training
    cl = eng.clone()
    assert lib.dm_dr_train_init(cl._h, C.byref(opts)) == STATE
    assert b"clone" in lib.dm_last_error(cl._h)
    assert fb(cl, seq, paths, B) == STATE and lib.dm_dr_adam_step(cl._h, 1.0) == STATE and lib.dm_dr_train_free(cl._h) == STATE
    cl.close()
    # after dm_dr_train_free the handle still searches, bit for bit as before
    eng.dr_adam_step(1.0)
    users = seq[:3]
    s0 = eng.dr_beam_search(users, 4)
    eng.dr_train_free()
    assert fb(eng, seq, paths, B) == STATE
    s1 = eng.dr_beam_search(users, 4)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(s0, s1))
    # loading a model drops the training state
    eng.dr_train_init()
    assert fb(eng, seq, paths, B) == OK
    eng.dr_load_model(wd, E, L, K, D, NI, dtype=np.float64)
    assert fb(eng, seq, paths, B) == STATE
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ G7
def test_one_e_step_m_step_round():
    from dismember_amd import dr_mstep
    K, D, L, E, NI, J = 12, 2, 4, 16, 80, 2
    rng = np.random.default_rng(9)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    item_paths = synth.make_dr_paths(NI, K, D, J, rng)
    eng = engine_for(wd, (E, L, K, D, NI), np.float64, train=False)
    tr = DRTrainer(eng, item_paths, lr=1e-2)
    seqs = rng.integers(0, NI, size=(5, 32, L)).astype(np.int32)
    seqs[rng.random(seqs.shape) < 0.1] = -1
    targets = rng.integers(0, NI, size=(5, 32))
    for s, t in zip(seqs, targets):
        loss = tr.step(s, t)
        assert loss.shape == (D,) and np.isfinite(loss).all()
    assert len(tr.losses) == 5 and expand_batch(seqs[0], targets[0], item_paths)[0].shape == (32 * J, L)
    sc = dr_mstep.batch_path_scores(eng, seqs.reshape(-1, L), targets.reshape(-1), 6)
    assert sorted(sc) == sorted(set(targets.reshape(-1).tolist()))
    for codes, scores in sc.values():
        assert len(codes) == len(scores) > 0 and (np.diff(scores) <= 0).all()
