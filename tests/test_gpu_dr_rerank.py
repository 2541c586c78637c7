"""GPU tests of the rerank model's training step (dm_dr_rerank_*) against tests/dr_rerank_ref.py.

G1 gradient and loss per case within |gpu - ref| <= k[tensor] eps_T A (k: tests/golden/dr_rerank_tolerances.json, measured on the CPU),
G2 accumulate / replace, G3 reproducibility, G4 the sampler, G5 Adam wiring, G6 serving after training, G7 layer and rerank steps
interleaved, G8 the full-softmax loss, G9 it learns, G10 refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dr_rerank_ref as R
from dismember_amd import synth
from dismember_amd.dr_train import DRTrainer, split_rerank

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = json.load(open(os.path.join(GOLDEN, "dr_rerank_tolerances.json")))
OK, INVALID, STATE, INDEX, UNSUPPORTED = 0, -1, -3, -4, -5
GRAPH = ("rerank_emb", "rerank_w", "rerank_b")


def engine_for(weights, dims, layer, dtype, S=None, **kw):
    """an engine holding the model; S: also the rerank training state"""
    from dismember_amd import Engine
    (E, L, NI), (K, D) = dims, layer
    eng = Engine(0)
    eng.dr_load_model(weights, E, L, K, D, NI, dtype=dtype)
    if S is not None:
        eng.dr_rerank_train_init(S, **kw)
    return eng


def case_engine(name, **kw):
    c = R.make_case(name)
    return c, engine_for(c["weights"], c["dims"], c["layer"], R.NP[c["dtype"]], S=c["S"], **kw)


def grads(eng):
    d = eng.dr_dims
    return split_rerank(eng.dr_rerank_download("graph", "grad"), eng.dr_rerank_download("softmax", "grad"), d["E"], d["L"], d["num_item"])


def state_bytes(eng):
    return [eng.dr_rerank_download(v, w).tobytes() for v in ("graph", "softmax") for w in ("weights", "grad", "s", "r")]


# ------------------------------------------------------------------------------------------------------------------------ G1
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gradient_and_loss_against_the_restatement(name):
    c, eng = case_engine(name)
    ref = R.reference(name)
    dt = c["dtype"]
    eps, k = R.EPS[dt], TOL[dt]["k"]
    loss = eng.dr_rerank_forward_backward(c["seq"], c["targets"], c["negatives"])
    got = grads(eng)
    eng.close()
    ratios, zeros_exact = R.ratios({n: v.astype(np.float64) for n, v in got.items()}, ref, eps)
    loss_ratio = abs(loss - ref["loss"]) / (eps * ref["A_loss"])
    print("%s: ratio / bound  %s  loss %.3g / %.3g" % (name, "  ".join("%s %.3g / %.3g" % (t, ratios[t], k[t]) for t in R.TENSORS), loss_ratio, k["loss"]))
    assert zeros_exact                      # what received nothing is exactly zero (padding, rows nobody named)
    for t in R.TENSORS:
        assert ratios[t] <= k[t], (t, ratios[t], k[t])
    assert loss_ratio <= k["loss"], (loss, ref["loss"])


# ------------------------------------------------------------------------------------------------------------------------ G2
@pytest.mark.parametrize("accumulate", [True, False])
def test_softmax_gradient_accumulates_or_is_replaced(accumulate):
    c, eng = case_engine("b63-f64", accumulate=accumulate)
    rng = np.random.default_rng(4)
    E, L, NI = c["dims"]
    seq2, tg2, neg2 = R.make_batch(rng, L, 40, c["S"], "pad")
    ref1 = R.reference("b63-f64")
    ref2 = R.step(c["weights"], c["dims"], seq2, tg2, neg2)
    eng.dr_rerank_forward_backward(c["seq"], c["targets"], c["negatives"])
    eng.dr_rerank_forward_backward(seq2, tg2, neg2)
    got = grads(eng)
    fresh = engine_for(c["weights"], c["dims"], c["layer"], np.float64, S=c["S"], accumulate=accumulate)
    fresh.dr_rerank_forward_backward(seq2, tg2, neg2)
    alone = grads(fresh)
    for t in GRAPH:                                              # zeroGradParameters: the graph's gradient is the second batch's alone
        assert got[t].tobytes() == alone[t].tobytes()
    eps, k = R.EPS["f64"], TOL["f64"]["k"]
    for t in ("softmax_w", "softmax_b"):
        if accumulate:
            want, A = ref1["g"][t] + ref2["g"][t], ref1["A"][t] + ref2["A"][t]
            assert (np.abs(got[t] - want) <= k[t] * eps * A).all()
            assert (got[t][A == 0] == 0).all() and (got[t][ref1["A"][t] > 0] != 0).all()
        else:
            assert got[t].tobytes() == alone[t].tobytes()
            only_first = (ref1["A"][t] > 0) & (ref2["A"][t] == 0)
            assert only_first.any() and (got[t][only_first] == 0).all()
    eng.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------------------------ G3
@pytest.mark.parametrize("name,accumulate", [("l13-s64-f32", True), ("b513-same-f64", True), ("b65-s63-f32", False)])
def test_three_steps_are_reproducible_to_the_byte(name, accumulate):
    c = R.make_case(name)
    rng = np.random.default_rng(7)
    E, L, NI = c["dims"]
    batches = [(c["seq"], c["targets"], c["negatives"])] + [R.make_batch(rng, L, c["B"], c["S"], "pad")[:2] + (None,) for _ in range(2)]
    runs = []
    for _ in range(2):
        _, eng = case_engine(name, lr=1e-2, seed=99, accumulate=accumulate)
        losses = []
        for seq, tg, neg in batches:                             # the last two draw their negatives on the device
            losses.append(eng.dr_rerank_forward_backward(seq, tg, neg))
            g = eng.dr_rerank_download("softmax", "grad").tobytes()
            eng.dr_rerank_adam_step(1.0)
        runs.append([losses, g] + state_bytes(eng))
        eng.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------------------------------ G4
@pytest.mark.parametrize("name", sorted(R.SAMPLER_CASES))
def test_sampler_equals_the_restated_sampler(name):
    """id = ((draw >> 32) * num_item) >> 32 over draw = splitmix(key(row) + k * 32 + attempt): tests/dr_rerank_ref.py sample_row"""
    N, S, B = R.SAMPLER_CASES[name]
    tg = R.sampler_targets(name)
    E, L, K, D = 16, 1, 4, 2
    wd = synth.make_dr_model(N, K, D, L, E, np.random.default_rng(0))
    drawn = []
    for i, seed in enumerate(R.SAMPLER_SEEDS):
        eng = engine_for(wd, (E, L, N), (K, D), np.float32, S=S, seed=seed)
        rows = B if i == 0 else min(B, 256)
        for step, n in ((0, rows), (1, min(B, 256))):
            got = eng.dr_rerank_sample(np.array(tg[:n], np.int32), step)
            assert (got == R.sample(seed, step, tg[:n], S, N)[0]).all(), (seed, step)
            drawn.append(got[:min(B, 256)].tobytes())
        if i == 0:
            # forward/backward call number n draws with step n: the same bytes as the given negatives of dm_dr_rerank_sample
            seq = np.array(tg[:64], np.int32).reshape(-1, 1)
            t64 = np.array(tg[:64], np.int32)
            l0 = eng.dr_rerank_forward_backward(seq, t64)
            g0 = eng.dr_rerank_download("softmax", "grad").tobytes()
            l1 = eng.dr_rerank_forward_backward(seq, t64)
            other = engine_for(wd, (E, L, N), (K, D), np.float32, S=S, seed=seed)
            assert other.dr_rerank_forward_backward(seq, t64, R.sample(seed, 0, tg[:64], S, N)[0]) == l0
            assert other.dr_rerank_download("softmax", "grad").tobytes() == g0
            assert other.dr_rerank_forward_backward(seq, t64, R.sample(seed, 1, tg[:64], S, N)[0]) == l1
            other.close()
        eng.close()
    assert len(set(drawn)) == (4 if N > 3 else len(set(drawn)))          # two seeds, two steps: four different draws


# ------------------------------------------------------------------------------------------------------------------------ G5
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_adam_wiring(dt):
    E, L, NI, B, S, K, D = 16, 4, R.NUM_ITEM, 8, 4, 4, 2
    dims, T = (E, L, NI), R.NP[dt]
    rng = np.random.default_rng(11)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    seq, tg, neg = R.make_batch(rng, L, B, S, "pad")
    b1, b2, gs = 0.9, 0.999, 0.5
    out = {}
    for mode in ("rows", "dense"):
        eng = engine_for(wd, dims, (K, D), T, S=S, lr=1e-2, accumulate=False)
        w0 = split_rerank(eng.dr_rerank_download("graph"), eng.dr_rerank_download("softmax"), E, L, NI)
        eng.dr_rerank_forward_backward(seq, tg, neg)
        g = grads(eng)
        if mode == "dense":
            os.environ["DM_ADAM_DENSE"] = "1"
        try:
            eng.dr_rerank_adam_step(gs)
        finally:
            os.environ.pop("DM_ADAM_DENSE", None)
        out[mode] = state_bytes(eng)
        w1 = split_rerank(eng.dr_rerank_download("graph"), eng.dr_rerank_download("softmax"), E, L, NI)
        s = split_rerank(eng.dr_rerank_download("graph", "s"), eng.dr_rerank_download("softmax", "s"), E, L, NI)
        r = split_rerank(eng.dr_rerank_download("graph", "r"), eng.dr_rerank_download("softmax", "r"), E, L, NI)
        assert all((v == 0).all() for v in grads(eng).values())              # accumulate = 0: the step zeroed what it visited
        eng.close()
    named = np.zeros(NI, bool); named[seq[seq >= 0]] = True
    cls = np.zeros(NI, bool); cls[tg] = True; cls[neg.ravel()] = True
    assert 4 * named.sum() < NI and 4 * cls.sum() < NI                       # few enough rows for the active-rows path
    for t, live in (("rerank_emb", named), ("softmax_w", cls), ("softmax_b", cls)):
        assert w0[t][~live].tobytes() == w1[t][~live].tobytes()
        assert (s[t][~live] == 0).all() and (r[t][~live] == 0).all()
        assert (w0[t][live] != w1[t][live]).reshape(live.sum(), -1).any(axis=1).all()
    for t in R.TENSORS:
        sg = T(gs) * g[t]
        for got, exp in ((s[t], T(1 - b1) * sg), (r[t], T(1 - b2) * (sg * sg))):
            assert (np.abs(got - exp) <= 2 * np.spacing(np.abs(exp))).all(), t
    assert out["rows"] == out["dense"]


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_reinit_resets_the_optimizer_state(dt):
    """dm_dr_rerank_train_init on a handle that has trained: both vectors' gradient (the criterion's accumulates), moments, time steps,
    active rows and remembered rows start over, and so does the sampler's call count.  Two steps, init again, one step on the FIRST
    batch with negatives drawn on the device: every buffer equals, byte for byte, a fresh engine's that was loaded with the weights
    at re-init; and a fresh engine's under DM_ADAM_DENSE=1 — a list that kept its bits but lost its count would leave the first
    batch's rows out of the rows path."""
    c = R.make_case("tiny-" + dt)                                            # E = 16, L = 1, B = 1
    E, L, NI = c["dims"]
    T, S = R.NP[dt], 1
    kw = dict(lr=1e-2, lr_decay=0.5, seed=5)
    rng = np.random.default_rng(14)
    first = (c["seq"], c["targets"])
    other = R.make_batch(rng, L, 3, S, "pad")

    def one_step(eng, dense=False):
        loss = eng.dr_rerank_forward_backward(*first)                        # the sampler's step 0 on a new training state
        g = [eng.dr_rerank_download(v, "grad").tobytes() for v in ("graph", "softmax")]
        if dense:
            os.environ["DM_ADAM_DENSE"] = "1"
        try:
            eng.dr_rerank_adam_step(1.0)
        finally:
            os.environ.pop("DM_ADAM_DENSE", None)
        return [loss] + g + state_bytes(eng)

    eng = engine_for(c["weights"], c["dims"], c["layer"], T, S=S, **kw)
    for batch in (first + (c["negatives"][:, :S],), other):
        eng.dr_rerank_forward_backward(*batch)
        eng.dr_rerank_adam_step(1.0)
    eng.dr_rerank_forward_backward(*other)                                   # gradients and remembered rows the new run must not see
    w_at = dict(c["weights"])
    w_at.update(split_rerank(eng.dr_rerank_download("graph"), eng.dr_rerank_download("softmax"), E, L, NI))
    eng.dr_rerank_train_init(S, **kw)
    assert all((eng.dr_rerank_download(v, w) == 0).all() for v in ("graph", "softmax") for w in ("grad", "s", "r"))
    got = one_step(eng)
    eng.close()
    for dense in (False, True):
        fresh = engine_for(w_at, c["dims"], c["layer"], T, S=S, **kw)
        want = one_step(fresh, dense)
        fresh.close()
        assert got == want, "dense twin" if dense else "fresh engine"


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("accumulate", [True, False])
def test_the_softmax_tables_have_their_own_optimizer(dt, accumulate):
    """graph options lr_decay = 0.5, eps 1e-8; the criterion's default: the same lr, NO decay, eps 1e-7.  Two steps: the softmax tables
    follow Adam with the criterion's options on the device's own gradients (accumulated or not), the graph follows the decayed one."""
    E, L, NI, B, S, K, D = 16, 4, R.NUM_ITEM, 8, 4, 4, 2
    T, lr = R.NP[dt], 1e-2
    rng = np.random.default_rng(12)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    eng = engine_for(wd, (E, L, NI), (K, D), T, S=S, lr=lr, lr_decay=0.5, accumulate=accumulate)
    w = {v: eng.dr_rerank_download(v) for v in ("graph", "softmax")}
    alt = {n: w["softmax"].copy() for n in ("eps 1e-8", "decayed")}
    mom = {n: (np.zeros_like(w["graph" if n == "graph" else "softmax"]), np.zeros_like(w["graph" if n == "graph" else "softmax"]))
           for n in ("graph", "softmax", "eps 1e-8", "decayed")}
    for t in (1, 2):
        eng.dr_rerank_forward_backward(*R.make_batch(rng, L, B, S, "pad"))
        g = {v: eng.dr_rerank_download(v, "grad") for v in ("graph", "softmax")}
        eng.dr_rerank_adam_step(1.0)
        R.adam_update(w["graph"], g["graph"], *mom["graph"], t, lr, eps=1e-8, lr_decay=0.5)
        R.adam_update(w["softmax"], g["softmax"], *mom["softmax"], t, lr, eps=1e-7)
        R.adam_update(alt["eps 1e-8"], g["softmax"], *mom["eps 1e-8"], t, lr, eps=1e-8)
        R.adam_update(alt["decayed"], g["softmax"], *mom["decayed"], t, lr, eps=1e-7, lr_decay=0.5)
        after = eng.dr_rerank_download("softmax", "grad")
        assert (after == (g["softmax"] if accumulate else 0)).all()          # the accumulating criterion's gradient survives its Adam
    got = {v: eng.dr_rerank_download(v) for v in ("graph", "softmax")}
    eng.close()
    tol = lambda a: 4 * np.spacing(np.maximum(np.abs(a), T(2 * lr)).astype(T))       # a step moves a weight by about lr: four ulp of that, or of the weight
    for v in ("graph", "softmax"):
        assert (np.abs(got[v] - w[v]) <= tol(w[v])).all(), v
    for n, a in alt.items():
        assert (np.abs(got["softmax"] - a) > tol(a)).any(), n


# ------------------------------------------------------------------------------------------------------------------------ G6, G7
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_serving_after_training_and_interleaved_steps(dt):
    from dismember_amd.dr_train import split_params
    K, D, L, E, NI, J, beam, topk = 12, 2, 4, 16, 80, 2, 6, 10
    T = R.NP[dt]
    rng = np.random.default_rng(9)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    wd = {k: ([a.astype(T) for a in v] if isinstance(v, list) else v.astype(T)) for k, v in wd.items()}
    item_paths = synth.make_dr_paths(NI, K, D, J, rng)
    pi = synth.dr_path_items(item_paths)
    seqs = rng.integers(0, NI, size=(5, 32, L)).astype(np.int32)
    seqs[rng.random(seqs.shape) < 0.1] = -1
    targets = rng.integers(0, NI, size=(5, 32))
    users = seqs[0, :12]
    a = engine_for(wd, (E, L, NI), (K, D), T)
    a.dr_load_path_items(*pi)
    before = a.dr_recommend(users, beam, topk)
    tr = DRTrainer(a, item_paths, lr=5e-2, rerank=True, num_sampled=8, seed=3)
    for s, t in zip(seqs, targets):
        layer_loss, rr_loss = tr.step(s, t)
        assert layer_loss.shape == (D,) and np.isfinite(rr_loss)
    assert len(tr.rerank_losses) == 5
    # G7: the layer model moved exactly as it does without the rerank step
    b = engine_for(wd, (E, L, NI), (K, D), T)
    tr_b = DRTrainer(b, item_paths, lr=5e-2)
    for s, t in zip(seqs, targets):
        assert tr_b.step(s, t).shape == (D,)
    assert a.dr_train_download("weights").tobytes() == b.dr_train_download("weights").tobytes()
    assert b.dr_rerank_download("graph").tobytes() == np.concatenate([wd[k].ravel() for k in GRAPH]).tobytes()      # rerank=False: untouched
    # G6: recommend on the training handle == a fresh engine loaded from the downloaded weights, bit for bit
    new = dict(split_params(a.dr_train_download("weights"), E, L, K, D, NI), **tr.rerank_weights())
    assert all((new[k] != wd[k]).any() for k in R.TENSORS)
    c = engine_for(new, (E, L, NI), (K, D), T)
    c.dr_load_path_items(*pi)
    ra, rc = a.dr_recommend(users, beam, topk), c.dr_recommend(users, beam, topk)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rc))
    assert not all(x.tobytes() == y.tobytes() for x, y in zip(ra, before))
    if dt == "f64":
        from oracle import pyoracle as po
        orc = po.DeepRetrieval(new, E, L, K, D, NI, path_items=pi)
        for u in range(len(users)):
            oi, osc = orc.recommend(users[u], topk, beam)
            assert ra[0][u, :ra[2][u]].tolist() == oi.tolist(), u
            np.testing.assert_allclose(ra[1][u, :ra[2][u]], osc, rtol=1e-9, atol=1e-12)
    # reRankStoppingEpoch: past it the rerank model stands still
    tr.rerank_epochs = 1
    tr.next_epoch()
    frozen = a.dr_rerank_download("softmax").tobytes()
    assert np.isnan(tr.step(seqs[0], targets[0])[1]) and a.dr_rerank_download("softmax").tobytes() == frozen
    tr.close(); tr_b.close()
    for e in (a, b, c):
        e.close()


# ------------------------------------------------------------------------------------------------------------------------ G8
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(R.FULL_CASES))
def test_full_loss_against_the_restatement(name, dt):
    c = R.make_full_case(name, dt)
    ref, A = R.full_loss(c["weights"], c["dims"], c["seq"], c["targets"])
    eng = engine_for(c["weights"], c["dims"], c["layer"], R.NP[dt])
    got = [eng.dr_rerank_full_loss(c["seq"], c["targets"])]
    os.environ["DM_DR_FULL_LOSS_ROWS"] = "64"                  # B = 130: two chunks and a remainder
    try:
        got.append(eng.dr_rerank_full_loss(c["seq"], c["targets"]))
    finally:
        os.environ.pop("DM_DR_FULL_LOSS_ROWS", None)
    eng.close()
    bound = TOL[dt]["k"]["full_loss"] * R.EPS[dt] * A
    print("%s %s: %s ref %.17g, fraction of the bound %s" % (name, dt, got, ref, [abs(g - ref) / bound for g in got]))
    assert all(abs(g - ref) <= bound for g in got)


# ------------------------------------------------------------------------------------------------------------------------ G9
def test_it_learns():
    p = R.learning_problem()
    E, L, NI = p["dims"]
    eng = engine_for(p["weights"], p["dims"], p["layer"], np.float64)
    tr = DRTrainer(eng, np.zeros((NI, 1, 2), np.int32), lr=p["lr"], rerank=True, num_sampled=p["S"], seed=p["sampler_seed"])
    first_full = tr.evaluate_rerank(p["seqs"], p["targets"])
    for _ in range(p["steps"]):
        tr.step(p["seqs"], p["targets"])
    first, last, last_full = tr.rerank_losses[0], tr.rerank_losses[-1], tr.evaluate_rerank(p["seqs"], p["targets"])
    print("sampled loss %.4f -> %.4f, full loss %.4f -> %.4f" % (first, last, first_full, last_full))
    assert last < p["fraction"] * first and last_full < p["fraction"] * first_full
    tr.close(); eng.close()


# ------------------------------------------------------------------------------------------------------------------------ G10
def test_refusals():
    from dismember_amd import Engine, _native as N
    lib = N.lib()
    K, D, L, E, NI, B, S = 4, 2, 3, 16, 50, 4, 5
    rng = np.random.default_rng(2)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    seq, tg, neg = R.make_batch(rng, L, B, S, "pad", num_item=NI)
    opts = N.AdamOpts(1e-3, 0.0, 0.9, 0.999, 1e-8)
    i32 = lambda a: None if a is None else a.ctypes.data_as(N.i32p)
    init = lambda e, s, g=opts: lib.dm_dr_rerank_train_init(e._h, None if g is None else C.byref(g), None, s, 1, 1)
    fb = lambda e, s, t, n, b: lib.dm_dr_rerank_forward_backward(e._h, i32(s), i32(t), i32(n), b, None)
    out = np.empty((B, S), np.int32)
    one = C.c_double(0.0)
    eng = Engine(0)
    assert init(eng, S) == STATE                                                      # no model yet
    no_rr = {k: v for k, v in wd.items() if k not in R.TENSORS}
    eng.dr_load_model(no_rr, E, L, K, D, NI, dtype=np.float64)
    assert init(eng, S) == STATE and b"rerank" in lib.dm_last_error(eng._h)           # a model without the five rerank arrays
    assert lib.dm_dr_rerank_full_loss(eng._h, i32(seq), i32(tg), B, C.byref(one)) == STATE
    eng.dr_load_model(wd, E, L, K, D, NI, dtype=np.float64)
    assert fb(eng, seq, tg, neg, B) == STATE and lib.dm_dr_rerank_adam_step(eng._h, 1.0) == STATE      # no training state yet
    assert lib.dm_dr_rerank_sample(eng._h, i32(tg), B, 0, i32(out)) == STATE
    assert lib.dm_dr_rerank_full_loss(eng._h, i32(seq), i32(tg), B, C.byref(one)) == OK                # needs none
    assert init(eng, S, None) == INVALID
    assert init(eng, 0) == INVALID and init(eng, NI) == INVALID and init(eng, -1) == INVALID
    assert init(eng, NI - 1) == OK and fb(eng, seq, tg, None, B) == UNSUPPORTED                        # 2 S > num_item: pass the negatives
    assert b"pass the negatives" in lib.dm_last_error(eng._h)
    assert lib.dm_dr_rerank_sample(eng._h, i32(tg), B, 0, i32(np.empty((B, NI - 1), np.int32))) == UNSUPPORTED
    assert init(eng, S) == OK
    assert fb(eng, seq, tg, neg, B) == OK and fb(eng, seq, tg, None, B) == OK
    for arr, which in ((seq, 0), (tg, 1), (neg, 2)):
        for v in (NI, -2 if which == 0 else -1):
            bad = arr.copy(); bad.ravel()[1] = v
            args = [seq, tg, neg]; args[which] = bad
            assert fb(eng, *args, B) == INDEX, (which, v)
    assert fb(eng, seq, tg, neg, 0) == INVALID and fb(eng, seq, tg, neg, -3) == INVALID
    assert fb(eng, None, tg, neg, B) == INVALID and fb(eng, seq, None, neg, B) == INVALID
    bad = tg.copy(); bad[0] = NI
    assert lib.dm_dr_rerank_sample(eng._h, i32(bad), B, 0, i32(out)) == INDEX
    assert lib.dm_dr_rerank_sample(eng._h, i32(tg), B, 0, None) == INVALID
    # more rows than the launches' grids can number: refused by name before anything is read (the arrays here are far too short)
    d_small = eng.dev_alloc(256)
    assert lib.dm_dr_rerank_forward_backward_dev(eng._h, d_small, d_small, d_small, 65535 * 64 + 1, None) == UNSUPPORTED
    assert b"batch too large" in lib.dm_last_error(eng._h)
    eng.dev_free(d_small)
    n = eng.dr_rerank_sizes()
    assert n == {"graph": NI * E + E * L * E + E, "softmax": NI * E + NI}
    buf = np.empty(n["graph"] + 1, np.float64)
    vp = buf.ctypes.data_as(C.c_void_p)
    assert lib.dm_dr_rerank_download(eng._h, 0, 1, vp, n["graph"] + 1) == INVALID and lib.dm_dr_rerank_download(eng._h, 0, 1, vp, n["softmax"]) == INVALID
    assert lib.dm_dr_rerank_download(eng._h, 1, 1, vp, n["graph"]) == INVALID and lib.dm_dr_rerank_download(eng._h, 2, 0, vp, n["graph"]) == INVALID
    assert lib.dm_dr_rerank_download(eng._h, 0, 4, vp, n["graph"]) == INVALID and lib.dm_dr_rerank_download(eng._h, 0, 1, None, n["graph"]) == INVALID
    assert lib.dm_dr_rerank_download(eng._h, 0, 1, vp, n["graph"]) == OK and lib.dm_dr_rerank_download(eng._h, 1, 3, vp, n["softmax"]) == OK
    # the cap of a wave's registers
    big = synth.make_dr_model(300, K, D, L, E, rng)
    e2 = Engine(0)
    e2.dr_load_model(big, E, L, K, D, 300, dtype=np.float32)
    assert init(e2, 256) == UNSUPPORTED and init(e2, 255) == OK
    e2.close()
    # a clone neither trains nor initialises training
    cl = eng.clone()
    assert init(cl, S) == STATE and b"clone" in lib.dm_last_error(cl._h)
    assert fb(cl, seq, tg, neg, B) == STATE and lib.dm_dr_rerank_adam_step(cl._h, 1.0) == STATE and lib.dm_dr_rerank_train_free(cl._h) == STATE
    assert lib.dm_dr_rerank_sample(cl._h, i32(tg), B, 0, i32(out)) == STATE and lib.dm_dr_rerank_full_loss(cl._h, i32(seq), i32(tg), B, C.byref(one)) == STATE
    assert lib.dm_dr_rerank_download(cl._h, 0, 0, vp, n["graph"]) == STATE
    cl.close()
    # the two training states are independent; free and load drop this one
    eng.dr_train_init()
    eng.dr_rerank_train_free()
    assert fb(eng, seq, tg, neg, B) == STATE and lib.dm_dr_rerank_download(eng._h, 0, 0, vp, n["graph"]) == OK
    assert lib.dm_dr_train_forward_backward(eng._h, i32(seq), i32(np.zeros((B, D), np.int32)), B, None) == OK
    assert init(eng, S) == OK
    eng.dr_train_free()
    assert fb(eng, seq, tg, neg, B) == OK
    eng.dr_load_model(wd, E, L, K, D, NI, dtype=np.float64)
    assert fb(eng, seq, tg, neg, B) == STATE
    eng.close()
