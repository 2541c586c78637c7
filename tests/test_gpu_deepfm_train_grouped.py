"""The user-grouped DeepFM training step on the device (csrc/dfm_train_grouped.hip.inc): loss and gradient against the
float64 ROW step of tests/deepfm_train_ref.py on the expanded rows under |gpu - ref| <= k eps32 A with k from
tests/golden/deepfm_train_grouped_tolerances.json (CPU-derived), the row step on the same batch, determinism, padded columns, serving
after training, the OTM route under DM_DFM_TRAIN_GROUPED=1, refusals and a problem it learns."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import deepfm_ref as R
import deepfm_train_ref as T
import deepfm_train_grouped_ref as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TOL = json.load(open(os.path.join(ROOT, "tests", "golden", "deepfm_train_grouped_tolerances.json")))
K, K_LONG = _TOL["k"], _TOL["k_long_segment"]
K_ROW = json.load(open(os.path.join(ROOT, "tests", "golden", "deepfm_train_tolerances.json")))["k"]


def live_allocs():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


def padded_view(eng, what):
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_deepfm_train_padded
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, N.f32p, N.i64p]
    n = C.c_int64(0)
    assert fn(eng._h, what, None, C.byref(n)) == 0
    out = np.empty(n.value, np.float32)
    assert fn(eng._h, what, out.ctypes.data_as(N.f32p), C.byref(n)) == 0
    return out


def engine(E, L, w, NI=G.NUM_INDEX):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_weights_deepfm(w, E, L, NI)
    return eng


@functools.lru_cache(maxsize=None)
def reference(kind, key):
    """the float64 row step of a case on its expanded rows, computed once"""
    if kind == "shape":
        E, L = key[0], key[1]
        w, seq, codes, y, _ = G.shape_case(*key)
    else:
        E, L = 16, 10
        w, seq, codes, y, _ = G.structure_case(key)
    o = G.row_reference(w, E, L, seq, codes, y)
    for v in (o["g"], o["A"]):
        v.setflags(write=False)
    return (w, E, L, seq, codes, y), o


def within(tag, loss, g, ref, E, L, k):
    assert np.isfinite(loss) and np.isfinite(g).all()
    ratios = T.ratios(g, ref["g"], ref["A"], E, L, G.NUM_INDEX)
    ratios["loss"] = abs(loss - ref["loss"]) / (T.EPS32 * ref["A_loss"])
    print("%s: share of the bound " % (tag,) + " ".join("%s %.3f" % (t, ratios[t] / k[t]) for t in sorted(ratios)))
    for t, v in ratios.items():
        assert v <= k[t], (tag, t, v, k[t])


def check_step(kind, key):
    (w, E, L, seq, codes, y), ref = reference(kind, key)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        loss = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        g = eng.deepfm_train_download("grad")
    finally:
        eng.close()
    within("%s %s" % (kind, key), loss, g, ref, E, L, K_LONG if key == "long_segment" else K)
    return loss, g


# --------------------------------------------------------------------------- gradient and loss
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "E%d-L%d-U%d-R%d" % s)
def test_step_shapes(shape):
    check_step("shape", shape)


def test_step_forced_grid_partial_last_round(monkeypatch):
    monkeypatch.setenv("DM_DFM_TRAIN_GRID", "2")           # 13 user tiles and 38 row tiles over 2 workgroups of 4 waves
    check_step("shape", G.GRID_CASE)


@pytest.mark.parametrize("name", G.STRUCTURES)
def test_step_structures(name):
    (w, E, L, seq, codes, y), ref = reference("structure", name)
    _, g = check_step("structure", name)
    emb = g[:G.NUM_INDEX * E].reshape(-1, E)
    read = np.zeros(G.NUM_INDEX, bool)
    read[codes[codes >= 0]] = True; read[seq[seq >= 0]] = True
    assert not emb[~read].any() and (~read).sum() > 100                      # rows no slot read stay exact zeros


# --------------------------------------------------------------------------- against the row step
def test_grouped_and_row_step_agree_on_the_same_batch():
    (w, E, L, seq, codes, y), ref = reference("shape", (128, 10, 19, 41))
    c, s, yy = G.expand(seq, codes, y)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        lr_ = eng.deepfm_train_forward_backward(c, s, yy)
        gr_ = eng.deepfm_train_download("grad")
        lg = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        gg = eng.deepfm_train_download("grad")
    finally:
        eng.close()
    within("row step", lr_, gr_, ref, E, L, K_ROW)
    within("grouped step", lg, gg, ref, E, L, K)
    print("|grouped loss - row loss| / (eps32 A_loss) = %.3f of %.3f" % (abs(lg - lr_) / (T.EPS32 * ref["A_loss"]), K["loss"]))
    assert abs(lg - lr_) <= K["loss"] * T.EPS32 * ref["A_loss"]                 # the two losses against each other: the one loss bound


# --------------------------------------------------------------------------- determinism
def test_repeats_are_byte_identical_also_forced_grid_and_after_a_row_step(monkeypatch):
    (w, E, L, seq, codes, y), _ = reference("shape", G.GRID_CASE)
    (_, _, _, seq2, codes2, y2), _ = reference("shape", (16, 1, 33, 1))
    c2, s2, yy2 = G.expand(seq2, codes2, y2)
    c2 = (c2 + 500) % G.NUM_INDEX                                            # other rows than the grouped batch reads
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        la = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        a = eng.deepfm_train_download("grad")
        lb = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        assert (la, a.tobytes()) == (lb, eng.deepfm_train_download("grad").tobytes())
        eng.deepfm_train_forward_backward(c2, s2, yy2)                       # a row step in between: its rows are cleared
        assert eng.deepfm_train_download("grad").tobytes() != a.tobytes()
        lc = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        assert (la, a.tobytes()) == (lc, eng.deepfm_train_download("grad").tobytes())
        eng.deepfm_train_forward_backward_grouped(seq2, codes2, y2)          # ... and a grouped step's rows by the row step
        g2 = eng.deepfm_train_download("grad")
        eng.deepfm_train_forward_backward(c2, s2, yy2)
        gr2 = eng.deepfm_train_download("grad")
        eng.deepfm_train_init()
        eng.deepfm_train_forward_backward(c2, s2, yy2)
        assert gr2.tobytes() == eng.deepfm_train_download("grad").tobytes()
        monkeypatch.setenv("DM_DFM_TRAIN_GRID", "2")
        ld = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        d = eng.deepfm_train_download("grad")
        le = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        assert (ld, d.tobytes()) == (le, eng.deepfm_train_download("grad").tobytes())
    finally:
        eng.close()


def test_padded_columns_stay_exact_zeros_after_five_steps():
    E, L, Ep, U, Rr = 24, 1, 32, 37, 9
    w = G.shape_case(24, 1, 1, 1)[0]
    rng = np.random.default_rng(3)
    seq = rng.integers(-1, G.NUM_INDEX, (U, L)).astype(np.int32); codes = rng.integers(0, G.NUM_INDEX, (U, Rr)).astype(np.int32)
    y = (rng.random((U, Rr)) < 0.4).astype(np.float32)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init(lr=0.01)
        for _ in range(5):
            eng.deepfm_train_forward_backward_grouped(seq, codes, y)
            gp = padded_view(eng, 1)
            eng.deepfm_adam_step()
        NI, Tt = G.NUM_INDEX, L + 1
        for what, v in ((0, padded_view(eng, 0)), (1, gp), (2, padded_view(eng, 2)), (3, padded_view(eng, 3))):
            assert v.size == NI * Ep + Tt * Tt * Ep + 2 * Tt + 1
            blocks = v[:NI * Ep + Tt * Tt * Ep].reshape(-1, Ep)
            assert not blocks[:, E:].any(), what
            assert blocks[:, :E].any(), what
    finally:
        eng.close()


# --------------------------------------------------------------------------- serving after training
def test_serving_after_grouped_steps_matches_a_fresh_load():
    import dfm_otm_ref as D
    E, L, beam, leaf = 16, 10, 20, 9
    w, ni = D.model(E, L, 9)
    seqs = D.histories(L, ni, 33)[:8]
    rng = np.random.default_rng(21)
    codes = rng.integers(0, ni, (8, 12)).astype(np.int32)
    y = (rng.random((8, 12)) < 0.3).astype(np.float32)
    eng, fresh = engine(E, L, w, ni), None
    try:
        eng.deepfm_train_init(lr=0.01)
        for _ in range(5):
            assert np.isfinite(eng.deepfm_train_forward_backward_grouped(seqs, codes, y))
            eng.deepfm_adam_step()
        wt = eng.deepfm_train_download("weights")
        assert wt.tobytes() != w.tobytes()
        fresh = engine(E, L, wt, ni)
        c, s, _ = G.expand(seqs, codes, y)
        assert eng.deepfm_forward(c, s).tobytes() == fresh.deepfm_forward(c, s).tobytes()
        for p, q in zip(eng.otm_beam_search(seqs, beam, leaf), fresh.otm_beam_search(seqs, beam, leaf)):
            assert p.tobytes() == q.tobytes()
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()


# --------------------------------------------------------------------------- the OTM route
@pytest.mark.parametrize("mode", ["pseudo", "normal"])
def test_otm_train_batch_under_the_variable_equals_the_grouped_steps(mode, monkeypatch):
    """with DM_DFM_TRAIN_GROUPED=1, dm_deepfm_otm_train_batch == traced search with fixed weights, then per level the batch of the
    restatement through the grouped step and dm_deepfm_adam_step: weights, moments and losses, bit for bit"""
    import dfm_otm_ref as D
    from dismember_amd import Engine
    from dismember_amd.otm_train import OTMTrainer
    E, L, beam, leaf, U = 16, 10, 20, 9, 8
    w, ni = D.model(E, L, 9)
    seqs = D.histories(L, ni, 33)[:U]
    targets = D.ragged_targets(20)[1:1 + U]
    a, b, c = Engine(0), Engine(0), Engine(0)
    try:
        for e in (a, b, c):
            e.load_weights_deepfm(w, E, L, ni)
        monkeypatch.setenv("DM_DFM_TRAIN_GROUPED", "1")
        tr = OTMTrainer(a, leaf_level=leaf, beam=beam, seq_len=L, lr=1e-3)
        losses = tr.train_batch(seqs, targets, mode)
        st = tr.last_stats()
        monkeypatch.setenv("DM_DFM_TRAIN_GROUPED", "0")                       # read per call: 0 is the row step
        losses_row = OTMTrainer(c, leaf_level=leaf, beam=beam, seq_len=L, lr=1e-3).train_batch(seqs, targets, mode)
        monkeypatch.delenv("DM_DFM_TRAIN_GROUPED")
        counts = D.level_counts(beam, leaf)
        assert len(losses) == len(counts) and st["pseudo_target_forward_rows"] == 0 and st["rows_trained"] == U * sum(counts)
        b.deepfm_train_init(lr=1e-3)
        levels = len(counts)
        _, _, _, tc, ts, tn = b.otm_beam_search_trace(seqs, beam, leaf, levels)
        tgt = D.pseudo_targets(targets, beam, leaf, mode)
        want = []
        for it in range(levels):
            codes, rows, labels = D.level_batch(tc, tn, it, tgt[it], seqs)
            assert (tn[:, it] == counts[it]).all()
            want.append(b.deepfm_train_forward_backward_grouped(seqs, codes.reshape(U, -1), labels.reshape(U, -1)))
            b.deepfm_adam_step()
        assert losses == want and all(np.isfinite(losses))
        for what in ("weights", "s", "r"):
            assert a.deepfm_train_download(what).tobytes() == b.deepfm_train_download(what).tobytes(), what
        # "0" is the row step: the bytes of the call without the variable
        b.load_weights_deepfm(w, E, L, ni)
        assert OTMTrainer(b, leaf_level=leaf, beam=beam, seq_len=L, lr=1e-3).train_batch(seqs, targets, mode) == losses_row
        assert b.deepfm_train_download("weights").tobytes() == c.deepfm_train_download("weights").tobytes()
    finally:
        a.close(); b.close(); c.close()


# --------------------------------------------------------------------------- refusals
def test_refusals_keep_the_live_allocation_count():
    from dismember_amd import DismemberError, Engine, _native as N
    import helpers
    (w, E, L, seq, codes, y), ref = reference("structure", "candidate_in_own_history")
    lib = N.lib()
    loss = C.c_double(0)
    U, Rr = codes.shape
    p256 = C.c_void_p(256)
    raw = lambda e, *a: lib.dm_deepfm_train_forward_backward_grouped_dev(e._h, *a, C.byref(loss))

    def refused(code, fn, *a):
        base = live_allocs()
        with pytest.raises(DismemberError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert live_allocs() == base

    eng = Engine(0)
    try:
        refused(-3, eng.deepfm_train_forward_backward_grouped, seq, codes, y)          # no model
        eng.load_weights_din(helpers.random_din_weights(np.random.default_rng(1), E, G.NUM_INDEX), E, G.NUM_INDEX)
        refused(-3, eng.deepfm_train_forward_backward_grouped, seq, codes, y)          # a DIN model
        eng.load_weights_deepfm(w, E, L, G.NUM_INDEX)
        refused(-3, eng.deepfm_train_forward_backward_grouped, seq, codes, y)          # before the init
        eng.deepfm_train_init()
        cl = eng.clone()
        try:
            refused(-3, cl.deepfm_train_forward_backward_grouped, seq, codes, y)       # on a clone
        finally:
            cl.close()
        refused(-1, eng.deepfm_train_forward_backward_grouped, seq[:, :9], codes, y)   # L != the model's
        base = live_allocs()
        assert raw(eng, p256, p256, p256, 0, Rr, L) == -1 and raw(eng, p256, p256, p256, -1, Rr, L) == -1
        assert raw(eng, p256, p256, p256, U, 0, L) == -1
        assert raw(eng, None, p256, p256, U, Rr, L) == -1 and raw(eng, p256, None, p256, U, Rr, L) == -1 and raw(eng, p256, p256, None, U, Rr, L) == -1
        # too large: refused before anything is read (the arrays are not touched)
        assert raw(eng, p256, p256, p256, 65535 * 64 + 1, 1, L) == -5                  # B > 4 194 240
        assert b"4 194 240" in lib.dm_last_error(eng._h)
        assert raw(eng, p256, p256, p256, 1 << 20, 5, L) == -5                         # 5 242 880 rows
        assert raw(eng, p256, p256, p256, 1, 65535 * 64 + 1, L) == -5
        assert raw(eng, p256, p256, p256, 1 << 40, 1 << 30, L) == -5                   # (no overflow in U R)
        assert live_allocs() == base
        # ... and the handle still trains
        got = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        assert abs(got - ref["loss"]) <= K["loss"] * T.EPS32 * ref["A_loss"]
        eng.deepfm_adam_step()
    finally:
        eng.close()


# --------------------------------------------------------------------------- a problem it learns
def test_learns_the_teacher_regrouped():
    w0, (seq, codes, y), NI = G.learning_case()
    eng = engine(T.LEARN["E"], T.LEARN["L"], w0, NI)
    try:
        eng.deepfm_train_init(lr=T.LEARN["lr"])
        losses = []
        for _ in range(T.LEARN["steps"]):
            losses.append(eng.deepfm_train_forward_backward_grouped(seq, codes, y))
            eng.deepfm_adam_step()
    finally:
        eng.close()
    assert min(losses) <= 0.8 * losses[0], losses
