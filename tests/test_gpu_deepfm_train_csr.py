"""The ragged (CSR) user-grouped DeepFM training step on the device (dm_deepfm_train_forward_backward_csr_dev in
csrc/dfm_train_grouped.hip.inc) and the sampler twin that feeds it: loss and gradient against the float64 ROW step of
tests/deepfm_train_ref.py on the expanded rows under |gpu - ref| <= k eps32 A with k from tests/golden/deepfm_train_csr_tolerances.json
(CPU-derived); the bytes of the rectangular entry point on uniform offsets; empty users; determinism; the sampler twin against the row
sampler; Engine.deepfm_train_step_sampled(grouped=True); TDMTrainer(grouped=...); refusals."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import deepfm_ref as R
import deepfm_train_ref as T
import deepfm_train_grouped_ref as G
import deepfm_train_csr_ref as S
import deepfm_train_csr_tree as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "deepfm_train_csr_tolerances.json")))["k"]
K_ROW = json.load(open(os.path.join(ROOT, "tests", "golden", "deepfm_train_tolerances.json")))["k"]


def live_allocs():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


def engine(E, L, w, NI=S.NUM_INDEX, tree=None):
    from dismember_amd import Engine
    eng = Engine(0)
    if tree is not None:
        eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
        eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_deepfm(w, E, L, NI)
    return eng


@functools.lru_cache(maxsize=None)
def reference(name):
    """a case and the float64 row step on its expanded rows, computed once"""
    case = S.shape_case(name)[:7] if name in S.CASES else S.structure_case(name)[:7]
    w, E, L, seq, row_off, codes, y = case
    o = S.row_reference(w, E, L, seq, row_off, codes, y)
    for v in (o["g"], o["A"]):
        v.setflags(write=False)
    return case, o


def within(tag, loss, g, ref, E, L, k, NI=S.NUM_INDEX):
    assert np.isfinite(loss) and np.isfinite(g).all()
    ratios = T.ratios(g, ref["g"], ref["A"], E, L, NI)
    ratios["loss"] = abs(loss - ref["loss"]) / (T.EPS32 * ref["A_loss"])
    print("%s: share of the bound " % (tag,) + " ".join("%s %.3f" % (t, ratios[t] / k[t]) for t in sorted(ratios)))
    for t, v in ratios.items():
        assert v <= k[t], (tag, t, v, k[t])


def check_step(name):
    (w, E, L, seq, row_off, codes, y), ref = reference(name)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        loss = eng.deepfm_train_forward_backward_csr(seq, row_off, codes, y)
        g = eng.deepfm_train_download("grad")
    finally:
        eng.close()
    within(name, loss, g, ref, E, L, K)
    emb = g[:S.NUM_INDEX * E].reshape(-1, E)
    read = np.zeros(S.NUM_INDEX, bool)
    read[codes[codes >= 0]] = True
    hist = seq[np.diff(row_off) > 0]                                         # the history of a user without rows is never read
    read[hist[hist >= 0]] = True
    assert not emb[~read].any() and (~read).any()                            # rows no slot read hold exact zeros
    return loss, g


# --------------------------------------------------------------------------- gradient and loss
@pytest.mark.parametrize("name", [n for n in S.CASES if n != S.GRID_CASE])
def test_step_cases(name):
    check_step(name)


def test_step_forced_grid_partial_last_round(monkeypatch):
    monkeypatch.setenv("DM_DFM_TRAIN_GRID", "2")           # 13 user tiles and 80 row tiles over 2 workgroups of 4 waves
    check_step(S.GRID_CASE)


@pytest.mark.parametrize("name", S.STRUCTURES)
def test_step_structures(name):
    check_step(name)


# --------------------------------------------------------------------------- uniform offsets: the rectangular entry point's bytes
@pytest.mark.parametrize("shape", [(16, 1, 1, 1), (16, 1, 17, 17), (16, 1, 33, 40), (128, 10, 19, 41)], ids=lambda s: "E%d-L%d-U%d-R%d" % s)
def test_uniform_offsets_equal_the_rectangular_entry_point_byte_for_byte(shape):
    E, L, U, Rr = shape
    if shape in G.SHAPES:
        w, seq, codes, y, _ = G.shape_case(*shape)
    else:                                                                    # no case of the rectangular sweeps: drawn here
        rng = np.random.default_rng(33040)
        w = R.random_deepfm_weights(rng, E, L, S.NUM_INDEX)
        seq, codes, y = G._draw(rng, E, L, U, Rr)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        la = eng.deepfm_train_forward_backward_grouped(seq, codes, y)
        a = eng.deepfm_train_download("grad")
        lb = eng.deepfm_train_forward_backward_csr(seq, S.offsets([Rr] * U), codes.reshape(-1), y.reshape(-1))
        b = eng.deepfm_train_download("grad")
    finally:
        eng.close()
    assert np.isfinite(la) and a.any()
    assert (la, a.tobytes()) == (lb, b.tobytes())


# --------------------------------------------------------------------------- empty users contribute nothing
@pytest.mark.parametrize("name", ["mixed8", "ends_empty"])
def test_empty_users_contribute_nothing(name):
    (w, E, L, seq, row_off, codes, y), _ = reference(name)
    keep = np.diff(row_off) > 0
    assert not keep.all()
    seq2, off2 = np.ascontiguousarray(seq[keep]), S.offsets(np.diff(row_off)[keep])
    out = []
    for s, o in ((seq, row_off), (seq2, off2)):
        eng = engine(E, L, w)
        try:
            eng.deepfm_train_init(lr=0.01)
            loss = eng.deepfm_train_forward_backward_csr(s, o, codes, y)
            g = eng.deepfm_train_download("grad")
            eng.deepfm_adam_step()
            out.append((loss, g.tobytes()) + tuple(eng.deepfm_train_download(x).tobytes() for x in ("weights", "s", "r")))
        finally:
            eng.close()
    assert out[0][0] == out[1][0]
    for i, what in enumerate(("grad", "weights", "s", "r"), 1):
        assert out[0][i] == out[1][i], what
    assert out[0][2] != w.tobytes()


# --------------------------------------------------------------------------- determinism
def test_repeats_are_byte_identical_also_forced_grid_and_after_other_steps(monkeypatch):
    (w, E, L, seq, row_off, codes, y), _ = reference(S.GRID_CASE)
    w2, seq2, codes2, y2, _ = G.shape_case(16, 1, 33, 1)
    c2, s2, yy2 = G.expand(seq2, codes2, y2)
    c2 = (c2 + 500) % S.NUM_INDEX                                            # other rows than the ragged batch reads
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        step = lambda: (eng.deepfm_train_forward_backward_csr(seq, row_off, codes, y), eng.deepfm_train_download("grad").tobytes())
        a = step()
        assert a == step()
        eng.deepfm_train_forward_backward(c2, s2, yy2)                       # a row step in between: its rows are cleared
        assert eng.deepfm_train_download("grad").tobytes() != a[1]
        assert a == step()
        eng.deepfm_train_forward_backward_grouped(seq2, c2.reshape(33, 1), y2)          # ... and a rectangular step's
        assert eng.deepfm_train_download("grad").tobytes() != a[1]
        assert a == step()
        eng.deepfm_train_forward_backward(c2, s2, yy2)                       # the ragged step's rows are cleared by the row step
        gr2 = eng.deepfm_train_download("grad")
        eng.deepfm_train_init()
        eng.deepfm_train_forward_backward(c2, s2, yy2)
        assert gr2.tobytes() == eng.deepfm_train_download("grad").tobytes()
        monkeypatch.setenv("DM_DFM_TRAIN_GRID", "2")
        d = step()
        assert d == step()
    finally:
        eng.close()


# --------------------------------------------------------------------------- the sampler twin
def _sampler_engine():
    tree = Q.tree()
    w = R.random_deepfm_weights(np.random.default_rng(17), 16, Q.L, Q.NUM_INDEX)
    return engine(16, Q.L, w, Q.NUM_INDEX, tree), w


@pytest.mark.parametrize("with_prob", [False, True], ids=["uniform", "with_prob"])
def test_sampler_twin_equals_the_row_sampler(with_prob):
    from dismember_amd import _native as N
    eng, w = _sampler_engine()
    seq, tgt = Q.targets()
    L = Q.L
    try:
        if with_prob:
            t = Q.tree()
            eng.set_node_probs(t["codes"], np.random.default_rng(2).random(t["codes"].size).astype(np.float32) + 0.1)
        eng.deepfm_train_init()
        _, (codes, rseq, lab) = eng.deepfm_train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=5, with_prob=with_prob, return_rows=True)
        c2, l2, sc, off = eng.deepfm_sample_train_batch_csr(seq, tgt, Q.NEG, Q.START_LEVEL, seed=5, with_prob=with_prob)
        assert codes.size > 100 and (c2.tobytes(), l2.tobytes()) == (codes.tobytes(), lab.tobytes())
        # the boundaries recovered from the row sampler's output: a label 1 at a level-START_LEVEL code opens a target
        want = Q.expected_counts(tgt)
        assert off.dtype == np.int64 and off[0] == 0 and off[-1] == codes.size and (np.diff(off) == want).all()
        first = np.flatnonzero((lab == 1) & (codes >= (1 << Q.START_LEVEL) - 1) & (codes < (1 << (Q.START_LEVEL + 1)) - 1))
        assert (first == off[:-1][want > 0]).all()
        assert want[3] == 0 and want[7] == 0 and len(set(want[want > 0].tolist())) == 2          # ragged: two leaf levels, two empty targets
        for t_ in range(len(tgt)):
            assert (rseq[off[t_]:off[t_ + 1]] == sc[t_]).all(), t_
        assert (sc == R.history_codes(Q.tree(), seq)).all()                   # also the targets without rows
        # the size query and the refusals are the row twin's
        n1, n2 = C.c_int64(0), C.c_int64(0)
        lib, o = N.lib(), N.SampleOpts(Q.START_LEVEL, int(with_prob), 20, 0, 5)
        neg = Q.NEG.ctypes.data_as(N.i32p)
        assert lib.dm_deepfm_sample_train_batch_dev(eng._h, None, None, len(tgt), L, neg, Q.NEG.size, C.byref(o), None, None, None, 0, C.byref(n1)) == 0
        assert lib.dm_deepfm_sample_train_batch_csr_dev(eng._h, None, None, len(tgt), L, neg, Q.NEG.size, C.byref(o), None, None, None, None, 0, C.byref(n2)) == 0
        assert n1.value == n2.value == len(tgt) * int(sum(1 + Q.NEG[l] for l in range(Q.START_LEVEL, Q.DEPTH + 1)))
        p256 = C.c_void_p(256)
        for opts, nneg, L_ in ((N.SampleOpts(Q.START_LEVEL, 0, 20, 1, 5), Q.NEG.size, L),          # use_mask = 1
                               (N.SampleOpts(0, 0, 20, 0, 5), Q.NEG.size, L),                     # start level 0
                               (o, Q.NEG.size - 1, L), (o, Q.NEG.size, L - 1)):                   # too few levels; L != the model's
            ra = lib.dm_deepfm_sample_train_batch_dev(eng._h, None, None, len(tgt), L_, neg, nneg, C.byref(opts), None, None, None, 0, C.byref(n1))
            ea = lib.dm_last_error(eng._h)
            rb = lib.dm_deepfm_sample_train_batch_csr_dev(eng._h, None, None, len(tgt), L_, neg, nneg, C.byref(opts), None, None, None, None, 0, C.byref(n2))
            eb = lib.dm_last_error(eng._h)
            assert ra == rb and ra < 0 and ea.replace(b"_csr_dev", b"_dev") == eb.replace(b"_csr_dev", b"_dev"), (ra, rb, ea, eb)
        # buffers too small / missing: -1 from both
        assert lib.dm_deepfm_sample_train_batch_dev(eng._h, p256, p256, len(tgt), L, neg, Q.NEG.size, C.byref(o), p256, p256, p256, 5, C.byref(n1)) == -1
        assert lib.dm_deepfm_sample_train_batch_csr_dev(eng._h, p256, p256, len(tgt), L, neg, Q.NEG.size, C.byref(o), p256, p256, p256, p256, 5, C.byref(n2)) == -1
        assert lib.dm_deepfm_sample_train_batch_csr_dev(eng._h, p256, p256, len(tgt), L, neg, Q.NEG.size, C.byref(o), p256, p256, None, p256, n1.value, C.byref(n2)) == -1
    finally:
        eng.close()


def test_step_sampled_grouped_against_the_row_path_from_one_seed():
    eng, w = _sampler_engine()
    seq, tgt = Q.targets()
    E, L, NI = 16, Q.L, Q.NUM_INDEX
    try:
        eng.deepfm_train_init()
        lr_, (codes, rseq, lab) = eng.deepfm_train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9, return_rows=True)
        gr_ = eng.deepfm_train_download("grad")
        bytes_row = eng._samp_bytes
        lg, (c2, sc, l2, off) = eng.deepfm_train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9, return_rows=True, grouped=True)
        gg = eng.deepfm_train_download("grad")
        assert (c2.tobytes(), l2.tobytes()) == (codes.tobytes(), lab.tobytes()) and (np.repeat(sc, np.diff(off), axis=0) == rseq).all()
        ref = T.step(w, E, L, NI, codes, rseq, lab)                          # the one float64 reference, on the downloaded rows
        within("row path", lr_, gr_, ref, E, L, K_ROW, NI)
        within("grouped path", lg, gg, ref, E, L, K, NI)
        assert abs(lg - lr_) <= K["loss"] * T.EPS32 * ref["A_loss"]
        # a batch with no rows: loss 0.0 without a step, as the row path
        g0 = eng.deepfm_train_download("grad").tobytes()
        assert eng.deepfm_train_step_sampled(seq[:2], np.zeros(2, np.int32), Q.NEG, Q.START_LEVEL, seed=9, grouped=True) == 0.0
        assert eng.deepfm_train_download("grad").tobytes() == g0
    finally:
        eng.close()
    # the [R][L] row histories are never carved: a fresh engine's sampler buffer is smaller by that much (up to the carving's alignment)
    eng2, _ = _sampler_engine()
    try:
        eng2.deepfm_train_init()
        eng2.deepfm_train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9, grouped=True)
        Rmax = len(tgt) * int(sum(1 + Q.NEG[l] for l in range(Q.START_LEVEL, Q.DEPTH + 1)))
        assert eng2._samp_bytes < bytes_row - Rmax * L * 4
    finally:
        eng2.close()


# --------------------------------------------------------------------------- the trainer
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
    return ids, sc, cnt


def _valid(ids, sc, cnt):
    m = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    return ids[m].tobytes() + sc[m].tobytes() + cnt.tobytes()


def test_trainer_grouped_learns_the_teacher_problem():
    """the weights, tree depth, learning rate, step count and criterion of tests/test_gpu_deepfm_train.py::test_learns_the_teacher; the
    rows and their labels are the sampler's (TDMTrainer draws its own batch): the same 33 histories and targets every step"""
    from dismember_amd.trainer import TDMTrainer
    w0, _, NI = T.learning_case()
    E, L = T.LEARN["E"], T.LEARN["L"]
    tree, _, seqs = R.search_case(E, L)
    assert int(tree["max_level"]) == T.LEARN["depth"]
    tgt = np.random.default_rng(11).choice(tree["leaf_ids"], seqs.shape[0]).astype(np.int32)
    eng = engine(E, L, w0, NI, tree)
    try:
        tr = TDMTrainer(eng, NEG9, 1, lr=T.LEARN["lr"], grouped=True)
        assert tr.grouped and tr.deepfm
        losses = [tr.step(seqs, tgt) for _ in range(T.LEARN["steps"])]
    finally:
        eng.close()
    assert min(losses) <= 0.8 * losses[0], losses


NEG9 = np.array([0, 1, 2, 3, 4, 4, 4, 4, 4, 4], np.int32)


def test_trainer_grouped_serving_after_five_steps_matches_a_fresh_load():
    from dismember_amd.trainer import TDMTrainer
    E, L = 16, 10
    tree, w, seqs = R.search_case(E, L)
    NI = (1 << (R.SEARCH_DEPTH + 1)) - 1
    tgt = np.random.default_rng(11).choice(tree["leaf_ids"], seqs.shape[0]).astype(np.int32)
    eng, fresh = engine(E, L, w, NI, tree), None
    try:
        tr = TDMTrainer(eng, NEG9, 1, lr=0.01, grouped=True)
        for _ in range(5):
            loss = tr.step(seqs, tgt)
            assert np.isfinite(loss) and loss > 0
        wt = eng.deepfm_train_download("weights")
        assert wt.tobytes() != w.tobytes()
        fresh = engine(E, L, wt, NI, tree)
        codes, hist, _ = eng.deepfm_make_train_batch(seqs, tgt, NEG9, 1, seed=99)
        assert eng.deepfm_forward(codes, hist).tobytes() == fresh.deepfm_forward(codes, hist).tobytes()
        want = fresh.tdm_beam_search(seqs, 8, 5, use_mask=False)
        assert _valid(*eng.tdm_beam_search(seqs, 8, 5, use_mask=False)) == _valid(*want)
        assert _valid(*_search_dev(eng, seqs, 8, 5)) == _valid(*want)
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()


def test_trainer_reads_the_variable_once_and_defaults_to_the_row_step(monkeypatch):
    from dismember_amd.trainer import TDMTrainer
    from dismember_amd import Engine
    import helpers
    E, L = 16, 10
    tree, w, seqs = R.search_case(E, L)
    NI = (1 << (R.SEARCH_DEPTH + 1)) - 1
    tgt = np.random.default_rng(11).choice(tree["leaf_ids"], seqs.shape[0]).astype(np.int32)

    def run(grouped, env, sampler="device", manual=False):
        if env is None:
            monkeypatch.delenv("DM_DFM_TRAIN_GROUPED", raising=False)
        else:
            monkeypatch.setenv("DM_DFM_TRAIN_GROUPED", env)
        eng = engine(E, L, w, NI, tree)
        try:
            if manual:                                                       # today's trainer, spelled out: row sampler, row step, Adam
                eng.deepfm_train_init(lr=0.01)
                for it in range(3):
                    eng.deepfm_train_step_sampled(seqs, tgt, NEG9, 1, seed=1000003 * it)
                    eng.deepfm_adam_step(1.0)
            else:
                tr = TDMTrainer(eng, NEG9, 1, lr=0.01, grouped=grouped, sampler=sampler)
                monkeypatch.delenv("DM_DFM_TRAIN_GROUPED", raising=False)     # read once, at construction
                for _ in range(3):
                    tr.step(seqs, tgt)
            return eng.deepfm_train_download("weights").tobytes()
        finally:
            eng.close()

    on = run(True, None)
    row = run(None, None, manual=True)
    assert on != row
    assert run(None, "1") == on                                              # the variable, with grouped=None
    assert run(None, None) == row and run(False, "1") == row and run(None, "0") == row
    assert run(True, None, sampler="host") == run(False, None, sampler="host")          # the host sampler keeps the row step
    # a DIN engine ignores it
    din = Engine(0)
    try:
        din.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
        din.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
        din.load_weights_din(helpers.random_din_weights(np.random.default_rng(1), E, NI), E, NI)
        tr = TDMTrainer(din, NEG9, 1, grouped=True)
        assert not tr.deepfm and np.isfinite(tr.step(seqs, tgt))
    finally:
        din.close()


# --------------------------------------------------------------------------- refusals
def test_refusals_keep_the_live_allocation_count():
    from dismember_amd import DismemberError, Engine, _native as N
    import helpers
    (w, E, L, seq, row_off, codes, y), ref = reference("candidate_in_own_history")
    lib = N.lib()
    loss = C.c_double(0)
    U, B = seq.shape[0], codes.size
    p256 = C.c_void_p(256)
    raw = lambda e, *a: lib.dm_deepfm_train_forward_backward_csr_dev(e._h, *a, C.byref(loss))
    good = lambda e: e.deepfm_train_forward_backward_csr(seq, row_off, codes, y)

    def refused(code, fn, *a):
        base = live_allocs()
        with pytest.raises(DismemberError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert live_allocs() == base

    eng = Engine(0)
    try:
        refused(-3, eng.deepfm_train_forward_backward_csr, seq, row_off, codes, y)          # no model
        eng.load_weights_din(helpers.random_din_weights(np.random.default_rng(1), E, S.NUM_INDEX), E, S.NUM_INDEX)
        refused(-3, eng.deepfm_train_forward_backward_csr, seq, row_off, codes, y)          # a DIN model
        eng.load_weights_deepfm(w, E, L, S.NUM_INDEX)
        refused(-3, eng.deepfm_train_forward_backward_csr, seq, row_off, codes, y)          # before the init
        eng.deepfm_train_init()
        cl = eng.clone()
        try:
            refused(-3, cl.deepfm_train_forward_backward_csr, seq, row_off, codes, y)       # on a clone
        finally:
            cl.close()
        refused(-1, eng.deepfm_train_forward_backward_csr, seq[:, :9], row_off, codes, y)   # L != the model's
        want = good(eng)
        gw = eng.deepfm_train_download("grad").tobytes()
        assert abs(want - ref["loss"]) <= K["loss"] * T.EPS32 * ref["A_loss"]
        base = live_allocs()
        for a in ((0, B), (-1, B), (U, 0), (U, -1)):                                        # U <= 0, B <= 0
            assert raw(eng, p256, p256, p256, p256, a[0], a[1], L) == -1
        for i in range(4):                                                                  # a null array
            ptrs = [p256] * 4
            ptrs[i] = None
            assert raw(eng, *ptrs, U, B, L) == -1
        assert raw(eng, p256, p256, p256, p256, U, B, L + 1) == -1
        assert good(eng) == want
        # too large: refused before anything is read (the arrays are not touched)
        big = 65535 * 64 + 1
        assert raw(eng, p256, p256, p256, p256, 1, big, L) == -5 and b"4 194 240" in lib.dm_last_error(eng._h)
        assert raw(eng, p256, p256, p256, p256, big, 1, L) == -5
        assert raw(eng, p256, p256, p256, p256, 1 << 40, 1 << 40, L) == -5
        assert live_allocs() == base
        assert (good(eng), eng.deepfm_train_download("grad").tobytes()) == (want, gw)
        # malformed offsets, through the wrapper (numpy) ...
        bad0 = row_off.copy(); bad0[0] = 1
        dec = row_off.copy(); dec[4] = dec[3] - 2                                           # users 3 | 4: a decreasing pair
        last = row_off.copy(); last[-1] = B - 1
        for off, word in ((bad0, "user 0"), (dec, "user 3"), (last, "user %d" % U)):
            with pytest.raises(ValueError) as e:
                eng.deepfm_train_forward_backward_csr(seq, off, codes, y)
            assert word in str(e.value)
            assert live_allocs() == base and good(eng) == want
        # ... and through the device entry: checked on the device, before anything is read through them
        al = lambda v: (v + 255) & ~255
        buf = eng.dev_alloc(al(U * L * 4) + al((U + 1) * 8) + 2 * al(B * 4))
        try:
            d_seq = C.c_void_p(buf.value); d_off = C.c_void_p(d_seq.value + al(U * L * 4))
            d_codes = C.c_void_p(d_off.value + al((U + 1) * 8)); d_lab = C.c_void_p(d_codes.value + al(B * 4))
            eng.h2d(d_seq, seq); eng.h2d(d_codes, codes); eng.h2d(d_lab, y)
            base = live_allocs()
            for off, word in ((bad0, b"user 0"), (dec, b"user 3"), (last, b"user %d" % U)):
                eng.h2d(d_off, off)
                assert raw(eng, d_seq, d_off, d_codes, d_lab, U, B, L) == -1 and word in lib.dm_last_error(eng._h), lib.dm_last_error(eng._h)
                assert eng.deepfm_train_download("grad").tobytes() == gw                    # the gradient was not touched
                eng.h2d(d_off, row_off)
                assert eng.deepfm_train_forward_backward_csr_dev(d_seq, d_off, d_codes, d_lab, U, B, L) == want
                assert live_allocs() == base
        finally:
            eng.dev_free(buf)
        eng.deepfm_adam_step()
    finally:
        eng.close()
