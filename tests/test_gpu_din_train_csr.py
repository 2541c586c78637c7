"""The ragged (CSR) user-grouped DIN training step on the device (dm_train_forward_backward_csr_dev in csrc/train_grouped_csr.hip.inc;
DESIGN.md §21) and the sampler twin that feeds it: loss and gradient against the float64 ROW step of tests/train_ref.py on the expanded
rows under |gpu - ref| <= k_T eps32 A with k from tests/golden/din_train_csr_tolerances.json (CPU-derived); Adam afterwards; the same
bytes on a repeat, under a forced grid, without the rowless users and after other steps; accumulation with the row step; the sampler twin
against the row sampler; Engine.train_step_sampled(grouped=True); TDMTrainer(din_grouped=...); two workers; refusals."""
import ctypes as C
import functools
import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

import train_ref as R
import din_train_csr_ref as S
import deepfm_train_csr_tree as Q
from helpers import random_din_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "din_train_csr_tolerances.json")))["k"]
K_ROW = json.load(open(os.path.join(ROOT, "tests", "golden", "train_tolerances.json")))["f32"]["k"]
NEW_KINDS = (56, 57, 58, 59, 68)          # EV_DTC_SETUP, _ROWS, _USER_BWD, _DW, _EMB (csrc/host_request.hip.inc)
NI = S.NUM_INDEX


def live_allocs():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


def engine(E, w, num_index=NI, tree=None, lr=1e-3, init=True):
    from dismember_amd import Engine
    eng = Engine(0)
    if tree is not None:
        eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
        eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_din(w, E, num_index)
    if init:
        eng.train_init(lr=lr)
    return eng


CASE_NAMES = list(S.CASES) + ["%s-%s" % (n, m) for n in S.STRUCTURES for m in ("masked", "nomask")]


def get_case(name):
    if name in S.CASES:
        return S.shape_case(name)
    n, m = name.rsplit("-", 1)
    return S.structure_case(n, m == "masked")


@functools.lru_cache(maxsize=None)
def reference(name):
    """a case and the float64 row step on its expanded rows, computed once"""
    case = get_case(name)
    w, E, L, seq, umask, row_off, codes, y = case
    o = S.row_reference(w, E, L, seq, umask, row_off, codes, y)
    for v in (o["g"], o["A"]):
        v.setflags(write=False)
    return case, o


def within(tag, loss, g, ref_g, ref_A, ref_loss, E, k, num_index=NI):
    """every tensor under its bound, exact zeros where nothing was added, the loss under its own bound"""
    assert np.isfinite(loss) and np.isfinite(g).all()
    print("%s loss %.9g  ref %.9g" % (tag, loss, ref_loss))
    assert abs(loss - ref_loss) <= S.loss_bound(ref_loss), (tag, loss, ref_loss)
    scale = R.element_scale(ref_A, E, num_index)
    for t, (a, b) in R.sections(E, num_index).items():
        live = scale[a:b] > 0
        assert (g[a:b][~live] == 0).all(), (tag, t, "non-zero where nothing was added")
        ratio = np.abs(g[a:b].astype(np.float64) - ref_g[a:b])[live] / (S.EPS32 * scale[a:b][live])
        worst = float(ratio.max()) if ratio.size else 0.0
        print("%s %-6s max |g - ref| / (eps A) = %9.3f  (k_T = %.3f)" % (tag, t, worst, k[t]))
        assert worst <= k[t], (tag, t, worst, k[t])


def check_step(oracle, name):
    (w, E, L, seq, umask, row_off, codes, y), ref = reference(name)
    eng = engine(E, w)
    try:
        loss = eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
        assert loss == np.float32(eng.train_last_loss())
        g = eng.train_download("grad")
        within(name, loss, g, ref["g"], ref["A"], ref["loss"], E, K)
        named = np.zeros(NI, bool)
        named[codes[codes >= 0]] = True
        hist = seq[np.diff(row_off) > 0]                                       # the history of a user without rows is never read
        named[hist[hist >= 0]] = True
        assert not g[:NI * E].reshape(NI, E)[~named].any() and (~named).any()      # rows no slot names hold exact zeros
        # Adam on the device's own gradient, bit for bit; the gradient is cleared
        eng.adam_step(1.0)
        want = w.copy()
        opt = oracle.Adam(want.size, np.float32, lr=1e-3)
        opt.step(want, g.copy())
        assert np.array_equal(eng.train_download("weights"), want)
        assert np.array_equal(eng.train_download("s"), opt.s) and np.array_equal(eng.train_download("r"), opt.r)
        assert (eng.train_download("grad") == 0).all()
    finally:
        eng.close()


# --------------------------------------------------------------------------- gradient, loss, Adam
@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n != S.GRID_CASE])
def test_step_cases(oracle, name):
    check_step(oracle, name)


def test_step_forced_grid_partial_last_round(oracle, monkeypatch):
    monkeypatch.setenv("DM_DIN_TRAIN_GRID", "2")           # 200 users and 125 row tiles over 2 workgroups of 4 waves
    check_step(oracle, S.GRID_CASE)


# --------------------------------------------------------------------------- determinism
def _fresh_step(case, before=None):
    """(loss, gradient bytes) of the case on a fresh handle; before(eng): steps that run first (the weights are reloaded after them)"""
    w, E, L, seq, umask, row_off, codes, y = case
    eng = engine(E, w)
    try:
        if before is not None:
            before(eng)
            eng.load_weights_din(w, E, NI)
            eng.train_init(lr=1e-3)
        loss = eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
        return loss, eng.train_download("grad").tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("name", [S.GRID_CASE, "tdm-E128-L10", "unmasked_pads-masked"])
def test_same_bytes_on_a_repeat_a_forced_grid_without_rowless_users_and_after_other_steps(name, monkeypatch):
    case, _ = reference(name)
    w, E, L, seq, umask, row_off, codes, y = case
    a = _fresh_step(case)
    assert np.frombuffer(a[1], np.float32).any()
    assert _fresh_step(case) == a                                               # a repeat
    monkeypatch.setenv("DM_DIN_TRAIN_GRID", "2")
    assert _fresh_step(case) == a                                               # the grid does not enter the bytes
    monkeypatch.delenv("DM_DIN_TRAIN_GRID")
    if not (np.diff(row_off) > 0).all():                                        # the same batch without its rowless users
        seq2, um2, off2 = S.drop_rowless(seq, umask, row_off)
        assert _fresh_step((w, E, L, seq2, um2, off2, codes, y)) == a
    c_, s_, pad, yy = S.expand(seq, umask, row_off, codes, y)

    def before(eng):                                                            # a row step and an Adam step before it
        eng.train_forward_backward(c_, s_, pad, yy)
        eng.adam_step(1.0)
    assert _fresh_step(case, before) == a


# --------------------------------------------------------------------------- ids outside [0, num_index) read as -1
@pytest.mark.parametrize("name", ["mixed8", "candidate_in_own_history-masked", "tdm-E128-L10"])
def test_ids_outside_the_table_read_as_minus_one(name):
    """candidate and history ids >= num_index (and below -1) on the entry that does not range-check: no gather, no table gradient, not
    marked active — the bytes, the loss and the rows the Adam step visits are those of the same batch with -1 in their places"""
    (w, E, L, seq, umask, row_off, codes, y), _ = reference(name)
    rng = np.random.default_rng(4)
    pop = np.flatnonzero(np.diff(row_off) > 0)
    seq_m, codes_m = seq.copy(), codes.copy()
    hit_c = rng.choice(codes.size, max(1, codes.size // 5), replace=False)
    hit_s = [(int(u), int(j)) for u in pop for j in range(L) if rng.random() < 0.3] or [(int(pop[0]), 0)]
    codes_m[hit_c] = -1
    for u, j in hit_s:
        seq_m[u, j] = -1
    seq_o, codes_o = seq_m.copy(), codes_m.copy()
    codes_o[hit_c] = np.where(np.arange(hit_c.size) % 3 == 0, -7, NI + np.arange(hit_c.size) * 1000003 % (2 ** 31 - 1 - NI)).astype(np.int32)
    for i, (u, j) in enumerate(hit_s):
        seq_o[u, j] = NI if i % 2 else 2 ** 31 - 1
    assert ((codes_o >= NI) | (codes_o < -1)).sum() == hit_c.size and (seq_o >= NI).sum() == len(hit_s)
    ref = S.row_reference(w, E, L, seq_m, umask, row_off, codes_m, y)
    out = []
    for sq, cd in ((seq_m, codes_m), (seq_o, codes_o)):
        eng = engine(E, w)
        try:
            loss = eng.train_forward_backward_csr(sq, umask, row_off, cd, y)
            g = eng.train_download("grad")
            eng.adam_step(1.0)
            out.append((loss, g.tobytes(), eng.adam_last_step_rows(), eng.train_download("weights").tobytes()))
        finally:
            eng.close()
    assert out[0] == out[1]
    within(name + " ids outside", out[1][0], np.frombuffer(out[1][1], np.float32), ref["g"], ref["A"], ref["loss"], E, K)
    named = np.zeros(NI, bool)
    named[codes_m[codes_m >= 0]] = True
    hist = seq_m[np.diff(row_off) > 0]
    named[hist[hist >= 0]] = True
    rows, sparse = out[1][2]                                                    # the active rows: exactly the rows a valid id names
    assert rows == (int(named.sum()) if sparse else NI) and (sparse or name != "mixed8")


# --------------------------------------------------------------------------- accumulation until the Adam step
def test_two_csr_calls_and_a_row_call_plus_a_csr_call_accumulate():
    (w, E, L, seq, umask, row_off, codes, y), ra = reference("mixed8")
    (w2, E2, L2, seq2, umask2, row_off2, codes2, y2), _ = reference("empty_tile")
    assert (E, L) == (E2, L2)
    rb = S.row_reference(w, E, L, seq2, umask2, row_off2, codes2, y2)           # the second batch on the FIRST case's weights
    # call i is within k_i eps A_i of its float64 gradient and adding the second to the first rounds once more (at most eps |sum| <= eps A):
    # the sum is within (max k_i + 1) eps (A_1 + A_2) of the float64 sum
    sum_g, sum_A = ra["g"] + rb["g"], R.element_scale(ra["A"], E, NI) + R.element_scale(rb["A"], E, NI)
    k_cc = {t: K[t] + 1 for t in K}
    k_rc = {t: max(K[t], K_ROW[t]) + 1 for t in K}
    c_, s_, pad, yy = S.expand(seq2, umask2, row_off2, codes2, y2)
    eng = engine(E, w)
    try:
        eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
        one = eng.train_download("grad")
        loss = eng.train_forward_backward_csr(seq2, umask2, row_off2, codes2, y2)
        g = eng.train_download("grad")
        assert not np.array_equal(g, one)
        within("csr + csr", loss, g, sum_g, sum_A, rb["loss"], E, k_cc)
        eng.adam_step(1.0)
        assert (eng.train_download("grad") == 0).all()
        eng.load_weights_din(w, E, NI)
        eng.train_init(lr=1e-3)
        eng.train_forward_backward(c_, s_, pad, yy)                             # the row step first, the ragged step on top
        loss = eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
        within("row + csr", loss, eng.train_download("grad"), sum_g, sum_A, ra["loss"], E, k_rc)
    finally:
        eng.close()


# --------------------------------------------------------------------------- the sampler twin
def _sampler_engine(E=16, init=True):
    w = random_din_weights(np.random.default_rng(17), E, Q.NUM_INDEX, std=0.2, bias_std=0.2)
    return engine(E, w, Q.NUM_INDEX, Q.tree(), init=init), w


def _history_codes(tree, seq):
    """TDMTree.idToCode over item-id histories: 0 and ids the maps do not know -> -1"""
    lut = {int(i): int(c) for i, c in zip(tree["leaf_ids"], tree["leaf_codes"])}
    return np.array([[lut.get(int(i), -1) if i != 0 else -1 for i in row] for row in seq], np.int32)


@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("with_prob", [False, True], ids=["uniform", "with_prob"])
def test_sampler_twin_equals_the_row_sampler(with_prob, use_mask):
    from dismember_amd import _native as N
    eng, _ = _sampler_engine(init=False)
    seq, tgt = Q.targets()
    L = Q.L
    try:
        if with_prob:
            t = Q.tree()
            eng.set_node_probs(t["codes"], np.random.default_rng(2).random(t["codes"].size).astype(np.float32) + 0.1)
        kw = dict(start_level=Q.START_LEVEL, seed=5, use_mask=use_mask, with_prob=with_prob)
        codes, rseq, rmask, lab = eng.make_train_batch(seq, tgt, Q.NEG, **kw)
        c2, l2, sc, um, off = eng.sample_train_batch_csr(seq, tgt, Q.NEG, **kw)
        assert codes.size > 100 and (c2.tobytes(), l2.tobytes()) == (codes.tobytes(), lab.tobytes())
        want = Q.expected_counts(tgt)
        assert off.dtype == np.int64 and off[0] == 0 and off[-1] == codes.size and (np.diff(off) == want).all()
        assert want[3] == 0 and want[7] == 0 and len(set(want[want > 0].tolist())) == 2          # ragged: two leaf levels, a padding target, one outside
        for t_ in range(len(tgt)):
            assert (rseq[off[t_]:off[t_ + 1]] == sc[t_]).all(), t_
            assert (rmask[off[t_]:off[t_ + 1]] == um[t_]).all(), t_              # the row sampler's rowmask, per row
        assert (sc == _history_codes(Q.tree(), seq)).all()                      # also the histories of the targets without rows
        assert um.dtype == np.uint32 and ((um == S.pad_mask(sc)).all() if use_mask else not um.any())
        assert use_mask is False or um[5] == (1 << L) - 1                       # (the all-padding history)
        # the size query and the refusals are the row twin's
        n1, n2 = C.c_int64(0), C.c_int64(0)
        lib, o = N.lib(), N.SampleOpts(Q.START_LEVEL, int(with_prob), 20, int(use_mask), 5)
        neg = Q.NEG.ctypes.data_as(N.i32p)
        assert lib.dm_tdm_sample_train_batch_dev(eng._h, None, None, len(tgt), L, neg, Q.NEG.size, C.byref(o), None, None, None, None, 0, C.byref(n1)) == 0
        assert lib.dm_tdm_sample_train_batch_csr_dev(eng._h, None, None, len(tgt), L, neg, Q.NEG.size, C.byref(o), None, None, None, None, None, 0, C.byref(n2)) == 0
        assert n1.value == n2.value == len(tgt) * int(sum(1 + Q.NEG[l] for l in range(Q.START_LEVEL, Q.DEPTH + 1)))
        p256 = C.c_void_p(256)
        for opts, nneg, L_ in ((N.SampleOpts(0, 0, 20, int(use_mask), 5), Q.NEG.size, L),              # start level 0
                               (o, Q.NEG.size - 1, L), (o, Q.NEG.size, 33), (o, Q.NEG.size, 0),        # too few levels; L out of range
                               (N.SampleOpts(Q.START_LEVEL, 1, -1, int(use_mask), 5), Q.NEG.size, L)):  # a negative tolerance / no node probabilities
            ra = lib.dm_tdm_sample_train_batch_dev(eng._h, None, None, len(tgt), L_, neg, nneg, C.byref(opts), None, None, None, None, 0, C.byref(n1))
            ea = lib.dm_last_error(eng._h)
            rb = lib.dm_tdm_sample_train_batch_csr_dev(eng._h, None, None, len(tgt), L_, neg, nneg, C.byref(opts), None, None, None, None, None, 0, C.byref(n2))
            eb = lib.dm_last_error(eng._h)
            assert ra == rb and ra < 0 and ea == eb, (ra, rb, ea, eb)
        # buffers too small / missing: -1 from both
        assert lib.dm_tdm_sample_train_batch_dev(eng._h, p256, p256, len(tgt), L, neg, Q.NEG.size, C.byref(o), p256, p256, p256, p256, 5, C.byref(n1)) == -1
        assert lib.dm_tdm_sample_train_batch_csr_dev(eng._h, p256, p256, len(tgt), L, neg, Q.NEG.size, C.byref(o), p256, p256, p256, p256, p256, 5, C.byref(n2)) == -1
        for missing in (9, 10, 11, 12):                                         # d_seq_codes, d_umask, d_row_off, d_labels
            a = [eng._h, p256, p256, len(tgt), L, neg, Q.NEG.size, C.byref(o), p256, p256, p256, p256, p256, n1.value, C.byref(n2)]
            a[missing] = None
            assert lib.dm_tdm_sample_train_batch_csr_dev(*a) == -1
    finally:
        eng.close()


def test_step_sampled_grouped_and_row_path_from_one_seed_against_one_reference():
    eng, w = _sampler_engine()
    seq, tgt = Q.targets()
    E, L, QNI = 16, Q.L, Q.NUM_INDEX
    try:
        codes, rseq, rmask, lab = eng.make_train_batch(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9)
        ref = R.step(w, E, L, QNI, codes, rseq, eng.rowmask_to_flat(rmask, L), lab)          # the one float64 reference, on the downloaded rows
        lr_ = eng.train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9)
        gr_ = eng.train_download("grad")
        bytes_row = eng._samp_bytes
        eng.adam_step(1.0)
        eng.load_weights_din(w, E, QNI)
        eng.train_init()
        lg = eng.train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9, grouped=True)
        gg = eng.train_download("grad")
        within("row path", lr_, gr_, ref["g"], ref["A"], ref["loss"], E, K_ROW, QNI)
        within("grouped path", lg, gg, ref["g"], ref["A"], ref["loss"], E, K, QNI)
        # a batch with no rows: loss 0.0 without a step
        g0 = gg.tobytes()
        assert eng.train_step_sampled(seq[:2], np.zeros(2, np.int32), Q.NEG, Q.START_LEVEL, seed=9, grouped=True) == 0.0
        assert eng.train_download("grad").tobytes() == g0
    finally:
        eng.close()
    # the [R][L] row histories are never carved: a fresh engine's sampler buffer is smaller by that much (up to the carving's alignment)
    eng2, _ = _sampler_engine()
    try:
        eng2.train_step_sampled(seq, tgt, Q.NEG, Q.START_LEVEL, seed=9, grouped=True)
        Rmax = len(tgt) * int(sum(1 + Q.NEG[l] for l in range(Q.START_LEVEL, Q.DEPTH + 1)))
        assert eng2._samp_bytes < bytes_row - Rmax * L * 4 // 2
    finally:
        eng2.close()


# --------------------------------------------------------------------------- the trainer
def _search_dev(eng, seqs, beam, topk):
    U, L = seqs.shape
    d_seq, d_ids, d_sc, d_cnt = eng.dev_alloc(U * L * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * 4)
    try:
        eng.h2d(d_seq, np.ascontiguousarray(seqs, np.int32))
        eng.tdm_beam_search_dev(d_seq, U, L, beam, topk, d_ids, d_sc, d_cnt)
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


def test_trainer_grouped_first_loss_and_serving_after_five_steps(monkeypatch):
    from dismember_amd.trainer import TDMTrainer
    monkeypatch.setenv("DM_G_TABLE", "1")                                       # the per-row set-up table of the beam kernel on
    seq, tgt = Q.targets()
    E, L, QNI = 16, Q.L, Q.NUM_INDEX
    eng, w = _sampler_engine(init=False)
    fresh = None
    try:
        tr = TDMTrainer(eng, Q.NEG, Q.START_LEVEL, lr=0.01, seed=3, din_grouped=True)
        assert tr.din_grouped and not tr.deepfm
        codes, rseq, rmask, lab = eng.make_train_batch(seq, tgt, Q.NEG, Q.START_LEVEL, seed=3)      # the trainer's first seed, rank 0
        want = R.step(w, E, L, QNI, codes, rseq, eng.rowmask_to_flat(rmask, L), lab, loss_only=True)
        losses = [tr.step(seq, tgt) for _ in range(5)]
        assert abs(losses[0] - want) <= S.loss_bound(want), (losses[0], want)
        assert all(np.isfinite(l) and l > 0 for l in losses)
        wt = eng.train_download("weights")
        assert wt.tobytes() != w.tobytes()
        fresh = engine(E, wt, QNI, Q.tree(), init=False)
        pad = eng.rowmask_to_flat(rmask, L)
        assert eng.din_forward(codes, rseq, pad).tobytes() == fresh.din_forward(codes, rseq, pad).tobytes()
        res = fresh.tdm_beam_search(seq, 8, 5)
        assert _valid(*eng.tdm_beam_search(seq, 8, 5)) == _valid(*res)
        assert _valid(*_search_dev(eng, seq, 8, 5)) == _valid(*res)
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()


def _kinds(eng):
    return [eng.timing_get_kind(k)[0] for k in NEW_KINDS]


def test_trainer_reads_the_variable_once_and_only_the_grouped_route_records_the_new_kinds(monkeypatch):
    from dismember_amd.trainer import TDMTrainer
    import deepfm_ref as DR
    monkeypatch.setenv("DM_TRAIN_TIME_LAUNCHES", "1")
    seq, tgt = Q.targets()

    def run(din_grouped, env, sampler="device", L=Q.L, deepfm=False):
        if env is None:
            monkeypatch.delenv("DM_DIN_TRAIN_GROUPED", raising=False)
        else:
            monkeypatch.setenv("DM_DIN_TRAIN_GROUPED", env)
        if deepfm:
            from dismember_amd import Engine
            eng = Engine(0)
            t = Q.tree()
            eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
            eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
            eng.load_weights_deepfm(DR.random_deepfm_weights(np.random.default_rng(1), 16, L, Q.NUM_INDEX), 16, L, Q.NUM_INDEX)
        else:
            eng, _ = _sampler_engine(init=False)
        try:
            tr = TDMTrainer(eng, Q.NEG, Q.START_LEVEL, lr=0.01, din_grouped=din_grouped, sampler=sampler)
            monkeypatch.delenv("DM_DIN_TRAIN_GROUPED", raising=False)           # read once, at construction
            eng.timing_reset()
            s = seq if L == Q.L else np.concatenate([seq, seq], axis=1)[:, :L]
            for _ in range(2):
                assert np.isfinite(tr.step(s, tgt))
            return _kinds(eng), tr.din_grouped
        finally:
            eng.close()

    on, flag = run(True, None)
    assert flag and all(n > 0 for n in on), on                                 # the grouped route records every new kind
    assert on[:3] == [2, 2, 2]                                                  # one set-up, rows and user-backward launch per step
    assert run(None, "1") == (on, True)                                         # the variable, with din_grouped=None
    for args in ((None, None), (False, "1"), (None, "0"), (True, None, "host"), (True, None, "device", 20)):
        kinds, _ = run(*args)
        assert kinds == [0] * len(NEW_KINDS), (args, kinds)
    kinds, flag = run(True, "1", deepfm=True)
    assert kinds == [0] * len(NEW_KINDS) and not flag


def test_new_kinds_are_recorded_only_under_the_switch(monkeypatch):
    (w, E, L, seq, umask, row_off, codes, y), _ = reference("mixed8")
    monkeypatch.delenv("DM_TRAIN_TIME_LAUNCHES", raising=False)
    eng = engine(E, w)
    try:
        eng.timing_reset()
        eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
        assert _kinds(eng) == [0] * len(NEW_KINDS)
        monkeypatch.setenv("DM_TRAIN_TIME_LAUNCHES", "1")
        eng.timing_reset()
        eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
        assert _kinds(eng) == [1] * len(NEW_KINDS)
    finally:
        eng.close()


# --------------------------------------------------------------------------- two workers on one GPU over the host transport
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


_WORKER_CASES = ("mixed8", "empty_tile")


def _worker(rank, world, port, q):
    from dismember_amd.comm import Comm
    w = S.shape_case(_WORKER_CASES[0])[0]                                        # one model, a batch per rank
    _, E, L, seq, umask, row_off, codes, y = S.shape_case(_WORKER_CASES[rank])
    eng = engine(E, w)
    comm = Comm(world, rank, "127.0.0.1", port, transport="host")
    eng.attach_comm(comm)
    loss = eng.train_forward_backward_csr(seq, umask, row_off, codes, y)
    local = eng.train_download("grad")
    eng.train_sync_gradients()
    summed = eng.train_download("grad")
    eng.adam_step(1.0 / world)
    q.put((rank, loss, local, summed) + tuple(eng.train_download(x) for x in ("weights", "s", "r")))
    comm.barrier()
    eng.close(); comm.close()


def test_two_workers_exchange_the_csr_gradient_and_stay_bit_identical():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    out = sorted((q.get(timeout=600) for _ in range(world)), key=lambda t: t[0])
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    w, E, L = S.shape_case(_WORKER_CASES[0])[:3]
    refs = [S.row_reference(w, E, L, *S.shape_case(n)[3:]) for n in _WORKER_CASES]
    for i in (4, 5, 6):                                                          # weights and both moments, byte for byte
        assert out[0][i].tobytes() == out[1][i].tobytes()
    assert out[0][4].tobytes() != w.tobytes()
    assert out[0][3].tobytes() == out[1][3].tobytes()
    assert np.array_equal(out[0][3], out[0][2] + out[1][2])                      # rank order: (0 + g_0) + g_1 in float32
    # each rank within K eps A_r of its float64 gradient, one more rounding in the rank-ordered sum (see the accumulation test)
    sum_A = R.element_scale(refs[0]["A"], E, NI) + R.element_scale(refs[1]["A"], E, NI)
    within("exchanged", out[1][1], out[0][3], refs[0]["g"] + refs[1]["g"], sum_A, refs[1]["loss"], E, {t: K[t] + 1 for t in K})


# --------------------------------------------------------------------------- refusals
def test_refusals_leave_the_gradient_and_the_live_allocation_count():
    from dismember_amd import DismemberError, Engine, _native as N
    import deepfm_ref as DR
    (w, E, L, seq, umask, row_off, codes, y), ref = reference("candidate_in_own_history-masked")
    lib = N.lib()
    loss = C.c_float(0)
    U, B = seq.shape[0], codes.size
    p256 = C.c_void_p(256)
    raw = lambda e, *a: lib.dm_train_forward_backward_csr_dev(e._h, *a, C.byref(loss))
    good = lambda e: e.train_forward_backward_csr(seq, umask, row_off, codes, y)

    def refused(code, fn, *a):
        base = live_allocs()
        with pytest.raises(DismemberError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert live_allocs() == base
        return str(e.value)

    eng = Engine(0)
    try:
        refused(-3, eng.train_forward_backward_csr, seq, umask, row_off, codes, y)              # no model
        eng.load_weights_deepfm(DR.random_deepfm_weights(np.random.default_rng(1), E, L, NI), E, L, NI)
        assert "DeepFM" in refused(-5, eng.train_forward_backward_csr, seq, umask, row_off, codes, y)      # the DIN entry points' refusal
        eng.load_weights_din(w.astype(np.float64), E, NI)
        eng.train_init()
        assert "f64" in refused(-5, eng.train_forward_backward_csr, seq, umask, row_off, codes, y)         # an f64 model
        eng.load_weights_din(w, E, NI)
        refused(-3, eng.train_forward_backward_csr, seq, umask, row_off, codes, y)              # before dm_train_init
        eng.train_init()
        # a cold handle (no step has run since it was created) and malformed offsets: the workspace is not reserved either
        al = lambda v: (v + 255) & ~255
        cold = eng.dev_alloc(al((U + 1) * 8))
        try:
            off_bad = row_off.copy(); off_bad[-1] = B - 1
            eng.h2d(cold, off_bad)
            base = live_allocs()
            assert raw(eng, p256, None, cold, p256, p256, U, B, L) == -1 and b"user %d" % U in lib.dm_last_error(eng._h)
            assert live_allocs() == base
        finally:
            eng.dev_free(cold)
        want = good(eng)
        assert abs(want - ref["loss"]) <= S.loss_bound(ref["loss"])
        eng.adam_step(1.0)
        eng.load_weights_din(w, E, NI)
        eng.train_init()
        want = good(eng)
        gw = eng.train_download("grad").tobytes()
        base = live_allocs()

        def untouched():
            assert live_allocs() == base and eng.train_download("grad").tobytes() == gw

        for a in ((0, B), (-1, B), (U, 0), (U, -1)):                                            # U <= 0, B <= 0
            assert raw(eng, p256, p256, p256, p256, p256, a[0], a[1], L) == -1
        for i in (0, 2, 3, 4):                                                                  # a null array other than d_umask
            ptrs = [p256] * 5
            ptrs[i] = None
            assert raw(eng, *ptrs, U, B, L) == -1
        for L_ in (0, -1, 33):
            assert raw(eng, p256, p256, p256, p256, p256, U, B, L_) == -1
        for L_ in (17, 32):
            assert raw(eng, p256, p256, p256, p256, p256, U, B, L_) == -5
            assert b"histories longer than 16 keep the row step" in lib.dm_last_error(eng._h)
        # sizes beyond the sort's key and index widths and the products' grids; B = 2 000 000, U = 16 384 passes these checks
        big = 65535 * 64 + 1
        assert raw(eng, p256, p256, p256, p256, p256, 1, big, L) == -5 and b"4 194 240" in lib.dm_last_error(eng._h)
        assert raw(eng, p256, p256, p256, p256, p256, big, 1, L) == -5
        assert raw(eng, p256, p256, p256, p256, p256, 1 << 40, 1 << 40, L) == -5
        untouched()
        # a clone: whatever train_check answers there (the row entry's answer on the same clone), through the wrapper and the device entry;
        # nothing allocated, the owner's gradient untouched, and the owner still steps (below)
        cl = eng.clone()
        try:
            refused(-3, cl.train_forward_backward_csr, seq, umask, row_off, codes, y)
            assert raw(cl, p256, p256, p256, p256, p256, U, B, L) == -3
            e_csr = lib.dm_last_error(cl._h)
            assert lib.dm_train_forward_backward_dev(cl._h, p256, p256, p256, p256, B, L, C.byref(loss)) == -3
            e_row = lib.dm_last_error(cl._h)
            assert e_csr and e_csr.replace(b"_csr_dev", b"_dev") == e_row, (e_csr, e_row)
        finally:
            cl.close()
        untouched()
        # malformed offsets, through the wrapper (numpy) ...
        bad0 = row_off.copy(); bad0[0] = 1
        dec = row_off.copy(); dec[4] = dec[3] - 2                                               # users 3 | 4: a decreasing pair
        last = row_off.copy(); last[-1] = B - 1
        for off, word in ((bad0, "user 0"), (dec, "user 3"), (last, "user %d" % U)):
            with pytest.raises(ValueError) as e:
                eng.train_forward_backward_csr(seq, umask, off, codes, y)
            assert word in str(e.value)
            untouched()
        # ... and through the device entry: checked on the device, before anything is read through them or added to the gradient
        buf = eng.dev_alloc(al(U * L * 4) + al(U * 4) + al((U + 1) * 8) + 2 * al(B * 4))
        try:
            d_seq = C.c_void_p(buf.value); d_um = C.c_void_p(d_seq.value + al(U * L * 4)); d_off = C.c_void_p(d_um.value + al(U * 4))
            d_codes = C.c_void_p(d_off.value + al((U + 1) * 8)); d_lab = C.c_void_p(d_codes.value + al(B * 4))
            eng.h2d(d_seq, seq); eng.h2d(d_um, umask); eng.h2d(d_codes, codes); eng.h2d(d_lab, y)
            base = live_allocs()
            for off, word in ((bad0, b"user 0"), (dec, b"user 3"), (last, b"user %d" % U)):
                eng.h2d(d_off, off)
                assert raw(eng, d_seq, d_um, d_off, d_codes, d_lab, U, B, L) == -1 and word in lib.dm_last_error(eng._h), lib.dm_last_error(eng._h)
                untouched()
            # ... and a good call through the same buffers on a fresh training state: the first call's loss and bytes
            eng.h2d(d_off, row_off)
            eng.adam_step(1.0)
            eng.load_weights_din(w, E, NI)
            eng.train_init()
            assert eng.train_forward_backward_csr_dev(d_seq, d_um, d_off, d_codes, d_lab, U, B, L) == want
            assert eng.train_download("grad").tobytes() == gw
        finally:
            eng.dev_free(buf)
        # a warm call allocates nothing (warm: the step has run at this size since dm_train_init, and the touched-row list, which
        # grows while gradients accumulate, was reset by an Adam step)
        eng.adam_step(1.0)
        good(eng)
        eng.adam_step(1.0)
        base = live_allocs()
        good(eng)
        assert live_allocs() == base
    finally:
        eng.close()
