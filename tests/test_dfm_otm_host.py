"""OTM with the DeepFM scorer, CPU side: the conditions tests/test_gpu_deepfm_otm.py rests on (no GPU).

(a) on every scored row of every case the float32 restatement (sequential sums: the least favourable reading of the reference's BLAS
    calls) stays within the tolerance of float64 — the tolerance is one the reference's own float32 arithmetic meets;
(b) the tolerance sees the faults a kernel could have: dropping e.s, dropping c, dropping the deep part, W1a scaled by 1.05 each move at
    least 90 % of the scored rows out of it;
(c) the replay fails on a trace with two swapped codes, with a tie broken the wrong way, with one score off by twice the tolerance;
(d) the pseudo-target restatement is OTMTree.computeTargets when both forwards return the same value;
(e) the header and the binding table declare the five entry points.
"""
import functools
import os
import re

import numpy as np
import pytest

import deepfm_ref as R
import dfm_otm_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dm_deepfm_otm_beam_search", "dm_deepfm_otm_beam_search_trace", "dm_deepfm_otm_beam_search_dev", "dm_deepfm_otm_pseudo_targets",
         "dm_deepfm_otm_train_batch")
# the scored rows do not depend on U = 1 vs 33 (the same users), nor does the arithmetic on the NaN row: finite cases, one per shape
FINITE = [c for c in D.CASES if c[5] != "nan" and c[4] == 33 and D.level_counts(c[2], c[3])]
USERS = (0, 1, 2, 7)          # user 1 is the all-pad history


@functools.lru_cache(maxsize=None)
def scored_rows(c):
    """(codes, user index) of every row the float64 search of the case scores, for USERS"""
    E, L, beam, leaf_level, U, kind = c
    w, ni, seqs = D.case_inputs(c)
    codes, users = [], []
    for u in USERS:
        for lc, _ in D.search(w, E, L, ni, seqs[u], beam, leaf_level):
            codes.append(lc); users.append(np.full(lc.size, u))
    return np.concatenate(codes), np.concatenate(users)


def forward_rows(c, w, dtype):
    E, L = c[0], c[1]
    _, ni, seqs = D.case_inputs(c)
    codes, users = scored_rows(c)
    return R.forward(w, E, L, ni, codes, seqs[users], dtype)


@pytest.mark.parametrize("c", FINITE, ids=D.case_id)
def test_float32_restatement_within_tolerance(c):
    w = D.case_inputs(c)[0]
    ref = forward_rows(c, w, np.float64)
    f32 = forward_rows(c, w, np.float32)
    err = np.abs(f32.astype(np.float64) - ref) / (D.ATOL + D.RTOL * np.abs(ref))
    print("%s: %d rows, float32 error / tolerance: max %.3f" % (D.case_id(c), ref.size, err.max()))
    assert D.close(f32, ref).all(), err.max()


def faulty(c, fault):
    """float64 logits of the case's rows with one term of the per-user form wrong"""
    E, L = c[0], c[1]
    w, ni, seqs = D.case_inputs(c)
    codes, users = scored_rows(c)
    emb, W1, b1, w2, b2 = R.split(w, E, L, ni, np.float64)
    out = np.empty(codes.size)
    for u in np.unique(users):
        m = users == u
        K = R.lookup(emb, seqs[u])
        s = K.sum(0)
        cc = (s @ s - (K * K).sum()) / 2.0 + b2
        a = W1[:, E:] @ K.reshape(-1) + b1
        e = R.lookup(emb, codes[m])
        W1a = W1[:, :E] * (1.05 if fault == "w1a" else 1.0)
        deep = np.maximum(e @ W1a.T + a[None, :], 0.0) @ w2
        out[m] = (0.0 if fault == "es" else e @ s) + (0.0 if fault == "c" else cc) + (0.0 if fault == "deep" else deep)
    return out


@pytest.mark.parametrize("c", FINITE, ids=D.case_id)
def test_tolerance_sees_kernel_faults(c):
    w = D.case_inputs(c)[0]
    ref = forward_rows(c, w, np.float64)
    assert D.close(faulty(c, None), ref).all()                      # the per-user form itself is the graph
    for fault in ("es", "c", "deep", "w1a"):
        out = 1.0 - D.close(faulty(c, fault), ref).mean()
        print("%s: fault %-4s moves %.1f %% of %d rows out of tolerance" % (D.case_id(c), fault, 100 * out, ref.size))
        if fault == "es":
            # an all-pad history has s = 0: e.s is absent from the graph itself; the condition is on the users that have a history
            # (user 1 everywhere; at L = 1 also every user whose one position is a pad)
            has_history = (D.case_inputs(c)[2] >= 0).any(1)[scored_rows(c)[1]]
            assert has_history.mean() >= 0.5
            out = 1.0 - D.close(faulty(c, fault), ref)[has_history].mean()
        assert out >= 0.9, (fault, out)


# ---- (c) the replay is a test: it fails on the three corruptions
def synthetic_trace(c):
    """what a correct device would return for the case: the float32 restatement's search, laid out as the device's trace"""
    E, L, beam, leaf_level, U, kind = c
    w, ni, seqs = D.case_inputs(c)
    U = 3
    counts = D.level_counts(beam, leaf_level)
    cap = D.trace_cap(beam)
    tc = np.zeros((U, len(counts), cap), np.int32); ts = np.zeros((U, len(counts), cap), np.float32); tn = np.zeros((U, len(counts)), np.int32)
    ids = np.full((U, 2 * beam), -1, np.int32); sc = np.zeros((U, 2 * beam), np.float32); cnt = np.zeros(U, np.int32)
    for u in range(U):
        for it, (lc, ls) in enumerate(D.search(w, E, L, ni, seqs[u], beam, leaf_level, np.float32)):
            tc[u, it, :lc.size] = lc; ts[u, it, :lc.size] = ls; tn[u, it] = lc.size
        ids[u, :lc.size] = lc; sc[u, :lc.size] = ls; cnt[u] = lc.size
    ref = lambda u, codes: D.ref_scores(w, E, L, ni, codes, seqs[u])
    return seqs[:U], (ids, sc, cnt), (tc, ts, tn), ref


def test_replay_detects_corruptions():
    c = (16, 10, 21, 9, 33, "twins")
    beam, leaf_level = c[2], c[3]
    seqs, outs, trace, ref = synthetic_trace(c)
    worst, ties = D.replay(seqs, beam, leaf_level, outs, trace, ref)
    assert worst <= 1.0 and ties > 0                                  # the intact trace passes, and its cuts fall on ties
    copy = lambda t: tuple(a.copy() for a in t)
    # two swapped codes (their scores swapped with them: only the order is wrong)
    o, t = copy(outs), copy(trace)
    t[0][0, 2, [0, 2]] = t[0][0, 2, [2, 0]]; t[1][0, 2, [0, 2]] = t[1][0, 2, [2, 0]]
    with pytest.raises(AssertionError, match="codes"):
        D.replay(seqs, beam, leaf_level, o, t, ref)
    # a tie broken the wrong way: the kept member of the pair the cut divides is the second one, not the first
    o, t = copy(outs), copy(trace)
    tc, ts, tn = t
    u, it = 0, 1
    n = int(tn[u, it])
    order = D.stable_argsort_desc(ts[u, it, :n].astype(np.float64))
    a, b = int(order[beam - 1]), int(order[beam])
    assert ts[u, it, a] == ts[u, it, b] and a < b
    kept = np.r_[order[:beam - 1], b]
    wrong = np.stack([2 * tc[u, it, kept] + 1, 2 * tc[u, it, kept] + 2], 1).reshape(-1)
    tc[u, it + 1, :wrong.size] = wrong
    with pytest.raises(AssertionError, match="codes"):
        D.replay(seqs, beam, leaf_level, o, t, ref)
    # one score off by twice the tolerance
    o, t = copy(outs), copy(trace)
    v = np.float64(t[1][1, 0, 5])
    t[1][1, 0, 5] = np.float32(v + 2.0 * (D.ATOL + D.RTOL * abs(v)))
    with pytest.raises(AssertionError, match="score"):
        D.replay(seqs, beam, leaf_level, o, t, ref)
    # the outputs are the last level's trace, byte for byte
    o, t = copy(outs), copy(trace)
    o[1][2, 3] = np.nextafter(o[1][2, 3], np.float32(np.inf))
    with pytest.raises(AssertionError, match="outputs"):
        D.replay(seqs, beam, leaf_level, o, t, ref)


def test_replay_nan_orders_first():
    """a NaN score is the greatest under Double.compare: first in the descending order, and the tolerance asks for NaN where the
    reference is NaN"""
    c = (16, 10, 20, 9, 33, "nan")
    seqs, outs, trace, ref = synthetic_trace(c)
    D.replay(seqs, c[2], c[3], outs, trace, ref)
    tc, ts, tn = trace
    i = int(np.flatnonzero(tc[0, 0, :tn[0, 0]] == D.NAN_CODE)[0])
    assert np.isnan(ts[0, 0, i]) and tc[0, 1, 0] == 2 * D.NAN_CODE + 1 and tc[0, 1, 1] == 2 * D.NAN_CODE + 2
    t = tuple(a.copy() for a in trace)
    t[1][0, 0, i] = 0.0
    with pytest.raises(AssertionError):
        D.replay(seqs, c[2], c[3], outs, t, ref)


# ---- (d)
@pytest.mark.parametrize("beam", (20, 3))
def test_pseudo_targets_are_compute_targets_with_equal_predictions(beam):
    from oracle import otm_oracle as oo
    targets = D.ragged_targets()
    leaf = D.RAGGED_TARGETS_LEAF
    _, s = D.level_start(beam)
    seqs = np.zeros((len(targets), 10), np.int32)
    want = oo.optimal_pseudo_targets(None, targets, seqs, 10, s, leaf, pred_fn=lambda nodes, rows: np.full(len(nodes), 0.25))
    got = D.pseudo_targets(targets, beam, leaf, "pseudo")
    assert len(got) == len(want) == leaf - s
    for lv in range(len(got) - 1):                                    # (the oracle's leaf level is a dict: a repeated target collapses)
        for u in range(len(targets)):
            assert got[lv][u] == list(want[lv][u].items()), (lv, u)
            assert all(lab == 1.0 for _, lab in got[lv][u])
    for u in range(len(targets)):
        assert got[-1][u] == [(t, 1.0) for t in targets[u]] and dict(got[-1][u]) == want[-1][u]
    normal = D.pseudo_targets(targets, beam, leaf, "normal")
    for lv in range(len(normal)):
        for u in range(len(targets)):
            assert [n for n, _ in normal[lv][u]] == [((t + 1) >> (leaf - s - 1 - lv)) - 1 for t in targets[u]]      # the ancestor on level s + 1 + lv


# ---- (e)
def test_header_and_bindings_declare_the_entry_points():
    from dismember_amd import _native as N
    header = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(dm_handle_t h," % name, header, re.M), name
        assert name in N.SIGNATURES, name
    assert len(N.SIGNATURES["dm_deepfm_otm_beam_search"][1]) == len(N.SIGNATURES["dm_otm_beam_search"][1])
    assert len(N.SIGNATURES["dm_deepfm_otm_beam_search_trace"][1]) == len(N.SIGNATURES["dm_otm_beam_search_trace"][1])
    assert len(N.SIGNATURES["dm_deepfm_otm_beam_search_dev"][1]) == len(N.SIGNATURES["dm_otm_beam_search_dev"][1])
    assert N.SIGNATURES["dm_deepfm_otm_pseudo_targets"] == N.SIGNATURES["dm_otm_pseudo_targets"]
    assert N.SIGNATURES["dm_deepfm_otm_train_batch"] == N.SIGNATURES["dm_otm_train_batch"]
