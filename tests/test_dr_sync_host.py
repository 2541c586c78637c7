"""CPU tests of the Deep-Retrieval gradient exchange's restatement (tests/dr_sync_ref.py), of the cases the GPU tests run, of the batch
slicing DRTrainer(comm=...) uses and of what data-parallel training computes; and that the ABI declares and binds the entry point."""
import os
import re

import numpy as np
import pytest

import dr_sync_ref as S
import dr_train_ref as R
from dismember_amd.dr_train import expand_batch, layer_slices, pack_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(name):
    c = S.case(name)
    return [S.batch_rows(seq, paths, c["dims"]) for seq, paths in c["batches"]]


def _local_gradients(c):
    """a made-up gradient per rank with the support a real one has: the batch's rows and the tail; magnitudes 37^rank apart.  An idle
    rank holds zeros."""
    T, dims = S.NP[c["dtype"]], c["dims"]
    NR, E = S.num_rows(dims), dims[0]
    out = []
    for r, (seq, paths) in enumerate(c["batches"]):
        rng = np.random.default_rng(900 + r)
        g = np.zeros(NR * E + S.tail_len(dims), T)
        rows = S.batch_rows(seq, paths, dims)
        if len(seq):
            g[:NR * E].reshape(NR, E)[rows] = (rng.standard_normal((rows.size, E)) * 37.0 ** r).astype(T)
            g[NR * E:] = (rng.standard_normal(S.tail_len(dims)) * 37.0 ** r).astype(T)
        out.append((rows, g))
    return out


def test_restatement_equals_the_dense_rank_ordered_sum_and_the_order_matters():
    order_seen = False
    for name in S.CASES:
        c = S.case(name)
        local = _local_gradients(c)
        union, acc, tail = S.exchange([S.split(g, rows, c["dims"]) for rows, g in local], c["dims"], c["dtype"])
        got = S.assemble(union, acc, tail, c["dims"])
        want = S.dense_sum([g for _, g in local])
        assert got.dtype == S.NP[c["dtype"]] and np.array_equal(got, want), name
        assert np.array_equal(union, np.unique(np.concatenate([rows for rows, _ in local]))), name
        if c["W"] == 3:
            # three ranks in reversed order give other bytes (two ranks cannot show it: a + b == b + a)
            order_seen = order_seen or not np.array_equal(S.dense_sum([g for _, g in local][::-1]), want)
    assert order_seen


def test_every_case_has_the_structure_it_names():
    for name in S.CASES:
        c = S.case(name)
        W, D, dt, NI, kind = S.SPECS[name]
        assert c["dims"] == (16, 4, 16, D, NI) and c["W"] == W == len(c["batches"]) and c["dtype"] == dt and name.endswith(dt)
        for seq, paths in c["batches"]:
            assert seq.dtype == np.int32 and paths.dtype == np.int32 and seq.shape == (len(paths), 4) and paths.shape == (len(seq), D)
            assert len(seq) == 0 or (-1 <= seq.min() and seq.max() < NI and 0 <= paths.min() and paths.max() < 16)
    assert {S.SPECS[n][:3] for n in S.CASES if n.startswith("shared")} == {(2, 2, "f64"), (2, 2, "f32"), (3, 3, "f64"), (3, 3, "f32")}
    for name in ("shared_w2_f64", "shared_w3_f32"):
        assert [len(b[0]) for b in S.case(name)["batches"]] == [7, 96, 300][:S.case(name)["W"]]
        assert any((b[0] == -1).any() for b in S.case(name)["batches"])
    # disjoint item rows; the node rows overlap
    NI = 64
    a, b = _rows("disjoint_items_f64")
    assert np.intersect1d(a[a < NI], b[b < NI]).size == 0 and a[a < NI].size > 20 and b[b < NI].size > 20
    assert np.intersect1d(a[a >= NI], b[b >= NI]).size > 8
    rr = _rows("identical_items_f32")
    assert all(np.array_equal(r[r < NI], rr[0][rr[0] < NI]) for r in rr) and rr[0][rr[0] < NI].size > 40
    c = S.case("all_padding_rank_f64")
    assert (c["batches"][0][0] == -1).any() and (c["batches"][0][0] >= 0).any() and (c["batches"][1][0] == -1).all() and len(c["batches"][1][0]) == 33
    a, b = _rows("all_padding_rank_f64")
    assert (b >= NI).all() and b.size > 0                            # nothing but node rows
    for name, idle, P in (("idle_middle_f64", 1, 2), ("idle_end_f32", 2, 2)):
        c = S.case(name)
        assert [len(b[0]) == 0 for b in c["batches"]] == [r == idle for r in range(3)] and c["P"] == P
        assert _rows(name)[idle].size == 0
    c = S.case("one_row_and_513_identical_f64")
    assert len(c["batches"][0][0]) == 1 and len(c["batches"][1][0]) == 513
    assert np.unique(c["batches"][1][0], axis=0).shape[0] == 1 and np.unique(c["batches"][1][1], axis=0).shape[0] == 1
    a, b = _rows("one_row_and_513_identical_f64")
    assert 7 in a and 7 in b
    for name, want in S.EXACT_ROWS.items():
        assert tuple(r.size for r in _rows(name)) == want, name
    assert [n % 2 for n in S.EXACT_ROWS["rows_odd_even_f64"]] == [1, 0] and [n % 2 for n in S.EXACT_ROWS["rows_even_odd_f64"]] == [0, 1]
    assert [n % 2 for n in S.EXACT_ROWS["rows_odd_odd_even_f64"]] == [1, 1, 0]
    assert S.ENV == {"adam_dense_f64": {"DM_ADAM_DENSE": "1"}} and all(S.case(n)["env"] == S.ENV.get(n, {}) for n in S.CASES)
    c, twin = S.case("adam_dense_f64"), S.case("one_row_and_513_identical_f64")
    assert c["w"] is twin["w"] and c["batches"] is twin["batches"]
    assert 4 * np.unique(np.concatenate(_rows("adam_dense_f64"))).size < S.num_rows(c["dims"])      # few enough rows for the active-rows path
    # the alignment rule: with ids padded to an even count and blocks sized in multiples of 8 bytes, every rows section and every tail
    # of an fp64 block starts 8-byte aligned in the receive buffer
    for name in S.CASES:
        c = S.case(name)
        off = 0
        for r in _rows(name):
            n = r.size
            assert (off + 4 * ((n + 1) // 2 * 2)) % 8 == 0
            off += S.block_bytes(n, c["dims"], c["dtype"])
            assert off % 8 == 0


def _reference_slices(B, W):
    """LocalOptimizer.trainLayerBatch (deep-retrieval/.../optim/LocalOptimizer.scala:142-149), written out"""
    task_size, extra_size = B // W, B % W
    parallelism = extra_size if task_size == 0 else W
    out = []
    for i in range(W):
        if i < parallelism:
            out.append((i * task_size + min(i, extra_size), task_size + (1 if i < extra_size else 0)))
        else:
            out.append(None)
    return out, parallelism


@pytest.mark.parametrize("W", [1, 2, 3])
def test_slicing_rule(W):
    for B in range(0, 3 * W + 2):
        got, P = layer_slices(B, W)
        want, P_ref = _reference_slices(B, W)
        assert P == P_ref and len(got) == W
        covered = []
        for i in range(W):
            if want[i] is None:
                assert got[i][1] == 0                                # a rank past P runs no step
            else:
                assert got[i] == want[i] and got[i][1] > 0
                covered += list(range(got[i][0], got[i][0] + got[i][1]))
        assert covered == list(range(B))


@pytest.mark.parametrize("W", [2, 4])
def test_mean_of_the_slices_gradients_is_the_whole_batch_gradient(W):
    """What DRTrainer(comm=...) computes when W divides B: (sum_r step(slice_r)) / W = step(whole) up to re-association of the B-term
    sums — |difference| <= B eps64 A per element, A the magnitude dr_train_ref.class_ratios measures against."""
    p = R.learning_problem()
    dims = p["dims"]
    w = pack_params(p["weights"])
    B = 64
    assert B % W == 0
    seq, paths = expand_batch(p["seqs"][:B], p["targets"][:B], p["item_paths"])
    whole = R.step(w, dims, seq, paths)
    slices, P = layer_slices(B, W)
    assert P == W
    parts = [R.step(w, dims, seq[lo:lo + n], paths[lo:lo + n]) for lo, n in slices]
    g = S.dense_sum([q["g"] for q in parts]) / W
    ratios, zeros_exact = R.class_ratios(g, whole, R.EPS["f64"], dims)
    print(ratios)
    assert zeros_exact and all(ratios[c] <= B for c in R.CLASSES), ratios
    assert max(ratios.values()) > 0                                  # (not the same sums: the slices re-associate them)
    loss = sum(q["loss"] for q in parts) / W
    assert (np.abs(loss - whole["loss"]) <= B * R.EPS["f64"] * whole["A_loss"]).all()


def test_header_declares_and_binding_binds_the_entry_point():
    from dismember_amd import _native as N
    src = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", src))
    assert "dm_dr_train_sync_gradients" in declared
    assert "dm_dr_train_sync_gradients" in N.SIGNATURES
    jni = open(os.path.join(ROOT, "jni", "dismember_jni.c")).read()
    assert "dm_dr_train_sync_gradients(" in jni
