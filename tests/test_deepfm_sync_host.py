"""CPU tests of the DeepFM gradient exchange's restatement (tests/deepfm_sync_ref.py) and of the cases the GPU tests run; and that the ABI
declares and binds the entry point."""
import os
import re

import numpy as np
import pytest

import deepfm_sync_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _local_gradients(c):
    """a made-up gradient per rank with the support a real one has: the batch's rows and the tail; magnitudes 37^rank apart.  A rank with an
    empty batch holds zeros."""
    E, L, NI = c["E"], c["L"], c["NI"]
    out = []
    for r, (codes, seqs, y) in enumerate(c["batches"]):
        rng = np.random.default_rng(900 + r)
        g = np.zeros(NI * E + S.tail_len(E, L), np.float32)
        rows = S.batch_rows(codes, seqs, NI)
        if codes.size:
            g[:NI * E].reshape(NI, E)[rows] = (rng.standard_normal((rows.size, E)) * 37.0 ** r).astype(np.float32)
            g[NI * E:] = (rng.standard_normal(S.tail_len(E, L)) * 37.0 ** r).astype(np.float32)
        out.append((rows, g))
    return out


@pytest.mark.parametrize("name", S.CASES)
def test_restatement_equals_the_dense_rank_ordered_sum(name):
    c = S.case(name)
    E, NI = c["E"], c["NI"]
    local = _local_gradients(c)
    union, acc, tail = S.exchange([S.split(g, rows, E, NI) for rows, g in local], E, NI)
    got = S.assemble(union, acc, tail, E, NI)
    want = S.dense_sum([g for _, g in local])
    assert np.array_equal(got, want)
    assert np.array_equal(union, np.unique(np.concatenate([rows for rows, _ in local])))
    if c["W"] == 3:
        # the order is part of the result: three ranks in reversed order give other bytes (two ranks cannot show it, a + b == b + a)
        assert not np.array_equal(S.dense_sum([g for _, g in local][::-1]), want)


def test_every_case_has_the_structure_it_names():
    rows = lambda name: [S.batch_rows(b[0], b[1], S.case(name)["NI"]) for b in S.case(name)["batches"]]
    for name in ("shared_w2", "shared_w3"):
        c, rr = S.case(name), rows(name)
        assert c["W"] == int(name[-1]) == len(rr) and (c["E"], c["L"], c["NI"]) == (16, 10, 8191) and all(b[0].size == 96 for b in c["batches"])
        common = functools_reduce_intersect(rr)
        # 768 live history slots per rank over 400 ids: a rank reaches an id with probability 1 - (399 / 400)^768 = 0.85, every one of
        # three ranks does with 0.62 -- more than half of the vocabulary is shared by ALL ranks
        assert common.size > 200
        for r, b in enumerate(c["batches"]):
            assert set(np.unique(b[2]).tolist()) == {0.0, 37.0 ** r}
    a, b = rows("disjoint")
    assert np.intersect1d(a, b).size == 0 and a.size > 500 and b.size > 500
    c = S.case("empty_rank")
    assert c["batches"][1][0].size == 0 and c["batches"][0][0].size == 96 and c["batches"][1][1].shape == (0, c["L"])
    c = S.case("one_row_and_513_identical")
    assert c["batches"][0][0].size == 1 and c["batches"][1][0].size == 513
    assert np.unique(c["batches"][1][1], axis=0).shape[0] == 1 and np.unique(c["batches"][1][0]).size == 1
    a, b = rows("one_row_and_513_identical")
    assert 7 in a and 7 in b
    assert S.case("embed_24")["E"] == 24 and S.case("seq_len_32")["L"] == 32
    a, b = rows("tile_4095_4097")
    assert (a.size, b.size) == (4095, 4097)                           # one below and one above the compaction's tile of 4096
    for name in S.CASES:
        c = S.case(name)
        for codes, seqs, y in c["batches"]:
            assert codes.dtype == np.int32 and seqs.dtype == np.int32 and y.dtype == np.float32 and seqs.shape == (codes.size, c["L"])
            assert codes.size == 0 or (max(codes.max(), seqs.max()) < c["NI"] and min(codes.min(), seqs.min()) >= -1)


def functools_reduce_intersect(arrays):
    out = arrays[0]
    for a in arrays[1:]:
        out = np.intersect1d(out, a)
    return out


def test_header_declares_and_binding_binds_the_entry_point():
    from dismember_amd import _native as N
    src = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", src))
    assert "dm_deepfm_train_sync_gradients" in declared
    assert "dm_deepfm_train_sync_gradients" in N.SIGNATURES
    jni = open(os.path.join(ROOT, "jni", "dismember_jni.c")).read()
    scala = open(os.path.join(ROOT, "scala", "com", "mass", "hip", "Native.scala")).read()
    assert "dm_deepfm_train_sync_gradients(" in jni and re.search(r"deepfm_?[Tt]rain_?[Ss]ync_?[Gg]radients", scala)
