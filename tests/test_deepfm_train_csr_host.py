"""CPU tests of the ragged (CSR) user-grouped DeepFM training step's restatement (tests/deepfm_train_csr_ref.py): it equals the row step
on the expanded rows in float64 and the rectangular restatement on uniform offsets, the committed tolerances reproduce, the bound sees
seven named faults in every case that can show them, the GPU cases hold their structures, the sampler's test tree has leaves on two
levels, and the ABI declares and binds the two entry points."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import deepfm_train_ref as T
import deepfm_train_grouped_ref as G
import deepfm_train_csr_ref as S

NAMES = ("dm_deepfm_train_forward_backward_csr_dev", "dm_deepfm_sample_train_batch_csr_dev")


def _declared():
    from dismember_amd import _native as N
    src = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    have = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", src))
    for name in NAMES:
        assert name in have, name
        assert name in N.SIGNATURES, name
    return N


@pytest.fixture(autouse=True)
def _needs_the_entry_points():
    _declared()


def _cases():
    import make_deepfm_train_csr_tolerances as M
    return M, M.all_cases()


def test_float64_csr_equals_the_row_step_on_the_expanded_rows():
    M, cases = _cases()
    worst = 0.0
    for name, (w, E, L, seq, row_off, codes, y) in cases.items():
        ref = S.row_reference(w, E, L, seq, row_off, codes, y)
        for reverse in (False, True):
            o = S.step_csr(w, E, L, S.NUM_INDEX, seq, row_off, codes, y, reverse=reverse)
            r = T.ratios(o["g"], ref["g"], ref["A"], E, L, S.NUM_INDEX)
            r["loss"] = abs(o["loss"] - ref["loss"]) / (T.EPS32 * ref["A_loss"])
            worst = max(worst, max(r.values()))
            for t, v in r.items():
                assert v <= 2.0 ** -20, (name, reverse, t, v)
    print("worst float64 difference: %.3g eps32 A" % worst)


@pytest.mark.parametrize("shape", [(16, 1, 1, 1), (16, 1, 17, 1), (16, 1, 2, 40), (128, 10, 19, 41)])
def test_uniform_offsets_equal_the_rectangular_restatement(shape):
    """the same algebra on the same numbers: equal up to float64 rounding (the two restatements hand BLAS products of other shapes, so
    not bit for bit), in order and reversed, and with every shared fault the same wrong step"""
    E, L, U, Rr = shape
    w, seq, codes, y, _ = G.shape_case(*shape)
    row_off = S.offsets([Rr] * U)
    A = G.row_reference(w, E, L, seq, codes, y)
    tol = 2.0 ** -20 * T.EPS32
    for fault in (None,) + G.FAULTS:
        for reverse in (False, True) if fault is None else (False,):
            a = G.step_grouped(w, E, L, S.NUM_INDEX, seq, codes, y, reverse=reverse, fault=fault)
            b = S.step_csr(w, E, L, S.NUM_INDEX, seq, row_off, codes.reshape(-1), y.reshape(-1), reverse=reverse, fault=fault)
            assert abs(a["loss"] - b["loss"]) <= tol * A["A_loss"], (fault, reverse)
            assert (np.abs(a["g"] - b["g"]) <= tol * A["A"]).all(), (fault, reverse)


def test_committed_tolerances_reproduce():
    M, cases = _cases()
    want = json.load(open(M.PATH))
    assert want["margin"] == 8.0 and sorted(want["cases"]) == sorted(cases)
    for t in M.CLASSES:
        assert want["k"][t] == pytest.approx(8.0 * max(c[t] for c in want["cases"].values()), rel=1e-12) and want["k"][t] > 0
    for name in sorted(cases):                                         # every case re-measured: an edited ratio does not pass
        for t, v in M.measure(*cases[name]).items():
            assert v == pytest.approx(want["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_the_bound_sees_every_fault_in_every_case():
    M, cases = _cases()
    K = json.load(open(M.PATH))["k"]
    for name, (E, L, counts) in S.CASES.items():
        w, E, L, seq, row_off, codes, y = cases[name]
        ref = S.row_reference(w, E, L, seq, row_off, codes, y)
        assert not S.fault_seen(w, E, L, seq, row_off, codes, y, None, ref, K)          # the step itself is inside
        for fault in S.applicable_faults(counts):
            assert S.fault_seen(w, E, L, seq, row_off, codes, y, fault, ref, K), (name, fault)
    # the exemptions, by name: one user cannot read a neighbour, one populated user has no previous populated user
    exempt = {n: set(S.FAULTS) - set(S.applicable_faults(c[2])) for n, c in S.CASES.items()}
    assert exempt.pop("single") == {"hh_of_neighbour", "row_user_shifted"}
    assert exempt.pop("ends_empty") == {"row_user_shifted"} and exempt.pop("only_last") == {"row_user_shifted"}
    assert not any(exempt.values()) and S.FAULTS[:5] == G.FAULTS and len(S.FAULTS) == 7


def test_gpu_cases_have_their_structure_margin_and_redraw_share():
    cnt = {n: np.asarray(c[2]) for n, c in S.CASES.items()}
    assert tuple(cnt["mixed8"]) == (1, 16, 0, 17, 15, 0, 0, 2)
    off = S.offsets(cnt["mixed8"])
    users_of_tile = [len({int(np.searchsorted(off, r, "right") - 1) for r in range(t, min(t + 16, off[-1]))}) for t in range(0, off[-1], 16)]
    assert len(users_of_tile) == 4 and min(users_of_tile) >= 2         # every row tile straddles users, one across an empty user
    assert tuple(cnt["ends_empty"]) == (0, 5, 0)
    c = cnt["empty_tile"]
    assert c.size == 48 and (c[16:32] == 0).all() and set(c[:16]) | set(c[32:]) <= {1, 2, 3} and (c[:16] > 0).all() and (c[32:] > 0).all()
    c = cnt["ones_then_513"]
    assert (c[:16] == 1).all() and c[16] == 513 and c.size == 17       # the first row tile holds 16 users; 513 rows: two slabs of the rows' product
    assert tuple(cnt["single"]) == (1,)
    c = cnt["only_last"]
    assert c.size == 17 and not c[:16].any() and c[16] == 3
    c = cnt["u513"]
    assert c.size == 513 and (c == np.arange(513) % 4).all() and c.sum() > 512          # two slabs of both products
    for n, (e, l) in {"tdm-E24-L15": (24, 15), "tdm-E128-L10": (128, 10), "tdm-E128-L32": (128, 32)}.items():
        assert S.CASES[n][:2] == (e, l) and cnt[n].size == 19 and set(cnt[n]) == {41, 47}
    assert tuple(cnt[S.GRID_CASE]) == (1, 16, 0, 17, 15, 0, 0, 2) * 25
    assert (cnt[S.GRID_CASE].size + 15) // 16 > 8 and (cnt[S.GRID_CASE].sum() + 15) // 16 > 8      # more tiles than a grid of 2 has waves
    for name in S.CASES:
        w, E, L, seq, row_off, codes, y, share = S.shape_case(name)
        U = cnt[name].size
        assert seq.shape == (U, L) and row_off.shape == (U + 1,) and row_off.dtype == np.int64 and (np.diff(row_off) == cnt[name]).all()
        assert codes.shape == y.shape == (row_off[-1],) and share <= T.MAX_REDRAWN
        assert S.row_reference(w, E, L, seq, row_off, codes, y, loss_only=True)["relu_margin"].min() >= T.MARGIN
    for name in S.STRUCTURES:
        w, E, L, seq, row_off, codes, y, share = S.structure_case(name)
        assert share <= T.MAX_REDRAWN and tuple(np.diff(row_off)) == S.STRUCT_COUNTS and 0 in S.STRUCT_COUNTS
        o = S.row_reference(w, E, L, seq, row_off, codes, y, loss_only=True)
        assert o["relu_margin"].min() >= T.MARGIN and np.isfinite(o["loss"])
        if name == "all_pad_history":
            assert (seq[2] == -1).all() and S.STRUCT_COUNTS[2] > 0
        elif name == "user_codes_minus_one":
            assert (codes[row_off[3]:row_off[4]] == -1).all() and row_off[4] > row_off[3]
        elif name == "candidate_in_own_history":
            assert (seq[3] == codes[row_off[3] + 4]).sum() >= 2
        elif name.startswith("saturated"):
            assert np.abs(o["z"]).min() > 40 and (o["z"] > 0).all() == (name == "saturated_pos") and 0 < y.mean() < 1


def test_sampler_tree_has_leaves_on_two_levels_and_ragged_rows():
    import deepfm_train_csr_tree as Q
    codes = Q.leaf_codes()
    levels = {int(np.log2(c + 1)) for c in codes}
    assert len(levels) >= 2 and len(set(codes.tolist())) == codes.size
    per = {lv: sum(1 + Q.NEG[l] for l in range(Q.START_LEVEL, lv + 1)) for lv in levels}
    assert len(set(per.values())) >= 2                                 # the row counts of a batch differ ...
    seq, tgt = Q.targets()
    assert (tgt == 0).any() and (tgt > Q.N_ITEMS).any()                # ... and a padding target and one outside the tree give none
    want = Q.expected_counts(tgt)
    assert (want[(tgt == 0) | (tgt > Q.N_ITEMS)] == 0).all() and len(set(want[want > 0].tolist())) >= 2


def test_header_declares_and_binding_binds_the_entry_points():
    N = _declared()
    assert len(N.SIGNATURES[NAMES[0]][1]) == 9 and len(N.SIGNATURES[NAMES[1]][1]) == 14
