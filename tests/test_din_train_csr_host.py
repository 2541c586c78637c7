"""CPU tests of the ragged (CSR) user-grouped DIN training step's restatement (tests/din_train_csr_ref.py): it equals the float64 row
step of tests/train_ref.py on the expanded rows, also with its rowless users removed; the committed tolerances reproduce; the bound sees
every named fault in every case that can show it; the GPU cases hold the structures they name; the ABI declares and binds the two entry
points."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import train_ref as R
import din_train_csr_ref as S

NAMES = ("dm_train_forward_backward_csr_dev", "dm_tdm_sample_train_batch_csr_dev")


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
    import make_din_train_csr_tolerances as M
    return M, M.all_cases()


def _ref(case):
    w, E, L, seq, umask, row_off, codes, y = case
    return S.row_reference(w, E, L, seq, umask, row_off, codes, y)


def test_float64_csr_equals_the_row_step_on_the_expanded_rows():
    _, cases = _cases()
    worst = 0.0
    for name, case in cases.items():
        w, E, L, seq, umask, row_off, codes, y = case
        ref = _ref(case)
        for reverse in (False, True):
            o = S.step_csr(w, E, L, S.NUM_INDEX, seq, umask, row_off, codes, y, reverse=reverse)
            r, zeros_exact = R.tensor_ratios(o["g"], ref, S.EPS32, E, S.NUM_INDEX)       # EVERY element: |g - ref| <= 2^-20 eps32 A
            assert zeros_exact, (name, reverse)
            worst = max(worst, max(r.values()))
            for t, v in r.items():
                assert v <= 2.0 ** -20, (name, reverse, t, v)
            assert abs(o["loss"] - ref["loss"]) <= 2.0 ** -20 * S.EPS32 * max(1.0, abs(ref["loss"])), (name, reverse)
    print("worst float64 difference: %.3g eps32 A" % worst)


def test_rowless_users_removed_give_the_same_float64_result():
    _, cases = _cases()
    seen = 0
    for name, case in cases.items():
        w, E, L, seq, umask, row_off, codes, y = case
        if (np.diff(row_off) > 0).all():
            continue
        seen += 1
        seq2, um2, off2 = S.drop_rowless(seq, umask, row_off)
        assert seq2.shape[0] < seq.shape[0] and off2[-1] == row_off[-1]
        a = S.step_csr(w, E, L, S.NUM_INDEX, seq, umask, row_off, codes, y)
        b = S.step_csr(w, E, L, S.NUM_INDEX, seq2, um2, off2, codes, y)
        assert a["loss"] == b["loss"] and a["g"].tobytes() == b["g"].tobytes(), name
    assert seen >= 8


def test_committed_tolerances_reproduce():
    M, cases = _cases()
    want = json.load(open(M.PATH))
    assert want["margin"] == 8.0 and sorted(want["cases"]) == sorted(cases)
    assert sorted(want["k"]) == sorted(R.TENSORS)
    for t in M.CLASSES:
        assert want["k"][t] == pytest.approx(8.0 * max(c[t] for c in want["cases"].values()), rel=1e-12) and want["k"][t] > 0
    for name in sorted(cases):                                         # every case re-measured: an edited ratio does not pass
        for t, v in M.measure(*cases[name]).items():
            assert v == pytest.approx(want["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_the_bound_sees_every_fault_in_every_case():
    M, cases = _cases()
    K = json.load(open(M.PATH))["k"]
    shown = {f: 0 for f in S.FAULTS}
    for name, case in cases.items():
        w, E, L, seq, umask, row_off, codes, y = case
        ref = _ref(case)
        o = S.step_csr(w, E, L, S.NUM_INDEX, seq, umask, row_off, codes, y)
        scale = R.element_scale(ref["A"], E, S.NUM_INDEX)
        for t, (a, b) in R.sections(E, S.NUM_INDEX).items():          # the step itself is inside
            assert (np.abs(o["g"][a:b] - ref["g"][a:b]) <= K[t] * S.EPS32 * scale[a:b]).all(), (name, t)
        for fault in S.applicable_faults(E, seq, umask, row_off):
            assert S.fault_seen(case, fault, ref, K), (name, fault)
            shown[fault] += 1
    # every fault is shown somewhere; the ones no structure restricts, in every case
    assert all(shown.values()), shown
    assert shown["last_row_of_user_dropped"] == len(cases)
    # the exemptions, by name
    app = lambda n: set(S.applicable_faults(cases[n][1], cases[n][3], cases[n][4], cases[n][5]))
    assert app("single") <= {"last_row_of_user_dropped", "attT_dT_dropped"}      # one user, one row, one history position
    assert "g_of_previous_user" not in app("ends_empty") | app("only_last") | app("single")
    assert "scale_of_padded_E" in app("E24-L15") and "scale_of_padded_E" not in app("E32-L16")
    assert "mask_ignored_in_ds" in app("all_masked_keys-masked") and "mask_ignored_in_ds" not in app("all_masked_keys-nomask")
    assert {"g_of_previous_user", "last_row_of_user_dropped", "attT_dT_dropped", "dq_without_ds_k"} <= app("tdm-E128-L10") & app("tdm-E128-L16")


def test_gpu_cases_have_their_structure_and_margin():
    cnt = {n: np.asarray(c[2]) for n, c in S.CASES.items()}
    assert S.NUM_INDEX == 1023
    assert tuple(cnt["mixed8"]) == (1, 16, 0, 17, 15, 0, 0, 2) and S.CASES["mixed8"][:2] == (16, 1)
    assert tuple(cnt["ends_empty"]) == (0, 5, 0)
    c = cnt["only_last"]
    assert c.size == 17 and not c[:16].any() and c[16] > 0
    c = cnt["ones_then_513"]
    assert (c[:16] == 1).all() and c[16] == 513 and c.size == 17
    assert tuple(cnt["single"]) == (1,)
    c = cnt["empty_tile"]
    assert c.size == 48 and (c[16:32] == 0).all() and (c[:16] > 0).all() and (c[32:] > 0).all()
    assert S.CASES["E24-L15"][:2] == (24, 15) and S.padded_E(24) == 32 and S.CASES["E32-L16"][:2] == (32, 16)
    for n, (e, l) in {"tdm-E128-L10": (128, 10), "tdm-E128-L16": (128, 16)}.items():
        assert S.CASES[n][:2] == (e, l) and cnt[n].size == 19 and set(cnt[n]) == {41, 47}
    assert tuple(cnt[S.GRID_CASE]) == (1, 16, 0, 17, 15, 0, 0, 2) * 25
    tiles = int(((cnt[S.GRID_CASE] + 15) // 16).sum())
    assert cnt[S.GRID_CASE].size > 8 and tiles > 8                      # more users and more tiles than a grid of 2 has waves
    for name in S.CASES:
        w, E, L, seq, umask, row_off, codes, y = S.shape_case(name)
        U = cnt[name].size
        assert seq.shape == (U, L) and umask.shape == (U,) and umask.dtype == np.uint32 and (umask == S.pad_mask(seq)).all()
        assert row_off.shape == (U + 1,) and row_off.dtype == np.int64 and (np.diff(row_off) == cnt[name]).all()
        assert codes.shape == y.shape == (row_off[-1],) and w.dtype == np.float32
        assert _ref((w, E, L, seq, umask, row_off, codes, y))["relu_margin"] >= S.MARGIN
    assert S.STRUCT_COUNTS == (7, 0, 5, 9, 3, 6, 0, 8) and S.STRUCT_L == 10
    for name in S.STRUCTURES:
        for with_mask in (True, False):
            case = S.structure_case(name, with_mask)
            w, E, L, seq, umask, row_off, codes, y = case
            assert tuple(np.diff(row_off)) == S.STRUCT_COUNTS and (umask is not None) == with_mask
            ref = _ref(case)
            assert ref["relu_margin"] >= S.MARGIN and np.isfinite(ref["loss"])
            if name == "all_pad_history":
                assert (seq[2] == -1).all() and S.STRUCT_COUNTS[2] > 0
            elif name == "all_masked_keys" and with_mask:
                assert umask[4] == (1 << L) - 1 and (seq[4] >= 0).any()
            elif name == "one_key_user":
                assert (seq[2] >= 0).sum() == 1
            elif name == "user_codes_minus_one":
                assert (codes[row_off[3]:row_off[4]] == -1).all() and row_off[4] > row_off[3]
            elif name == "candidate_in_own_history":
                assert (seq[3] == codes[row_off[3] + 4]).sum() >= 2
            elif name == "id_twice_in_history":
                assert seq[3, 1] == seq[3, 7] >= 0
            elif name == "unmasked_pads":
                assert (seq[3, :4] == -1).all() and (umask is None or umask[3] == 0)
            elif name.startswith("saturated"):
                c_, s_, pad, yy = S.expand(seq, umask, row_off, codes, y)
                from helpers import numpy_din_forward
                x = numpy_din_forward(w, E, L, S.NUM_INDEX, c_, s_, pad)
                assert np.abs(x).min() > 40 and (x > 0).all() == (name == "saturated_pos") and 0 < y.mean() < 1


def test_header_declares_and_binding_binds_the_entry_points():
    N = _declared()
    assert len(N.SIGNATURES[NAMES[0]][1]) == 10 and len(N.SIGNATURES[NAMES[1]][1]) == 15
    shim = open(os.path.join(ROOT, "jni", "dismember_jni.c")).read()
    for name in NAMES:
        assert name + "(" in shim, name
