"""CPU tests of the user-grouped DeepFM training step's restatement (tests/deepfm_train_grouped_ref.py): it equals the row step on the
expanded rows in float64, the committed tolerances reproduce, the bound sees five named faults in every sweep case, the GPU cases hold
their structures, and the ABI declares and binds the entry point."""
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

NAME = "dm_deepfm_train_forward_backward_grouped_dev"


def _declared():
    from dismember_amd import _native as N
    src = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert NAME in set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", src)), NAME
    assert NAME in N.SIGNATURES, NAME
    return N


@pytest.fixture(autouse=True)
def _needs_the_entry_point():
    _declared()


def _cases():
    import make_deepfm_train_grouped_tolerances as M
    return M, M.all_cases()


def test_float64_grouped_equals_the_row_step_on_the_expanded_rows():
    M, cases = _cases()
    worst = 0.0
    for name, (w, E, L, seq, codes, y) in cases.items():
        ref = G.row_reference(w, E, L, seq, codes, y)
        for reverse in (False, True):
            o = G.step_grouped(w, E, L, G.NUM_INDEX, seq, codes, y, reverse=reverse)
            r = T.ratios(o["g"], ref["g"], ref["A"], E, L, G.NUM_INDEX)
            r["loss"] = abs(o["loss"] - ref["loss"]) / (T.EPS32 * ref["A_loss"])
            worst = max(worst, max(r.values()))
            for t, v in r.items():
                assert v <= 2.0 ** -20, (name, reverse, t, v)
    print("worst float64 difference: %.3g eps32 A" % worst)


def test_committed_tolerances_reproduce():
    M, cases = _cases()
    want = json.load(open(M.PATH))
    assert want["margin"] == 8.0 and sorted(want["cases"]) == sorted(cases)
    for t in M.CLASSES:
        drawn = max(c[t] for n, c in want["cases"].items() if n != M.LONG)
        assert want["k"][t] == pytest.approx(8.0 * drawn, rel=1e-12) and want["k"][t] > 0
        assert want["k_long_segment"][t] == pytest.approx(max(8.0 * drawn, 8.0 * want["cases"][M.LONG][t]), rel=1e-12)
    # re-measured: the case that sets each k (an edited worst ratio does not pass), and a few more
    setters = {max((n for n in want["cases"] if n != M.LONG), key=lambda n: want["cases"][n][t]) for t in M.CLASSES}
    for name in sorted(setters | {"E16-L1-U1-R17", "E24-L1-U1-R1", "E16-L16-U2-R1", "E16-L1-U513-R1", "all_pad_history", M.LONG}):
        for t, v in M.measure(*cases[name]).items():
            assert v == pytest.approx(want["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_the_bound_sees_every_fault_in_every_sweep_case():
    M, cases = _cases()
    K = json.load(open(M.PATH))["k"]
    for shape in G.SHAPES + (G.GRID_CASE,):
        w, E, L, seq, codes, y = cases[M.case_name(shape)]
        ref = G.row_reference(w, E, L, seq, codes, y)
        assert not G.fault_seen(w, E, L, seq, codes, y, None, ref, K)          # the step itself is inside
        for fault in G.applicable_faults(shape[2]):
            assert G.fault_seen(w, E, L, seq, codes, y, fault, ref, K), (shape, fault)
    assert G.applicable_faults(1) == G.FAULTS[:4] and G.applicable_faults(2) == G.FAULTS


def test_gpu_cases_have_their_structure_margin_and_redraw_share():
    assert {s[0] for s in G.SHAPES} >= {16, 24, 64, 128} and {s[1] for s in G.SHAPES} >= {1, 10, 15, 16, 31, 32}
    assert {s[3] for s in G.SHAPES} >= {1, 15, 16, 17, 40, 513} and {s[2] for s in G.SHAPES} >= {1, 2, 15, 16, 17, 33, 513}
    for e, l, u, r in G.SHAPES:                                        # every E, L and R of the sweeps also with two users
        assert u != 1 or (e, l, 2, r) in G.SHAPES
    assert (128, 10, 19, 41) in G.SHAPES and (128, 32, 19, 41) in G.SHAPES
    for E, L, U, R in G.SHAPES + (G.GRID_CASE,):
        w, seq, codes, y, share = G.shape_case(E, L, U, R)
        assert seq.shape == (U, L) and codes.shape == (U, R) and y.shape == (U, R) and share <= T.MAX_REDRAWN
        assert G.row_reference(w, E, L, seq, codes, y, loss_only=True)["relu_margin"].min() >= T.MARGIN
    E, L = 16, 10
    for name in G.STRUCTURES:
        w, seq, codes, y, share = G.structure_case(name)
        assert share <= T.MAX_REDRAWN
        o = G.row_reference(w, E, L, seq, codes, y, loss_only=True)
        assert o["relu_margin"].min() >= T.MARGIN and np.isfinite(o["loss"])
        if name == "all_pad_history":
            assert (seq[2] == -1).all()
        elif name == "user_codes_minus_one":
            assert (codes[1] == -1).all()
        elif name == "candidate_in_own_history":
            assert (seq[3] == codes[3, 4]).sum() >= 2
        elif name == "identical_histories":
            assert (seq[4] == seq[0]).all() and (seq[0] >= 0).any()
        elif name == "id_twice_in_history":
            assert seq[5, 1] == seq[5, 6] >= 0
        elif name == "long_segment":
            assert codes.shape == (3, 513) and (codes == codes[0, 0]).all() and codes[0, 0] >= 0
        elif name == "labels_all_0":
            assert not y.any()
        elif name == "labels_all_1":
            assert y.all()
        elif name.startswith("saturated"):
            assert np.abs(o["z"]).min() > 40 and (o["z"] > 0).all() == (name == "saturated_pos") and 0 < y.mean() < 1


def test_learning_case_regrouped_reaches_four_fifths_under_numpy_adam():
    w0, (seq, codes, y), NI = G.learning_case()
    assert seq.shape == (32, T.LEARN["L"]) and codes.shape == (32, 16) and 0.2 < y.mean() < 0.8
    _, losses = T.train(w0, T.LEARN["E"], T.LEARN["L"], NI, [G.expand(seq, codes, y)], T.LEARN["lr"], T.LEARN["steps"])
    assert losses.min() <= 0.8 * losses[0], losses


def test_header_declares_and_binding_binds_the_entry_point():
    N = _declared()
    assert len(N.SIGNATURES[NAME][1]) == 8
