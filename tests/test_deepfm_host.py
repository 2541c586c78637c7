"""DeepFM, CPU side: the numpy restatement (tests/deepfm_ref.py) against itself in the two precisions and against the per-user
restructured form the level kernel computes, the parameter layout, and the declarations of the new entry points.

The GPU tests compare device scores with the float64 restatement under |gpu - ref64| <= 1e-5 + 1e-4 |ref64|.  The first test here
shows that the tolerance is not tighter than the reference's own float32 arithmetic on the very inputs those tests use."""
import os
import re

import numpy as np
import pytest

import deepfm_ref as R

RTOL, ATOL = 1e-4, 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("E", R.ROW_E)
@pytest.mark.parametrize("L", R.ROW_L)
def test_float32_restatement_within_tolerance_of_float64_rows(E, L):
    w, codes, seqs = R.row_case(E, L)
    r64 = R.forward(w, E, L, R.ROW_NUM_INDEX, codes, seqs, np.float64)
    r32 = R.forward(w, E, L, R.ROW_NUM_INDEX, codes, seqs, np.float32)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    ratio = np.abs(r32.astype(np.float64) - r64) / (ATOL + RTOL * np.abs(r64))
    print("E=%d L=%d float32 restatement error / tolerance: max %.3f" % (E, L, ratio.max()))
    assert ratio.max() <= 1.0
    # the all-pad history and the -1 item are rows like any other
    assert np.isfinite(r64[[5, 9]]).all()


@pytest.mark.parametrize("E", R.SEARCH_E)
@pytest.mark.parametrize("L", R.SEARCH_L)
def test_restatements_agree_on_search_inputs(E, L):
    """Every user of the search tests against a fixed sample of 128 tree nodes (a search scores a subset of the nodes)."""
    tree, w, seqs = R.search_case(E, L)
    NI = (1 << (R.SEARCH_DEPTH + 1)) - 1
    hist = R.history_codes(tree, seqs)
    assert (hist[1] == -1).all() and hist[2, -1] == 37
    nodes = np.random.default_rng(5).choice(tree["codes"], 128, replace=False).astype(np.int32)
    U = hist.shape[0]
    codes = np.tile(nodes, U)
    tiled = np.repeat(hist, nodes.size, axis=0)
    r64 = R.forward(w, E, L, NI, codes, tiled, np.float64)
    r32 = R.forward(w, E, L, NI, codes, tiled, np.float32)
    ratio = np.abs(r32.astype(np.float64) - r64) / (ATOL + RTOL * np.abs(r64))
    print("E=%d L=%d float32 restatement error / tolerance: max %.3f" % (E, L, ratio.max()))
    assert ratio.max() <= 1.0
    for u in range(U):      # the restructured per-user formula is the same function
        rs = R.forward_restructured(w, E, L, NI, nodes, hist[u], np.float64)
        assert np.abs(rs - r64[u * nodes.size:(u + 1) * nodes.size]).max() <= 1e-12


@pytest.mark.parametrize("E", R.ROW_E)
@pytest.mark.parametrize("L", R.ROW_L)
def test_restructured_formula_matches_direct_rows(E, L):
    w, codes, seqs = R.row_case(E, L)
    for row in (0, 5, 9, 16):
        tiled = np.tile(seqs[row], (codes.size, 1))
        direct = R.forward(w, E, L, R.ROW_NUM_INDEX, codes, tiled, np.float64)
        rs = R.forward_restructured(w, E, L, R.ROW_NUM_INDEX, codes, seqs[row], np.float64)
        assert np.abs(rs - direct).max() <= 1e-12


def test_parameter_count_and_block_offsets():
    for E, L, NI in ((16, 10, 1023), (24, 1, 7), (128, 32, 8191)):
        T = L + 1
        o = R.deepfm_offsets(E, L, NI)
        assert R.deepfm_param_count(E, L, NI) == NI * E + T * T * E + 2 * T + 1 == o["end"]
        assert (o["emb"], o["l1_w"]) == (0, NI * E)
        assert o["l1_b"] - o["l1_w"] == T * (T * E)          # Linear(T E, T): weight [out = T, in = T E]
        assert o["l2_w"] - o["l1_b"] == T and o["l2_b"] - o["l2_w"] == T and o["end"] - o["l2_b"] == 1
        w = np.arange(o["end"], dtype=np.float64)
        emb, W1, b1, w2, b2 = R.split(w, E, L, NI, np.float64)
        assert emb.shape == (NI, E) and W1.shape == (T, T * E) and b1.shape == (T,) and w2.shape == (T,)
        assert W1[1, 0] == o["l1_w"] + T * E and b2 == o["end"] - 1
    assert R.random_deepfm_weights(np.random.default_rng(0), 16, 10, 1023).dtype == np.float32


def test_entry_points_declared():
    from dismember_amd import _native
    header = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    for name in ("dm_load_weights_deepfm", "dm_deepfm_forward", "dm_get_scorer_kind"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _native.SIGNATURES, name
    # argument counts of the ctypes table match the header's declarations
    for name in ("dm_load_weights_deepfm", "dm_deepfm_forward", "dm_get_scorer_kind"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), name
