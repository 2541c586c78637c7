"""CPU tests of the DeepFM training step's reference (tests/deepfm_train_ref.py), of the committed tolerances and of the GPU cases;
and that the ABI declares and binds the training entry points."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import deepfm_ref as R
import deepfm_train_ref as T

NEW_NAMES = ("dm_deepfm_train_init", "dm_deepfm_train_free", "dm_deepfm_train_forward_backward", "dm_deepfm_train_forward_backward_dev",
             "dm_deepfm_adam_step", "dm_deepfm_train_param_count", "dm_deepfm_train_download", "dm_deepfm_make_train_batch",
             "dm_deepfm_sample_train_batch_dev")


def _small():
    E, L, NI, B = 8, 3, 40, 9
    rng = np.random.default_rng(5)
    w = R.random_deepfm_weights(rng, E, L, NI, std=0.3).astype(np.float64)
    codes = rng.integers(0, NI, B); seqs = rng.integers(0, NI, (B, L))
    seqs[1] = -1; codes[2] = -1; seqs[4, 1] = codes[4]; seqs[0, 0] = -1
    y = (rng.random(B) < 0.5).astype(np.float64)
    return w, E, L, NI, codes, seqs, y


def test_finite_differences_on_all_five_tensors():
    w, E, L, NI, codes, seqs, y = _small()
    o = T.step(w, E, L, NI, codes, seqs, y)
    assert o["relu_margin"].min() > 1e-4                      # (central differences of 1e-6 stay on one side of every kink)
    rng = np.random.default_rng(6)
    touched = np.unique(np.concatenate([codes, seqs.ravel()]))
    touched = touched[touched >= 0]
    for name, (a, b) in T.sections(E, L, NI).items():
        picks = rng.choice(np.arange(a, b), min(12, b - a), replace=False)
        if name == "emb":
            picks = np.concatenate([touched[:6] * E + rng.integers(0, E, touched[:6].size), picks[:4]])
        for i in picks:
            d = 1e-6
            wp, wm = w.copy(), w.copy()
            wp[i] += d; wm[i] -= d
            fd = (T.step(wp, E, L, NI, codes, seqs, y, loss_only=True)["loss"] - T.step(wm, E, L, NI, codes, seqs, y, loss_only=True)["loss"]) / (2 * d)
            assert abs(fd - o["g"][i]) <= 1e-6 * max(1.0, abs(fd)), (name, int(i), fd, o["g"][i])


def test_loss_and_logits_equal_the_forward_reference():
    for E, L in ((16, 1), (24, 10), (128, 32)):
        w, codes, seqs, y, _ = T.shape_case(E, L, 1) if (E, L, 1) in T.SHAPES else T.shape_case(E, L, 777)
        o = T.step(w, E, L, T.NUM_INDEX, codes, seqs, y, loss_only=True)
        z = R.forward(w, E, L, T.NUM_INDEX, codes, seqs)
        assert np.abs(o["z"] - z).max() <= 1e-12 * max(1.0, np.abs(z).max())
        yy = y.astype(np.float64)
        loss = float((np.maximum(z, 0) - z * yy + np.log1p(np.exp(-np.abs(z)))).mean())
        assert abs(o["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))


def test_committed_tolerances_reproduce():
    import make_deepfm_train_tolerances as M
    cases = M.all_cases()
    want = json.load(open(M.PATH))
    assert want["margin"] == 8.0 and sorted(want["cases"]) == sorted(cases)
    for t in M.CLASSES:
        assert want["k"][t] == pytest.approx(8.0 * max(c[t] for c in want["cases"].values()), rel=1e-12)
        assert want["k"][t] > 0
    for name in ("E16-L1-B17", "E24-L1-B1", "E16-L16-B1", "all_pad_history", "identical_rows_513"):
        for t, v in M.measure(*cases[name]).items():
            assert v == pytest.approx(want["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_gpu_cases_have_their_structure_margin_and_redraw_share():
    NI = T.NUM_INDEX
    assert {s[0] for s in T.SHAPES} >= {16, 24, 64, 128} and {s[1] for s in T.SHAPES} >= {1, 10, 14, 15, 16, 30, 31, 32}
    assert {s[2] for s in T.SHAPES} >= {1, 15, 16, 17, 511, 512, 513, 1025, 777}
    assert (128, 10, 777) in T.SHAPES and (128, 32, 777) in T.SHAPES
    for E, L, B in T.SHAPES + (T.GRID_CASE,):
        w, codes, seqs, y, share = T.shape_case(E, L, B)
        assert codes.shape == (B,) and seqs.shape == (B, L) and share <= T.MAX_REDRAWN
        assert T.step(w, E, L, NI, codes, seqs, y, loss_only=True)["relu_margin"].min() >= T.MARGIN
    E, L = 16, 10
    for name in T.STRUCTURES:
        w, codes, seqs, y, share = T.structure_case(name)
        assert share <= T.MAX_REDRAWN
        o = T.step(w, E, L, NI, codes, seqs, y, loss_only=True)
        assert o["relu_margin"].min() >= T.MARGIN and np.isfinite(o["loss"])
        if name == "all_pad_history":
            assert (seqs[3] == -1).all() and (seqs[17] == -1).all()
        elif name == "item_minus_one":
            assert codes[0] == -1 and codes[16] == -1 and (seqs[16] == -1).all()
        elif name == "item_in_own_history":
            assert (seqs[5] == codes[5]).sum() >= 2 and seqs[21, 0] == codes[21]
        elif name == "identical_rows_513":
            assert codes.size == 513 and (codes == codes[0]).all() and (seqs == seqs[0]).all() and (seqs[0] == codes[0]).any()
        elif name == "labels_all_0":
            assert not y.any()
        elif name == "labels_all_1":
            assert y.all()
        elif name.startswith("saturated"):
            assert np.abs(o["z"]).min() > 40 and (o["z"] > 0).all() == (name == "saturated_pos") and 0 < y.mean() < 1


def test_learning_case_reaches_four_fifths_under_numpy_adam():
    w0, batches, NI = T.learning_case()
    _, losses = T.train(w0, T.LEARN["E"], T.LEARN["L"], NI, batches, T.LEARN["lr"], T.LEARN["steps"])
    assert losses.min() <= 0.8 * losses[0], losses
    assert 0.2 < batches[0][2].mean() < 0.8


def test_header_declares_and_binding_binds_the_training_entry_points():
    from dismember_amd import _native as N
    src = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", src))
    for name in NEW_NAMES:
        assert name in declared, name
        assert name in N.SIGNATURES, name
