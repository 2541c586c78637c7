"""CPU tests of the sample-grouped Deep-Retrieval training step's yardstick: the grouped algebra restated in numpy
(tests/dr_train_grouped_ref.py) equals the row restatement (tests/dr_train_ref.py) on the expanded batch, the structure of every batch
tests/test_gpu_dr_train_grouped.py runs, the tolerance file's provenance, the declarations."""
import json
import os
import re

import numpy as np
import pytest

import dr_train_grouped_ref as G
import dr_train_ref as R
from dismember_amd.dr_train import DRTrainer, expand_batch, param_sections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = json.load(open(os.path.join(GOLDEN, "dr_train_grouped_tolerances.json")))
CHEAP = sorted(n for n in G.CASES if n.endswith("f64") and not n.startswith(("c5-like", "same-sample")))


@pytest.mark.parametrize("name", CHEAP)
@pytest.mark.parametrize("rev", [(False, False), (True, False), (False, True), (True, True)])
def test_grouped_algebra_equals_the_row_step_on_the_expanded_batch(name, rev):
    c, ref = G.make_case(name), G.reference(name)
    got = G.step(c["w"], c["dims"], c["seq"], c["paths"], reverse_samples=rev[0], reverse_paths=rev[1])
    k = TOL["f64"]["k"]
    ratios, zeros_exact = R.class_ratios(got["g"], ref, R.EPS["f64"], c["dims"])
    assert zeros_exact                                                 # elements whose A is 0 are exactly 0
    for t in R.CLASSES:
        assert ratios[t] <= k[t], (t, ratios[t])
    assert G.loss_ratio(got["loss"], ref, R.EPS["f64"]) <= k["loss"]
    only = G.step(c["w"], c["dims"], c["seq"], c["paths"], reverse_samples=rev[0], reverse_paths=rev[1], loss_only=True)
    assert np.array_equal(only["loss"], got["loss"]) and not only["g"].any()


def test_expand_is_transform_layer_data():
    rng = np.random.default_rng(0)
    item_paths = rng.integers(0, 9, size=(30, 3, 2)).astype(np.int32)
    seqs = rng.integers(0, 30, size=(11, 4)).astype(np.int32)
    targets = rng.integers(0, 30, size=11)
    a, b = expand_batch(seqs, targets, item_paths)
    c, d = G.expand(seqs, item_paths[targets])
    assert np.array_equal(a, c) and np.array_equal(b, d)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_gpu_case_has_the_structure_it_names(name):
    c = G.make_case(name)
    K, D, L, E, S, J, kind, dt = G.CASES[name]
    seq, paths = c["seq"], c["paths"]
    assert seq.shape == (S, L) and paths.shape == (S, J, D) and c["dims"] == (E, L, K, D, G.NUM_ITEM) and (c["S"], c["J"]) == (S, J)
    assert seq.min() >= -1 and seq.max() < G.NUM_ITEM and paths.min() >= 0 and paths.max() < K
    assert (c["w"] == c["w"].astype(R.NP[dt])).all()                 # exactly representable in the device's type
    pad = seq == -1
    if kind == "nopad":
        assert not pad.any()
    if kind == "allpad":
        mid = np.flatnonzero(pad.all(axis=1))
        assert S // 2 in mid and 0 < S // 2 < S - 1 and not pad.all()
    if kind == "pad" and S * L >= 50:
        assert pad.any() and not pad.all()
    if kind == "duppaths":
        assert (paths[S // 2] == paths[S // 2, 0]).all() and J >= 2
        assert sum((paths[s] == paths[s, 0]).all() for s in range(S)) < S          # ... and others whose paths differ
    if kind == "same":
        assert (seq == seq[0, 0]).all() and (paths == paths[0, 0]).all() and seq[0, 0] >= 0
    stem = name.rsplit("-", 1)[0]
    R_ = S * J
    edges = {"s-63": S == 63 and J == 2, "s-64": S == 64 and J == 2, "s-65": S == 65 and J == 2,
             "slab-511": S == 511 and J == 1, "slab-512": S == 512 and J == 1, "slab-513": S == 513 and J == 1,
             "rows-513": R_ == 513 and S < 512, "rows-512": R_ == 512 and S < 512, "fwd-127": S == 127, "fwd-129": S == 129,
             "row-1023": K == 1023 and L == 1 and S == 2, "row-1024": K == 1024 and L == 1 and S == 2, "row-1025": K == 1025 and L == 1 and S == 2,
             "cache-13": D == 4 and L == 10 and L + D - 1 == 13, "c5-like": (K, D, L, E, S, J) == (100, 4, 10, 128, 43, 3),
             "grid-4096": R_ == 4096 and K == 7 and L == 1, "grid-4097": R_ == 4097 and K == 7 and L == 1,
             "tiny": (K, D, L, E, S, J) == (7, 2, 1, 16, 1, 1), "one-node": K == 1,
             "j-1": J == 1, "j-2": J == 2, "j-3": J == 3, "j-5": J == 5}
    assert edges.get(stem, True), name
    ref = G.reference(name)
    sec = param_sections(*c["dims"])
    touched = R.touched_rows(dict(dims=c["dims"], seq=seq, paths=paths.reshape(-1, D)))
    A_emb = ref["A"][slice(*sec["emb"])].reshape(-1, E)
    assert (A_emb[~touched] == 0).all()
    if K == 1:
        assert (ref["g"] == 0).all() and (ref["loss"] == 0).all()
        return
    assert (A_emb[touched] > 0).all()
    assert np.isfinite(ref["loss"]).all() and (ref["loss"] > 0).all()


def test_every_edge_the_kernels_have_is_among_the_cases():
    stems = {n.rsplit("-", 1)[0] for n in G.CASES}
    assert {"tiny", "one-node", "j-1", "j-2", "j-3", "j-5", "dup-paths", "same-sample", "all-pad-sample", "s-63", "s-64", "s-65", "slab-511", "slab-512",
            "slab-513", "rows-513", "rows-512", "fwd-127", "fwd-129", "row-1023", "row-1024", "row-1025", "cache-13", "c5-like", "grid-4096",
            "grid-4097"} <= stems
    assert {G.CASES[n][3] for n in G.CASES} >= {16, 32, 128}
    assert all(n[:-3] + "f32" in G.CASES and n[:-3] + "f64" in G.CASES for n in G.CASES)


def test_tolerance_file_matches_its_script():
    """the committed constants are what the script gives for a sample of cheap cases, and 8 x the largest ratio"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dr_train_grouped_tolerances", os.path.join(GOLDEN, "make_dr_train_grouped_tolerances.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    assert TOL["margin"] == 8.0
    for dt in ("f32", "f64"):
        assert sorted(TOL[dt]["cases"]) == sorted(n for n in G.CASES if n.endswith(dt))
        for t in R.CLASSES + ("loss",):
            assert TOL[dt]["k"][t] == pytest.approx(8.0 * max(c[t] for c in TOL[dt]["cases"].values()), rel=1e-12)
            assert TOL[dt]["k"][t] > 0
    for name in ("tiny-f32", "rows-513-f64", "s-63-f32", "j-5-f64"):
        got = mk.measure(name)
        for t, v in got.items():
            assert v == pytest.approx(TOL[name[-3:]]["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_declarations_exist():
    from dismember_amd import _native as N
    from dismember_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    for fn in ("dm_dr_train_forward_backward_grouped", "dm_dr_train_forward_backward_grouped_dev", "dm_dr_layer_loss"):
        assert re.search(r"\bint %s\(dm_handle_t h, const int32_t \*\w+, const int32_t \*\w+, int64_t S, int64_t J, double \*out_loss\);" % fn, header), fn
        assert fn in N.SIGNATURES and len(N.SIGNATURES[fn][1]) == 6
    for m in ("dr_train_forward_backward_grouped", "dr_train_forward_backward_grouped_dev", "dr_layer_loss"):
        assert callable(getattr(Engine, m))
    for m in ("evaluate_layer", "eval_loss_fn"):
        assert callable(getattr(DRTrainer, m))
    src = open(os.path.join(ROOT, "dismember_amd", "csrc", "dm_hip.hip")).read()
    assert src.index('#include "dr_train.hip.inc"') < src.index('#include "dr_train_grouped.hip.inc"')


def test_trainer_reads_the_environment_switch(monkeypatch):
    class FakeEngine:
        dr_dims = dict(num_item=5, D=2, L=3, K=4, E=16)
        calls = []

        def dr_train_init(self, **kw):
            pass

        def dr_train_forward_backward_grouped(self, seq, paths):
            self.calls.append(("grouped", np.shape(seq), np.shape(paths)))
            return np.zeros(2)

        def dr_train_forward_backward(self, seq, paths):
            self.calls.append(("row", np.shape(seq), np.shape(paths)))
            return np.zeros(2)

        def dr_adam_step(self, scale):
            pass

    paths = np.zeros((5, 3, 2), np.int32)
    seqs, targets = np.zeros((7, 3), np.int32), np.arange(7) % 5
    monkeypatch.delenv("DM_DR_TRAIN_GROUPED", raising=False)
    assert not DRTrainer(FakeEngine(), paths).grouped and DRTrainer(FakeEngine(), paths, grouped=True).grouped
    monkeypatch.setenv("DM_DR_TRAIN_GROUPED", "1")
    assert DRTrainer(FakeEngine(), paths).grouped and not DRTrainer(FakeEngine(), paths, grouped=False).grouped
    FakeEngine.calls.clear()
    DRTrainer(FakeEngine(), paths).step(seqs, targets)
    DRTrainer(FakeEngine(), paths, grouped=False).step(seqs, targets)
    assert FakeEngine.calls == [("grouped", (7, 3), (7, 3, 2)), ("row", (21, 3), (21, 2))]
