"""CPU tests of the Deep-Retrieval training step's yardstick: the numpy restatement tests/dr_train_ref.py against the reference's
recorded cross-entropy answers, the serving oracle's logits and finite differences, the structure of every batch
tests/test_gpu_dr_train.py runs, and the tolerance file's provenance (tests/golden/make_dr_train_tolerances.py)."""
import json
import os

import numpy as np
import pytest

import dr_train_ref as R
from dismember_amd import synth
from dismember_amd.dr_train import expand_batch, pack_params, param_sections, split_params

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_cross_entropy_reproduces_the_recorded_answers():
    k = json.load(open(os.path.join(GOLDEN, "dr_train_known.json")))
    loss, grad, _ = R.softmax_ce(np.array(k["input"], np.float64), np.array(k["targets_zero_based"]))
    assert abs(loss - k["loss"]) < k["atol"]
    assert np.abs(grad.ravel() - np.array(k["grad"])).max() < k["atol"]


def test_logits_equal_the_serving_oracle():
    from oracle import pyoracle as po
    po.build()
    K, D, L, E, NI = 9, 3, 4, 16, 60
    rng = np.random.default_rng(3)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    orc = po.DeepRetrieval(wd, E, L, K, D, NI)
    seq, paths = R.make_batch(rng, K, D, L, 12, "allpad", num_item=NI)
    w = pack_params(wd)
    for d in range(D):
        Z = R.logits(w, (E, L, K, D, NI), seq, paths, d)
        for r in range(len(seq)):
            ids = list(seq[r]) + [NI + t * K + int(paths[r, t]) for t in range(d)]
            np.testing.assert_allclose(Z[r], orc.inference(ids, d), rtol=1e-12, atol=0)


def test_pack_and_split_are_inverse():
    K, D, L, E, NI = 5, 3, 2, 16, 11
    wd = synth.make_dr_model(NI, K, D, L, E, np.random.default_rng(0))
    w = pack_params(wd)
    assert w.size == list(param_sections(E, L, K, D, NI).values())[-1][1]
    back = split_params(w, E, L, K, D, NI)
    assert all((a == b).all() for a, b in zip(back["layer_w"], wd["layer_w"])) and (back["layer_emb"] == wd["layer_emb"]).all()
    assert all((a == b).all() for a, b in zip(back["layer_b"], wd["layer_b"]))


def test_gradient_against_central_differences():
    """200 random elements per tensor (all of a smaller one).  "1e-6 relative" is read per TENSOR: |fd - g_i| <= 1e-6 max(|g_i|, the
    tensor's largest |g|).  Central differences at h = 1e-5 in fp64 carry an absolute error of about eps |loss| / h = 1e-10 whatever
    the element's size, so agreement relative to each element alone would fail on the small ones for a reason that is not the gradient's."""
    K, D, L, E, NI, B = 6, 3, 3, 16, 30, 17
    dims = (E, L, K, D, NI)
    rng = np.random.default_rng(1)
    w = pack_params(synth.make_dr_model(NI, K, D, L, E, rng))
    seq, paths = R.make_batch(rng, K, D, L, B, "allpad", num_item=NI)
    ref = R.step(w, dims, seq, paths)
    total = lambda v: float(R.step(v, dims, seq, paths, loss_only=True)["loss"].sum())
    h = 1e-5
    for name, (a, b) in param_sections(*dims).items():
        live = a + np.flatnonzero(ref["A"][a:b] > 0)
        picks = rng.choice(live, min(200, live.size), replace=False)
        for i in picks:
            wp, wm = w.copy(), w.copy()
            wp[i] += h
            wm[i] -= h
            fd = (total(wp) - total(wm)) / (2 * h)
            assert abs(fd - ref["g"][i]) <= 1e-6 * max(abs(ref["g"][i]), np.abs(ref["g"][a:b]).max()), (name, i, fd, ref["g"][i])
    # rows nobody named and padding receive nothing
    assert (ref["g"][ref["A"] == 0] == 0).all()


def test_row_order_does_not_change_the_answer():
    c = R.make_case("all-pad-row-f64")
    a, b = R.reference("all-pad-row-f64"), R.step(c["w"], c["dims"], c["seq"], c["paths"], reverse=True)
    np.testing.assert_allclose(a["g"], b["g"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-14)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gpu_case_has_the_structure_it_names(name):
    c = R.make_case(name)
    K, D, L, E, B, kind, dt = R.CASES[name]
    seq, paths = c["seq"], c["paths"]
    assert seq.shape == (B, L) and paths.shape == (B, D) and c["dims"] == (E, L, K, D, R.NUM_ITEM)
    assert seq.min() >= -1 and seq.max() < R.NUM_ITEM and paths.min() >= 0 and paths.max() < K
    assert (c["w"] == c["w"].astype(R.NP[dt])).all()                 # exactly representable in the device's type
    pad = seq == -1
    if kind == "nopad":
        assert not pad.any()
    if kind == "allpad":
        assert pad.all(axis=1).any() and not pad.all()
    if kind == "pad" and B * L >= 50:
        assert pad.any() and not pad.all()
    if kind == "same":
        assert (seq == seq[0, 0]).all() and (paths == paths[0]).all() and seq[0, 0] >= 0
    if B >= 100 and kind != "same":                                   # duplicates: some row is named more than once
        ids = seq[seq >= 0]
        assert len(np.unique(ids)) < ids.size
    ref = R.reference(name)
    sec = param_sections(*c["dims"])
    A_emb = ref["A"][slice(*sec["emb"])].reshape(-1, E)
    touched = R.touched_rows(c)
    assert (A_emb[~touched] == 0).all() and (ref["g"][slice(*sec["emb"])].reshape(-1, E)[~touched] == 0).all()
    if K == 1:
        assert (ref["g"] == 0).all() and (ref["A"] == 0).all() and (ref["loss"] == 0).all()
        return
    assert (A_emb[touched] > 0).all()
    for d in range(D):
        assert (ref["A"][slice(*sec["b%d" % d])] > 0).all()
        _, X = R.inputs(c["w"][slice(*sec["emb"])].reshape(-1, E), seq.astype(np.int64), paths.astype(np.int64), d, R.NUM_ITEM, K)
        fed = (X != 0).any(axis=0)
        assert ((ref["A"][slice(*sec["W%d" % d])].reshape(K, -1) > 0) == fed[None, :]).all()
    assert np.isfinite(ref["loss"]).all() and (ref["loss"] > 0).all() and (ref["A_loss"] >= ref["loss"]).all()


def test_tolerance_file_matches_its_script():
    """the committed constants are what the script gives for a sample of cheap cases, and 8 x the largest ratio"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dr_train_tolerances", os.path.join(GOLDEN, "make_dr_train_tolerances.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    tol = json.load(open(os.path.join(GOLDEN, "dr_train_tolerances.json")))
    assert tol["margin"] == 8.0
    for dt in ("f32", "f64"):
        assert sorted(tol[dt]["cases"]) == sorted(n for n in R.CASES if n.endswith(dt))
        for t in R.CLASSES + ("loss",):
            assert tol[dt]["k"][t] == pytest.approx(8.0 * max(c[t] for c in tol[dt]["cases"].values()), rel=1e-12)
            assert tol[dt]["k"][t] > 0
    for name in ("tiny-f32", "slab-513-f64", "below-tile-f32"):
        got = mk.measure(name)
        for t, v in got.items():
            assert v == pytest.approx(tol[name[-3:]]["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_learning_case_learns_in_the_restatement():
    p = R.learning_problem()
    dims = p["dims"]
    seq, paths = expand_batch(p["seqs"], p["targets"], p["item_paths"])
    assert len(seq) == 256 and p["item_paths"].shape == (64, 1, 2)
    code = p["item_paths"][:, 0, 0] * dims[2] + p["item_paths"][:, 0, 1]
    assert (code[p["seqs"]] == code[p["targets"]][:, None]).all()        # histories share the target's path

    def grads(w):
        r = R.step(w, dims, seq, paths)
        return r["loss"], r["g"]
    losses = R.adam_reference(pack_params(p["weights"]), grads, p["steps"], p["lr"])
    assert (losses[-1] < 0.8 * losses[0]).all(), losses[[0, -1]]
