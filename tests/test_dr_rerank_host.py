"""CPU tests of the rerank training step's yardstick: the numpy restatement tests/dr_rerank_ref.py against finite differences, the serving
oracle's rerank and the reference's own test property; its restated sampler; the structure of every batch tests/test_gpu_dr_rerank.py
runs; and the tolerance file's provenance (tests/golden/make_dr_rerank_tolerances.py)."""
import json
import os
import re

import numpy as np
import pytest

import dr_rerank_ref as R
from dismember_amd import synth
from dismember_amd.dr_train import init_rerank_weights, pack_rerank, split_rerank

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gradient_against_central_differences():
    """All five tensors, 200 random live elements each (all of a smaller one).  "1e-6" is read per TENSOR, as
    tests/test_dr_train_host.py reads it: |fd - g_i| <= 1e-6 max(|g_i|, the tensor's largest |g|) — central differences at h = 1e-5 carry
    an absolute error of about eps |loss| / h whatever the element's size."""
    E, L, NI, B, S = 16, 3, 30, 17, 5
    dims = (E, L, NI)
    rng = np.random.default_rng(1)
    w = {k: v for k, v in synth.make_dr_model(NI, 4, 2, L, E, rng).items() if k in R.TENSORS}
    seq, tg, neg = R.make_batch(rng, L, B, S, "allpad", num_item=NI)
    neg[3, 1] = neg[3, 0]                                   # a repeated negative and one that equals its row's target
    neg[4, 2] = tg[4]
    ref = R.step(w, dims, seq, tg, neg)
    total = lambda v: float(R.step(v, dims, seq, tg, neg, loss_only=True)["loss"])
    h = 1e-5
    for name in R.TENSORS:
        g = ref["g"][name].ravel()
        live = np.flatnonzero(ref["A"][name].ravel() > 0)
        assert live.size
        for i in rng.choice(live, min(200, live.size), replace=False):
            wp, wm = dict(w), dict(w)
            wp[name], wm[name] = w[name].copy(), w[name].copy()
            wp[name].ravel()[i] += h
            wm[name].ravel()[i] -= h
            fd = (total(wp) - total(wm)) / (2 * h)
            assert abs(fd - g[i]) <= 1e-6 * max(abs(g[i]), np.abs(g).max()), (name, i, fd, g[i])
        assert (g[ref["A"][name].ravel() == 0] == 0).all()      # rows nobody named and padding receive nothing


def test_user_vector_and_scores_equal_the_serving_oracle():
    from oracle import pyoracle as po
    po.build()
    K, D, L, E, NI = 5, 2, 4, 16, 60
    rng = np.random.default_rng(3)
    wd = synth.make_dr_model(NI, K, D, L, E, rng)
    orc = po.DeepRetrieval(wd, E, L, K, D, NI)
    seq, tg, neg = R.make_batch(rng, L, 12, 6, "allpad", num_item=NI)
    r = R.step(wd, (E, L, NI), seq, tg, neg, loss_only=True)
    for i in range(len(seq)):
        np.testing.assert_allclose(r["z"][i], orc.rerank(r["items"][i], seq[i]), rtol=1e-12, atol=1e-15)
    # the user vector alone: scores against an identity table are the vector itself
    eye = dict(wd, softmax_w=np.eye(NI, E), softmax_b=np.zeros(NI))
    orc2 = po.DeepRetrieval(eye, E, L, K, D, NI)
    for i in range(len(seq)):
        np.testing.assert_allclose(r["U"][i], orc2.rerank(np.arange(E), seq[i]), rtol=1e-12, atol=1e-15)


def test_pack_and_split_are_inverse():
    wd = init_rerank_weights(11, 2, 16, np.random.default_rng(0))
    g, s = pack_rerank(wd)
    assert g.size == 11 * 16 + 16 * 2 * 16 + 16 and s.size == 11 * 16 + 11
    back = split_rerank(g, s, 16, 2, 11)
    assert all((back[k] == wd[k]).all() and back[k].shape == wd[k].shape for k in R.TENSORS)
    assert (wd["rerank_b"] == 0).all() and (wd["softmax_b"] == 0).all() and 0.03 < wd["softmax_w"].std() < 0.07


def test_the_references_own_property_the_loss_falls_strictly():
    """SampledSoftmaxLossTest: B = 6, E = 10, S = 4, 200 classes, lr 7e-3, inputs uniform in +-0.05, weights N(0, 0.01), zero biases,
    fixed negatives, only the softmax tables move (accumulating gradient): the loss falls strictly over 7 steps.  The inputs reach the
    criterion as U through an identity Linear over one-item histories."""
    B, E, S, NI, lr = 6, 10, 4, 200, 7e-3
    rng = np.random.default_rng(2022)
    w = dict(rerank_emb=np.zeros((NI, E)), rerank_w=np.eye(E), rerank_b=np.zeros(E), softmax_w=rng.standard_normal((NI, E)) * 0.01,
             softmax_b=np.zeros(NI))
    w["rerank_emb"][:B] = rng.uniform(-0.05, 0.05, (B, E))
    seq = np.arange(B).reshape(B, 1)
    tg = rng.choice(NI, B, replace=False)
    neg = np.array([rng.choice(np.setdiff1d(np.arange(NI), [t]), S, replace=False) for t in tg])
    assert np.allclose(R.step(w, (E, 1, NI), seq, tg, neg, loss_only=True)["U"], w["rerank_emb"][:B])
    w1, losses = R.train(w, (E, 1, NI), [(seq, tg, neg)], lr, steps=7, accumulate=True, graph=False)
    assert (np.diff(losses) < 0).all(), losses
    assert (w1["rerank_emb"] == w["rerank_emb"]).all() and (w1["softmax_w"] != w["softmax_w"]).any()


@pytest.mark.parametrize("name", sorted(R.SAMPLER_CASES))
def test_restated_sampler(name):
    N, S, B = R.SAMPLER_CASES[name]
    tg = R.sampler_targets(name)
    assert set(tg) == set(range(N)) and 2 * S <= N
    for seed in R.SAMPLER_SEEDS:
        neg, fallbacks = R.sample(seed, 0, tg, S, N)
        assert fallbacks == 0                                       # the fallback is never reached on these inputs
        assert neg.shape == (B, S) and neg.min() >= 0 and neg.max() < N
        assert (np.diff(neg, axis=1) > 0).all()                     # ascending, hence distinct
        assert (neg != np.array(tg)[:, None]).all()
    other, _ = R.sample(R.SAMPLER_SEEDS[0], 1, tg[:64], S, N)
    assert (other != R.sample(R.SAMPLER_SEEDS[0], 0, tg, S, N)[0][:len(other)]).any() or N == 3
    if name == "n64-s8":
        # every id is drawn B (63/64) (8/63) = 4096 times in the mean; six standard deviations of that binomial (p = 1/8) are 359
        assert B == 32768 and abs(6 * np.sqrt(B * (1 / 8) * (7 / 8)) - 359) < 1
        counts = np.bincount(R.sample(R.SAMPLER_SEEDS[0], 0, tg, S, N)[0].ravel(), minlength=N)
        assert counts.min() >= 4096 - 359 and counts.max() <= 4096 + 359, (counts.min(), counts.max())


def test_sampler_fallback_finds_the_free_id():
    """num_item = S + 1: the last negative has one free id, so now and then it exhausts its draws; the row still comes out complete"""
    hit = 0
    for row in range(100):
        neg, fb = R.sample_row(1, 0, row, 3, 12, 13)
        hit += fb
        assert neg == [i for i in range(13) if i != 3]
    assert hit > 0


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gpu_case_has_the_structure_it_names(name):
    c = R.make_case(name)
    E, L, B, S, kind, dt = R.CASES[name]
    seq, tg, neg = c["seq"], c["targets"], c["negatives"]
    assert seq.shape == (B, L) and tg.shape == (B,) and neg.shape == (B, S) and c["dims"] == (E, L, R.NUM_ITEM)
    assert seq.min() >= -1 and seq.max() < R.NUM_ITEM and min(tg.min(), neg.min()) >= 0 and max(tg.max(), neg.max()) < R.NUM_ITEM
    assert all((c["weights"][k] == c["weights"][k].astype(R.NP[dt])).all() for k in R.TENSORS)      # exactly representable on the device
    pad = seq == -1
    if kind == "allpad":
        assert pad.all(axis=1).any() and not pad.all()
    if kind == "pad" and B * L >= 50 and L > 1:
        assert pad.any() and not pad.all()
    if kind == "rephist":
        assert (seq[:, 0] == seq[:, 1]).all() and (seq[0] == seq[0, 0]).all()
    if kind == "same":
        assert (seq == seq[0]).all() and (tg == tg[0]).all() and (neg == neg[0]).all() and B == 513
    if kind == "negdup":
        assert (neg[:, 0] == neg[:, 1]).all() and (neg[0] == neg[0, 0]).all()
    if kind == "negtgt":
        assert np.isin(neg[:, 0], tg).all() and neg[5, 2] == tg[5]
    ref = R.reference(name)
    named = np.zeros(R.NUM_ITEM, bool)
    named[seq[seq >= 0]] = True
    cls = np.zeros(R.NUM_ITEM, bool)
    cls[tg] = True
    cls[neg.ravel()] = True
    A, g = ref["A"], ref["g"]
    assert (A["rerank_emb"][~named] == 0).all() and (g["rerank_emb"][~named] == 0).all() and (A["rerank_emb"][named] > 0).all()
    assert (A["softmax_w"][~cls] == 0).all() and (g["softmax_w"][~cls] == 0).all() and (A["softmax_w"][cls] > 0).all()
    assert ((A["softmax_b"] > 0) == cls).all() and (A["rerank_b"] > 0).all()
    assert np.isfinite(ref["loss"]) and ref["loss"] > 0 and ref["A_loss"] >= ref["loss"]


def test_cases_cover_what_the_kernels_branch_on():
    sh = R.SHAPES.values()
    assert {s[0] for s in sh} >= {16, 48, 64, 128} and {s[1] for s in sh} >= {1, 10, 13}
    assert {s[2] for s in sh} >= {1, 63, 64, 65, 511, 512, 513, 1025} and {s[3] for s in sh} >= {1, 4, 63, 64, 255}
    assert {s[4] for s in sh} >= {"allpad", "rephist", "same", "negdup", "negtgt"}


def test_row_order_does_not_change_the_answer():
    c = R.make_case("b512-allpad-f64")
    a = R.reference("b512-allpad-f64")
    b = R.step(c["weights"], c["dims"], c["seq"], c["targets"], c["negatives"], reverse=True)
    for k in R.TENSORS:
        np.testing.assert_allclose(a["g"][k], b["g"][k], rtol=0, atol=1e-14)
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-14)


def test_tolerance_file_matches_its_script():
    """the committed constants are what the script gives for a sample of cheap cases, and 8 x the largest ratio"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dr_rerank_tolerances", os.path.join(GOLDEN, "make_dr_rerank_tolerances.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    tol = json.load(open(os.path.join(GOLDEN, "dr_rerank_tolerances.json")))
    assert tol["margin"] == 8.0
    for dt in ("f32", "f64"):
        assert sorted(tol[dt]["cases"]) == sorted(n for n in R.CASES if n.endswith(dt))
        for t in R.TENSORS + ("loss",):
            assert tol[dt]["k"][t] == pytest.approx(8.0 * max(c[t] for c in tol[dt]["cases"].values()), rel=1e-12)
            assert tol[dt]["k"][t] > 0
        assert tol[dt]["k"]["full_loss"] == pytest.approx(8.0 * max(tol[dt]["full_loss_cases"].values()), rel=1e-12) and tol[dt]["k"]["full_loss"] > 0
    for name in ("tiny-f32", "b63-f64", "b64-f32"):
        got = mk.measure(name)
        for t, v in got.items():
            assert v == pytest.approx(tol[name[-3:]]["cases"][name][t], rel=1e-6, abs=1e-12), (name, t)


def test_learning_case_reaches_its_threshold_in_the_restatement():
    p = R.learning_problem()
    E, L, NI = p["dims"]
    assert (p["targets"] == (p["seqs"][:, -1] + 1) % NI).all()
    tg = tuple(int(x) for x in p["targets"])
    batches = [(p["seqs"], p["targets"], R.sample(p["sampler_seed"], t, tg, p["S"], NI)[0]) for t in range(p["steps"])]
    for accumulate in (True, False):
        w, losses = R.train(p["weights"], p["dims"], batches, p["lr"], accumulate=accumulate)
        assert losses[-1] < p["fraction"] * losses[0], losses[[0, -1]]
        assert R.full_loss(w, p["dims"], p["seqs"], p["targets"])[0] < p["fraction"] * R.full_loss(p["weights"], p["dims"], p["seqs"], p["targets"])[0]


def test_header_declares_the_rerank_training_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    from dismember_amd import _native as N
    for fn in ("dm_dr_rerank_train_init", "dm_dr_rerank_train_free", "dm_dr_rerank_forward_backward", "dm_dr_rerank_forward_backward_dev",
               "dm_dr_rerank_sample", "dm_dr_rerank_adam_step", "dm_dr_rerank_download", "dm_dr_rerank_full_loss"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in N.SIGNATURES
