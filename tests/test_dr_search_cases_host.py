"""CPU checks of tests/dr_search_cases.py: the cases sit in the regimes they are named for, the numpy restatement is the fp64 oracle's
search, the committed f32 tolerances are what tests/golden/make_dr_search_tolerances.py measures, and the model of the sliced route's
tabulated-product cut loses winners on the wide cases with the rule of the parent kernels and none with the guarded rule of
dr_sliced.hip.inc (DrsTol::pmax_min, prod_min) — the CPU check of those constants."""
import importlib.util
import json
import os

import numpy as np
import pytest

import dr_search_cases as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
WIDE = [n for n, c in R.CASES.items() if c["group"] == "wide"]
F64 = [n for n, c in R.CASES.items() if c["dtype"] == "f64"]
F32 = [n for n, c in R.CASES.items() if c["dtype"] == "f32"]


def test_case_table():
    groups = {}
    for n, c in R.CASES.items():
        groups.setdefault(c["group"], []).append((c["K"], c["D"], c["L"], c["E"], c["beam"], c["U"], c["scale"], c["dtype"]))
        assert c["num_item"] == 500
    assert sorted(groups["control"]) == [(100, 3, 4, 16, 20, 48, 0.3, "f32"), (100, 3, 4, 16, 20, 48, 0.3, "f64")]
    assert sorted(groups["wide"]) == [(100, 3, 4, 16, 20, 48, 2.0, "f32"), (100, 3, 4, 16, 20, 48, 2.25, "f32"),
                                      (100, 3, 4, 16, 20, 48, 6.0, "f64"), (100, 3, 4, 16, 20, 48, 7.0, "f64")]
    assert sorted(g[:5] + g[7:] for g in groups["ties"]) == [(70, 3, 3, 16, 7, "f32"), (70, 3, 3, 16, 7, "f64"), (70, 3, 3, 16, 64, "f32"),
                                                             (70, 3, 3, 16, 64, "f64")]
    assert sorted(g[:2] + g[4:] for g in groups["edges"]) == [(129, 3, 64, 8, 0.3, "f64"), (1001, 4, 64, 8, 0.3, "f64"), (1024, 2, 64, 8, 0.3, "f64")]


@pytest.mark.parametrize("name", list(R.CASES))
def test_numpy_search_is_the_oracle_search(name, oracle):
    """The float64 restatement the labels and tolerances rest on returns the fp64 oracle's paths, and its probabilities to 1e-12."""
    c = R.build(name)
    orc = oracle.DeepRetrieval(c["w"], c["E"], c["L"], c["K"], c["D"], c["num_item"])
    paths, probs, cnt, _ = R.beam64(name)
    for u in range(c["U"]):
        op, ov = orc.beam_search(c["seqs"][u], c["beam"])
        assert cnt[u] == len(op) and paths[u, :cnt[u]].tolist() == op.tolist(), u
        np.testing.assert_allclose(probs[u, :cnt[u]], ov, rtol=1e-12, atol=0)
    assert np.array_equal(c["seqs"][1], c["seqs"][2]) and (c["seqs"][0] == -1).all()


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["group"] in ("control", "edges")])
def test_control_and_edges_are_fast(name):
    lc = R.label_counts(name)
    c = R.CASES[name]
    assert lc == {"fast": c["U"] * (c["D"] - 1), "must_exact": 0, "open": 0}


@pytest.mark.parametrize("name", WIDE)
def test_wide_cases_reach_the_fallback_regimes(name):
    lc = R.label_counts(name)
    assert lc["must_exact"] >= 5 and lc["open"] >= 20, lc
    c = R.build(name)
    _, probs, cnt, _ = R.beam64(name)
    assert (cnt == c["beam"]).all()
    assert probs.min() >= (1e-30 if c["dtype"] == "f32" else 1e-280)          # no result is subnormal in the device's type


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["group"] == "ties"])
def test_ties_must_take_the_exact_path(name):
    c = R.CASES[name]
    recs = R.classify(name)
    assert len(recs) == c["U"] * (c["D"] - 1)
    for r in recs:
        n_cand = len(r["gaps"]) * c["K"]
        assert r["ties"] == n_cand
        if n_cand > R.nl_of(c["beam"]):
            assert r["label"] == "must_exact"
    assert all(len(r["gaps"]) * c["K"] > R.nl_of(c["beam"]) for r in recs)       # at these beams that is every layer d >= 1


@pytest.mark.parametrize("name", [n for n in F64 if R.CASES[n]["group"] != "ties"])
def test_f64_lists_have_no_near_ties(name):
    """Bit-exact path lists are a fair demand: no two consecutive probabilities of a user's fp64 list within 1e-6 relative."""
    _, probs, cnt, _ = R.beam64(name)
    for u in range(len(cnt)):
        v = probs[u, :cnt[u]]
        assert (v[:-1] - v[1:] > 1e-6 * v[1:]).all(), u


def _script():
    spec = importlib.util.spec_from_file_location("make_dr_search_tolerances", os.path.join(GOLDEN, "make_dr_search_tolerances.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", F32)
def test_committed_f32_tolerances_are_the_measured_ones(name):
    tol = json.load(open(os.path.join(GOLDEN, "dr_search_tolerances.json")))
    mod = _script()
    assert tol["margin"] == mod.MARGIN == 4.0 and sorted(tol["cases"]) == sorted(F32)
    got, want = mod.measure(name), tol["cases"][name]
    assert abs(got["err"] - want["err"]) <= 0.01 * want["err"] and got["same"] == want["same"]
    assert want["rtol"] == 4.0 * max(want["err"], R.CASES[name]["D"] * 2.0 ** -24)
    if name in WIDE:
        assert want["same"] >= 0.95          # the f32 restatement as a whole search against the fp64 lists; the device test asks 0.9
        assert 1e-5 < want["rtol"] < 2e-3    # |logit| ~ 100 at 2^-24: above test_beam_search_f32's regime, far below a wrong probability


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("name", WIDE)
def test_cut_model_parent_rule_loses_winners_guarded_rule_none(name, flush):
    par = R.sliced_cut_model(name, flush, "parent")
    assert par["layers"] == 96 and par["missed"] > 0 and par["miss_layers"] > 0 and par["worst"] > 1.0, par
    new = R.sliced_cut_model(name, flush, "guarded")
    assert new["missed"] == 0 and new["damaged_kept"] == 0, new
    must = R.label_counts(name)["must_exact"]
    assert new["exact"] >= must and new["exact"] >= par["exact"]


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["group"] in ("control", "edges")])
def test_cut_model_keeps_the_fast_cases_on_the_product_cut(name, flush):
    """Nothing changes for inputs labelled fast: no user-layer leaves the tabulated-product cut under either rule."""
    for rule in ("parent", "guarded"):
        m = R.sliced_cut_model(name, flush, rule)
        assert m["exact"] == 0 and m["missed"] == 0 and m["damaged_kept"] == 0 and m["s_zero"] == 0, (rule, m)
