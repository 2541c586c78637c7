"""GPU tests of the Deep-Retrieval beam search at the logit ranges its data-dependent paths exist for (cases and labels:
tests/dr_search_cases.py; their CPU checks: tests/test_dr_search_cases_host.py), on both routes, with the counters that say which path ran.

  * fp64 cases: paths and counts BIT-EXACT against the fp64 oracle for every user, probabilities within rtol 1e-9, rows past the count
    -1 / 0 — the contract of test_gpu_dr.py, here where the sliced route's bound Mhat sits hundreds of units above the logits.
  * f32 cases: full lists, non-increasing, distinct; EVERY returned path's probability within the case's tolerance of
    tests/golden/dr_search_tolerances.json (measured on the CPU) of the fp64 probability of that path; kept mass within the same;
    lists identical to the oracle's for >= 90 % of the users.
  * counters (Engine.dr_search_counters): cases labelled fast never leave the fast cut; user-layers labelled must_exact are counted
    on the exact path; no user-layer is counted twice.

Each (case, route) is searched once on the device; the tests share that run and the oracle's lists.
"""
import json
import os

import numpy as np
import pytest

import dr_search_cases as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROUTES = ["one_kernel", "sliced"]
_runs, _refs = {}, {}


def run(name, route):
    """Paths, probabilities, counts and counters of one search of the case on the route.  DM_DR_SLICED_MIN_USERS=1 forces the column-sliced
    pipeline onto these small batches, DM_DR_SLICED=0 forces the one-workgroup-per-user kernel; both are read at model load."""
    if (name, route) not in _runs:
        from dismember_amd import Engine
        c = R.build(name)
        key, val = ("DM_DR_SLICED_MIN_USERS", "1") if route == "sliced" else ("DM_DR_SLICED", "0")
        os.environ[key] = val
        try:
            eng = Engine(0)
            eng.dr_load_model(c["w"], c["E"], c["L"], c["K"], c["D"], c["num_item"], dtype=R.NP_T[c["dtype"]])
            eng.dr_search_counters(reset=True)
            paths, probs, cnt = eng.dr_beam_search(c["seqs"], c["beam"])
            exact, wave, reasons = eng.dr_search_counters(reset=True)
            eng.close()
        finally:
            os.environ.pop(key, None)
        _runs[(name, route)] = dict(paths=paths, probs=probs, cnt=cnt, exact=exact, wave=wave, reasons=reasons)
    return _runs[(name, route)]


def ref(name, oracle):
    """The fp64 oracle's lists, once per case."""
    if name not in _refs:
        c = R.build(name)
        orc = oracle.DeepRetrieval(c["w"], c["E"], c["L"], c["K"], c["D"], c["num_item"])
        _refs[name] = [orc.beam_search(c["seqs"][u], c["beam"]) for u in range(c["U"])]
    return _refs[name]


def layer0_exact(c):
    """(least, most) exact layers the one-kernel route counts at LAYER 0, which shares the counter.  Layer 0 has one path, so ceil(K / 16)
    non-empty blocks of 16 columns.  With fewer than the kb = min(beam, 64) block maxima its bound needs, the bound is -inf and every
    user takes the exact select BY CONSTRUCTION (K = 100, beam = 20: 7 blocks).  With exactly kb blocks (K = 1024, beam = 64) the radix
    select may stop after its first 11-bit digit — all 64 keys in one bin, all wanted — and the bound is then the bottom of a binade:
    more survivors than the list holds, exact select again, but by the data (measured: 8 of 8 users).  More blocks than kb: none.
    The sliced route's layer 0 is a one-wave kernel without that bound; it counts only the users it hands to the block kernel."""
    nblk, kb = -(-c["K"] // 16), min(c["beam"], 64)
    return (c["U"], c["U"]) if nblk < kb else ((0, c["U"]) if nblk == kb else (0, 0))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["dtype"] == "f64"])
def test_f64_lists_are_the_oracles(name, route, oracle):
    c, r, o = R.build(name), run(name, route), ref(name, oracle)
    bad = [u for u in range(c["U"]) if r["cnt"][u] != len(o[u][0]) or r["paths"][u, :r["cnt"][u]].tolist() != o[u][0].tolist()]
    print(name, route, "users with other paths:", bad, "counters:", r["exact"], r["wave"], r["reasons"])
    assert not bad, bad
    for u in range(c["U"]):
        n = r["cnt"][u]
        np.testing.assert_allclose(r["probs"][u, :n], o[u][1], rtol=1e-9, atol=0)
        assert (r["paths"][u, n:] == -1).all() and (r["probs"][u, n:] == 0).all()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["dtype"] == "f32"])
def test_f32_lists_against_the_oracle(name, route, oracle):
    c, r, o = R.build(name), run(name, route), ref(name, oracle)
    rtol = json.load(open(os.path.join(GOLDEN, "dr_search_tolerances.json")))["cases"][name]["rtol"]
    U, beam = c["U"], c["beam"]
    worst, worst_mass, same = 0.0, 0.0, 0
    want = [R.path_probs(name, u, np.clip(r["paths"][u], 0, c["K"] - 1), np.float64) for u in range(U)]
    for u in range(U):
        worst = max(worst, float((np.abs(r["probs"][u] - want[u]) / want[u]).max()))
        worst_mass = max(worst_mass, abs(r["probs"][u].sum() - o[u][1].sum()) / o[u][1].sum())
        same += int(r["paths"][u].tolist() == o[u][0].tolist())
    print(name, route, "worst rel. error %.3e, of the kept mass %.3e (rtol %.3e), same lists %d / %d, counters:" % (worst, worst_mass, rtol, same, U),
          r["exact"], r["wave"], r["reasons"])
    for u in range(U):
        assert r["cnt"][u] == beam
        assert (np.diff(r["probs"][u]) <= 0).all(), u
        assert len({tuple(p) for p in r["paths"][u]}) == beam, u
        assert (np.abs(r["probs"][u] - want[u]) <= rtol * want[u]).all(), u          # every path, not a sample of ranks
        assert abs(r["probs"][u].sum() - o[u][1].sum()) <= rtol * o[u][1].sum(), u
    assert same >= 0.9 * U, same


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["group"] == "ties"])
def test_ties_keep_the_stable_order(name, route):
    """Every logit is 0: layer 0 keeps nodes 0 .. min(beam, K) - 1, layer 1 the first `beam` of (0, 0 ..), and so on: lexicographic
    prefixes for every user, in both precisions (test_gpu_dr.py::test_ties_are_stable)."""
    c, r = R.build(name), run(name, route)
    K, beam = c["K"], c["beam"]
    l0 = list(range(min(beam, K)))
    l1 = [(a, b) for a in l0 for b in range(K)][:beam]
    exp = [list(t) for t in [(a, b, k) for (a, b) in l1 for k in range(K)][:beam]]
    for u in range(c["U"]):
        assert r["cnt"][u] == beam and r["paths"][u].tolist() == exp, u
        np.testing.assert_allclose(r["probs"][u], 1.0 / K ** 3, rtol=1e-6)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_counters_say_which_path_ran(name, route):
    c, r = R.build(name), run(name, route)
    lc = R.label_counts(name)
    layers = c["U"] * (c["D"] - 1)
    exact, wave, reasons = r["exact"], r["wave"], r["reasons"]
    print(name, route, "labels", lc, "exact_layers", exact, "wave_fallbacks", wave, "reasons", reasons)
    assert sum(reasons) == wave and reasons[0] == 0 and reasons[7] == 0
    # a user-layer takes the exact path at most once: the D - 1 layers with tables, and layer 0 (counted by the same counter)
    assert exact <= layers + c["U"] and wave <= layers
    if route == "one_kernel":
        assert wave == 0
    if c["group"] in ("control", "edges"):
        lo, hi = layer0_exact(c) if route == "one_kernel" else (0, 0)         # no layer d >= 1 leaves the fast cut on either route
        assert lo <= exact <= hi
        assert wave == 0
    elif c["group"] == "wide":
        if route == "sliced":
            assert wave >= lc["must_exact"] and exact >= lc["must_exact"]
            assert reasons[1] >= lc["must_exact"]        # every product of a path is zero: the sum is zero
            assert reasons[6] >= 1                       # and, short of that, products in the underflow range (the cut model: dozens)
    else:
        assert exact >= lc["must_exact"] == layers


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_identical_users_get_identical_results(name, route):
    c, r = R.build(name), run(name, route)
    assert np.array_equal(c["seqs"][1], c["seqs"][2])
    assert np.array_equal(r["paths"][1], r["paths"][2]) and np.array_equal(r["probs"][1], r["probs"][2])
