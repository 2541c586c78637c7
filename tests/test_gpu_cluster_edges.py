"""TDMClusterTree on the device, the edges test_gpu_cluster.py (G1-G7) leaves open: Lloyd on segments of several tiles at every
native embed size against the fp64 restatement (G8), the seeds and the winning restart predicted from the restated counter RNG
(G9), degenerate inputs with exact known answers (G10), embed sizes the library pads (G11), non-finite rows refused (G12).
The conditions these tests put on their inputs are proved on the CPU in test_cluster_host.py; tolerances are in
tests/golden/cluster_tolerances.json.  With CUT = 256 (the LDS cut-off) and TILE = 1024, n = 2500 gives streamed levels of
3 tiles (1024, 1024, 452), 2 tiles (1024, 226), 1 tile (625) and 1 tile (312 / 313); level 4 and below run inside the LDS."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cluster_ref as R
from dismember_amd import Engine, _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = json.load(open(os.path.join(ROOT, "tests", "golden", "cluster_tolerances.json")))
N8, DATA_SEED, G8_SEED, G9_SHAPES, G9_WINNER_SEEDS = R.N8, R.DATA_SEED, R.G8_SEED, R.G9_SHAPES, R.G9_WINNER_SEEDS


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("E", [16, 32, 64, 128])
def test_g8_multi_tile_lloyd_matches_restatement(eng, E):
    """Every streamed node (levels 0-3: 3, 2, 1, 1 tiles per segment), every LDS node of level 4 and eight nodes per deeper level:
    the restatement run from the traced seeds on the node's members gives the traced centroid 0, distortion and iteration count.
    A node is compared when no item ever came within 64 E 2^-24 (relative) of the bisecting boundary; none of the 15 streamed
    nodes may miss that, and at most a tenth of the others.  The data (R.hierarchy) is scaled so that the distortion tolerance is
    under a hundredth of the distortion at every compared node, and some streamed and some LDS node takes three iterations or more
    (tests/test_cluster_host.py asserts both on the predicted tree), so all three checks bind."""
    x = R.g8_data(E)
    codes, st, tr = eng.cluster_tree(x, restarts=4, seed=G8_SEED, trace=True)
    R.check_structure(codes, N8)
    assert st["levels_streamed"] == 4
    bound = TOL["centroid_multi_tile"]["hierarchy_2500x%d" % E]["bound_abs"]
    worst_c, worst_d, streamed, lds, skipped, long_runs = 0.0, 0.0, 0, 0, 0, [0, 0]
    for code, level, items in R.nodes(N8, tr["perm"]):
        if len(items) < 3 or code - ((1 << level) - 1) not in R.sampled_indices(level):
            continue
        items = np.sort(items)                                   # membership only; the restatement runs from the traced seeds
        s0, s1 = (int(np.flatnonzero(items == s)[0]) for s in tr["seeds"][code])
        c0, c1, a, D, it, mg = R.lloyd(x[items], s0, s1, margin=True)
        if mg < R.margin_floor(E):
            assert level > 3, (code, level, mg, "a streamed node is too close to a boundary to be compared")
            skipped += 1
            lds += 1
            continue
        streamed, lds = streamed + (level <= 3), lds + (level > 3)
        assert R.distortion_tol(E, D) <= 0.01 * D, (code, level, D)
        long_runs[level > 3] += int(tr["iters"][code]) >= 3
        err = float(np.abs(c0 - tr["centroid0"][code]).max())
        derr = abs(D - tr["distortion"][code])
        worst_c, worst_d = max(worst_c, err), max(worst_d, derr / R.distortion_tol(E, D))
        assert err <= bound, (code, level, len(items), err, bound)
        assert derr <= R.distortion_tol(E, D), (code, level, D, tr["distortion"][code])
        assert abs(int(tr["iters"][code]) - it) <= 1, (code, level, tr["iters"][code], it)
    print("G8 E=%d: %d streamed + %d LDS nodes (%d skipped), worst |centroid0 - restatement| %.3g (bound %.3g), worst distortion "
          "error / its tolerance %.3g" % (E, streamed, lds, skipped, worst_c, bound, worst_d))
    assert streamed == 15 and lds >= 16 + 8 * 4 and skipped <= 0.1 * lds and min(long_runs) >= 1, long_runs


@pytest.mark.parametrize("n,E", G9_SHAPES)
def test_g9_seeds_are_the_predicted_draws(eng, n, E):
    """restarts = 1 at node 0 (perm is the identity): the first seed is cl_first_seed(seed, 0, 0, n) and the second the D^2-weighted
    pick, both predicted from the restated RNG (R.predict_seeds).  n = 200 is one walk inside the LDS kernel; 300 and 1500 are
    streamed (chunks of 2 and of 6 positions; 1500 is two tiles).  The oracle library does not export its draw (orc_draw is
    static), so this test is also the pin of the restated dm_sample_draw against the device."""
    x = R.g8_data(E)[:n]
    single = 0
    for seed in range(1, 33):
        _, _, tr = eng.cluster_tree(x, restarts=1, seed=seed, trace=True)
        s0, cand = R.predict_seeds(x, seed, 0, 0)
        assert int(tr["seeds"][0][0]) == s0, (seed, tr["seeds"][0], s0)
        assert int(tr["seeds"][0][1]) in cand, (seed, tr["seeds"][0], cand)
        single += len(cand) == 1
    print("G9 %dx%d: 32 seeds, %d with a single second-seed candidate" % (n, E, single))
    assert single >= 30


@pytest.mark.parametrize("n,E", G9_SHAPES)
def test_g9_lowest_distortion_restart_wins(eng, n, E):
    """restarts = 32 (the high half of the assignment mask and of the per-group restart loop): all 32 seed pairs predicted, each run
    through the restatement; the traced seeds and distortion are the predicted winner's.  For every seed, eight restarts are no
    worse than one (restart 0 of both runs is the same stream)."""
    x = R.blobs(n, E, 3)
    worst = 0.0
    for seed in G9_WINNER_SEEDS[(n, E)]:
        r, (s0, s1), D, _, _ = R.predict_winner(x, seed, 0, 32)
        _, _, tr = eng.cluster_tree(x, restarts=32, seed=seed, trace=True)
        assert (int(tr["seeds"][0][0]), int(tr["seeds"][0][1])) == (s0, s1), (seed, r, tr["seeds"][0], (s0, s1))
        derr = abs(tr["distortion"][0] - D)
        worst = max(worst, derr / R.distortion_tol(E, D))
        assert derr <= R.distortion_tol(E, D), (seed, r, D, tr["distortion"][0])
        _, _, t1 = eng.cluster_tree(x, restarts=1, seed=seed, trace=True)
        _, _, t8 = eng.cluster_tree(x, restarts=8, seed=seed, trace=True)
        assert t8["distortion"][0] <= t1["distortion"][0], (seed, t8["distortion"][0], t1["distortion"][0])
    print("G9 %dx%d, 32 restarts: worst distortion error / its tolerance %.3g" % (n, E, worst))


@pytest.mark.parametrize("E", [16, 128])
@pytest.mark.parametrize("n", [3, 257, 2500, 9000])
def test_g10_identical_rows(eng, n, E):
    """every sort key equal: each split keeps the parent's order (across the radix sort's tiles — n = 9 000 is three tiles of 4 096 —
    and in the LDS rank), so the tree is the balanced recursion over the identity order; the mean of copies is the row, the
    distortion 0, one iteration"""
    row = np.random.default_rng(E).standard_normal(E).astype(np.float32)
    row[0], row[1] = -1.5, 0.0
    x = np.tile(row, (n, 1))
    codes, _, tr = eng.cluster_tree(x, restarts=3, seed=4, trace=True)
    assert np.array_equal(tr["perm"], np.arange(n))
    assert np.array_equal(codes, R.balanced_codes(n))
    for code, size in R.expected_node_sizes(n).items():
        if size >= 3:
            assert np.array_equal(tr["centroid0"][code].view(np.uint32), row.view(np.uint32)), code
            assert tr["distortion"][code] == 0.0 and tr["iters"][code] == 1, (code, tr["distortion"][code], tr["iters"][code])


@pytest.mark.parametrize("E", [16, 128])
def test_g10_two_values(eng, E):
    """1 700 copies of a and 800 of b, interleaved 17 : 8 in every 25 rows.  Sums of fewer than 2^12 copies of a float32 are exact in
    fp64 and so are their quotients, so centroid 0 of every node is, bit for bit, the row traced as its first seed; a mixed node
    orders its items stably by "differs from that value", a pure one keeps its order: an exact known answer for the whole tree."""
    rng = np.random.default_rng(100 + E)
    a, b = rng.standard_normal((2, E)).astype(np.float32)
    is_b = (np.arange(N8) * 8) % 25 < 8
    assert is_b.sum() == 800
    x = np.where(is_b[:, None], b, a).astype(np.float32)
    codes, _, tr = eng.cluster_tree(x, restarts=3, seed=6, trace=True)
    R.check_structure(codes, N8)
    want = np.zeros(N8, np.int64)
    stack, fitted = [(0, np.arange(N8))], 0
    while stack:
        code, items = stack.pop()
        if len(items) == 1:
            want[items[0]] = code
            continue
        if len(items) >= 3:
            first = x[tr["seeds"][code][0]]
            assert np.array_equal(tr["centroid0"][code].view(np.uint32), first.view(np.uint32)), code
            items = items[np.argsort((x[items] != first).any(axis=1), kind="stable")]
            fitted += 1
        h = len(items) // 2
        stack += [(2 * code + 1, items[:h]), (2 * code + 2, items[h:])]
    assert fitted > 1000 and np.array_equal(codes, want)


def test_g10_one_iteration(eng):
    x = R.g8_data(16)
    codes, _, tr = eng.cluster_tree(x, restarts=4, max_iter=1, seed=G8_SEED, trace=True)
    R.check_structure(codes, N8)
    for code, size in R.expected_node_sizes(N8).items():
        if size >= 3:
            assert tr["iters"][code] == 1, (code, size, tr["iters"][code])
    assert R.check_split_rule(x, tr, TOL["distance_edges"]["hierarchy_2500x16"]["bound_rel"], "G10 max_iter = 1") > 1000


@pytest.mark.parametrize("E", [1, 24, 48, 100])
def test_g11_padded_embed_sizes(eng, E):
    """an embed size the library pads to the next native one: the structure, the split rule, a traced centroid of E columns, and,
    exactly, the tree of the same rows zero-padded by the caller (a padding column adds fmaf(0, 0, d) = d)"""
    n = 600
    x = np.random.default_rng(40 + E).random((n, E), dtype=np.float32)
    codes, st, tr = eng.cluster_tree(x, restarts=4, seed=8, trace=True)
    R.check_structure(codes, n)
    assert st["levels_streamed"] == 2 and tr["centroid0"].shape == (1023, E)
    assert R.check_split_rule(x, tr, TOL["distance_edges"]["uniform_600x%d" % E]["bound_rel"], "G11 E = %d" % E) > 100
    EP = next(v for v in (16, 32, 64, 128) if v >= E)
    xp = np.zeros((n, EP), np.float32)
    xp[:, :E] = x
    codes_p, _, tr_p = eng.cluster_tree(xp, restarts=4, seed=8, trace=True)
    assert np.array_equal(codes, codes_p) and np.array_equal(tr["perm"], tr_p["perm"])
    fitted = ~np.isnan(tr["centroid0"][:, 0])
    assert np.array_equal(tr["centroid0"].view(np.uint32), tr_p["centroid0"][:, :E].view(np.uint32)) and not tr_p["centroid0"][fitted, E:].any()


@pytest.mark.parametrize("n,row", [(600, 17), (2500, 1300), (2500, 2499)])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_g12_non_finite_row_is_refused(eng, n, row, bad):
    """one NaN or +Inf anywhere (n = 600: two streamed levels, then the LDS; n = 2500: the multi-tile path, row 2499 being the last
    row of the ragged third tile) is refused before any clustering kernel runs, the message names the row, the handle stays usable"""
    L = N.lib()
    x = R.g8_data(16)[:n]
    poisoned = x.copy()
    poisoned[row, 5] = bad
    codes = np.zeros(n, np.int32)
    rc = L.dm_cluster_tree(eng._h, poisoned.ctypes.data_as(N.f32p), n, 16, 3, 100, 1e-4, 1, codes.ctypes.data_as(N.i32p), None, None)
    assert rc == -1 and b"dm_cluster_tree: row %d " % row in L.dm_last_error(eng._h), L.dm_last_error(eng._h)
    good, _, _ = eng.cluster_tree(x, restarts=3, seed=1)
    R.check_structure(good, n)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_g12_non_finite_table_row_is_refused(bad):
    from helpers import random_din_weights, synthetic_tree
    rng = np.random.default_rng(12)
    t = synthetic_tree(rng, 10, 600)
    w = random_din_weights(rng, 16, 2047)
    e = Engine(0)
    e.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    e.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    ids, k = t["leaf_ids"], 417
    poisoned = w.copy()
    poisoned[int(t["leaf_codes"][k]) * 16 + 9] = bad
    e.load_weights_din(poisoned, 16, 2047)
    L = N.lib()
    codes = np.zeros(600, np.int32)
    rc = L.dm_cluster_tree_model(e._h, ids.ctypes.data_as(N.i32p), 600, 3, 100, 1e-4, 1, codes.ctypes.data_as(N.i32p), None, None)
    msg = L.dm_last_error(e._h)
    assert rc == -1 and b"dm_cluster_tree_model: row %d (item id %d)" % (k, ids[k]) in msg, msg
    e.load_weights_din(w, 16, 2047)
    good, _, _ = e.cluster_tree(item_ids=ids, restarts=3, seed=1)
    R.check_structure(good, 600)
    e.close()
