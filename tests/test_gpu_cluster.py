"""TDMClusterTree on the device (dismember_amd/csrc/cluster.hip.inc) through the C ABI: structure (G1), the split rule on the
device's own numbers (G2), Lloyd against the numpy restatement (G3), a planted tree (G4), the table path (G5), config 1 end to
end (G6), argument errors (G7).  The reference is unseeded, so there is no reference-produced tree; parity is structural and
numerical.  Tolerances: tests/golden/cluster_tolerances.json (how they were derived is written there)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cluster_ref as R
from dismember_amd import Engine, _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = json.load(open(os.path.join(GOLDEN, "cluster_tolerances.json")))
DEPTH, E_PL, SIGMA, PL_SEED = 10, 16, 1e-4, 7          # the planted data of G2 / G3 (the CPU test file checks its properties)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _uniform(n, E, seed=11):
    return np.random.default_rng(seed).random((n, E), dtype=np.float32)


@pytest.mark.parametrize("E", [16, 128])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 5000, 100003])
def test_g1_structure(eng, n, E):
    x = _uniform(n, E)
    codes, st, _ = eng.cluster_tree(x, restarts=3, seed=5)
    R.check_structure(codes, n)
    again, _, _ = eng.cluster_tree(x, restarts=3, seed=5)
    assert np.array_equal(codes, again), "two runs with one seed differ"
    other, _, _ = eng.cluster_tree(x, restarts=3, seed=6)
    R.check_structure(other, n)
    if n > 256:
        assert st["levels_streamed"] >= 1 and st["lloyd_passes"] >= st["levels_streamed"]
    else:
        assert st["levels_streamed"] == 0


_nodes, _check_split_rule = R.nodes, R.check_split_rule      # (shared with test_gpu_cluster_edges.py)


@pytest.mark.parametrize("case", ["planted_1024x16", "uniform_5000x16", "uniform_1000x128"])
def test_g2_split_rule_on_device_numbers(eng, case):
    if case == "planted_1024x16":
        x, _ = R.planted(DEPTH, E_PL, SIGMA, PL_SEED)
    elif case == "uniform_5000x16":
        x = _uniform(5000, 16, 21)
    else:
        x = _uniform(1000, 128, 22)
    codes, _, tr = eng.cluster_tree(x, restarts=4, seed=3, trace=True)
    R.check_structure(codes, len(x))
    # the final order and the codes agree: position p of the last level holds the row with the p-th smallest flattened code
    flat = R.flatten_leaves(codes, 2 ** tr["max_level"] - 1)
    assert np.array_equal(np.argsort(flat, kind="stable"), tr["perm"])
    assert _check_split_rule(x, tr, TOL["distance"][case]["bound_rel"]) > 0


def test_g3_lloyd_matches_restatement(eng):
    x, _ = R.planted(DEPTH, E_PL, SIGMA, PL_SEED)
    codes, _, tr = eng.cluster_tree(x, restarts=10, seed=9, trace=True)
    bound = TOL["centroid"]["bound_abs"]
    rng = np.random.default_rng(0)
    worst, seen = 0.0, {}
    for code, level, items in _nodes(len(x), tr["perm"]):
        if len(items) < 3 or (level > 0 and seen.get(level, 0) >= 8 and rng.random() > 0.1):
            continue
        seen[level] = seen.get(level, 0) + 1
        items = np.sort(items)                                   # membership only; the restatement runs from the traced seeds
        s0, s1 = (int(np.flatnonzero(items == s)[0]) for s in tr["seeds"][code])
        c0, c1, a, D, it = R.lloyd(x[items], s0, s1)
        err = float(np.abs(c0 - tr["centroid0"][code]).max())
        worst = max(worst, err)
        assert err <= bound, (code, level, err)
        # distortion: the device sums float32 distances of E sequential terms (relative error <= E * 2^-24 each, twice that allowed),
        # and the two may stop one iteration apart where |D_{t-1} - D_t| straddles the tolerance (<= tol = 1e-4 of difference)
        assert abs(D - tr["distortion"][code]) <= 1e-4 + 2 * E_PL * 2.0 ** -24 * D, (code, D, tr["distortion"][code])
        # fixed point: (device centroid 0, the restatement's centroid 1) reassigned and averaged moves by less than the tolerance
        dev0 = tr["centroid0"][code].astype(np.float64)
        a2 = R.sqdist(x[items], c1) < R.sqdist(x[items], dev0)
        assert (~a2).any() and np.sqrt(((x[items][~a2].astype(np.float64).mean(axis=0) - dev0) ** 2).sum()) < 1e-4
    print("G3: nodes per level %s, worst |centroid0 - restatement| %.3g (bound %.3g)" % (seen, worst, bound))
    assert sorted(seen) == list(range(0, DEPTH - 1))             # every level that has nodes of three items or more


@pytest.mark.parametrize("sigma", [0.0, 1e-4, 1e-3])
def test_g4_planted_tree_is_found(eng, sigma):
    x, leaf = R.planted(DEPTH, E_PL, sigma, PL_SEED)
    codes, _, _ = eng.cluster_tree(x, restarts=10, seed=1)
    rec = [R.recovery(codes, leaf, DEPTH, l) for l in range(1, DEPTH + 1)]
    print("G4 sigma %g: recovery per level %s" % (sigma, rec))
    assert rec[:6] == [1.0] * 6


def _fixture_model(eng):
    t = np.load(os.path.join(GOLDEN, "tdm_tree.npz"))
    w = np.load(os.path.join(GOLDEN, "din_f32.npy"))
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_din(w, 16, 8191)
    return t, w


def test_g5_table_path():
    e = Engine(0)
    t, w = _fixture_model(e)
    order = np.argsort(t["leaf_ids"])
    ids, lcodes = t["leaf_ids"][order], t["leaf_codes"][order]
    emb = e.leaf_embeddings(ids)
    assert emb.shape == (3706, 16)
    assert np.array_equal(emb.view(np.uint32), w[:8191 * 16].reshape(8191, 16)[lcodes].view(np.uint32))
    a, _, _ = e.cluster_tree(item_ids=ids, restarts=5, seed=4)
    b, _, _ = e.cluster_tree(embeddings=emb, restarts=5, seed=4)
    R.check_structure(a, 3706)
    assert np.array_equal(a, b)
    e.close()


def test_g6_config1_end_to_end(tmp_path):
    from test_tasks import _conf
    from dismember_amd import tasks, tree_io
    conf = _conf(tmp_path, **{"model.iteration_number": 20, "model.show_progress_interval": 0})
    tasks.tdm_initialize_tree(conf)
    r = tasks.tdm_train_deep_model(conf, time_recommend=False)
    r["engine"].close()
    embed = r["params"]["embed_path"]
    assert sum(1 for _ in open(embed)) == 3325
    c = tasks.tdm_cluster_tree(conf)
    assert c["stats"]["levels_streamed"] >= 1
    t = tree_io.read_tree_file(c["params"]["tree_protobuf_path"])
    assert t["max_level"] == 12 and len(set(t["leaf_codes"].tolist())) == 3325 and sorted(t["leaf_ids"].tolist()) == sorted(c["ids"].tolist())
    assert ((t["leaf_codes"] >= (1 << 12) - 1) & (t["leaf_codes"] < (1 << 13) - 1)).all()
    e2 = Engine(0)
    r2 = tasks.tdm_train_deep_model(conf, engine=e2, time_recommend=False, max_iterations=5)
    assert len(r2["recommendation"]) == 3
    e2.close()


def test_g7_argument_errors(eng):
    L = N.lib()
    x = _uniform(10, 16)
    codes = np.zeros(10, np.int32)
    xp, cp = x.ctypes.data_as(N.f32p), codes.ctypes.data_as(N.i32p)
    call = lambda *a: L.dm_cluster_tree(eng._h, *a)
    assert call(xp, 0, 16, 3, 100, 1e-4, 1, cp, None, None) == -1
    assert call(xp, 10, 0, 3, 100, 1e-4, 1, cp, None, None) == -5 and call(xp, 10, 129, 3, 100, 1e-4, 1, cp, None, None) == -5
    assert call(xp, 10, 16, 0, 100, 1e-4, 1, cp, None, None) == -1 and call(xp, 10, 16, 33, 100, 1e-4, 1, cp, None, None) == -5
    assert call(None, 10, 16, 3, 100, 1e-4, 1, cp, None, None) == -1 and call(xp, 10, 16, 3, 100, 1e-4, 1, None, None, None) == -1
    assert call(xp, 10, 16, 3, 0, 1e-4, 1, cp, None, None) == -1
    assert b"restarts" in L.dm_last_error(eng._h) or b"max_iter" in L.dm_last_error(eng._h)
    small = N.ClusterTrace(1, 1, None, None, np.zeros(1, np.int32).ctypes.data_as(N.i32p), None, None, None)
    assert call(xp, 10, 16, 3, 100, 1e-4, 1, cp, C.byref(small), None) == -1 and b"node_cap" in L.dm_last_error(eng._h)
    assert L.dm_cluster_tree(None, xp, 10, 16, 3, 100, 1e-4, 1, cp, None, None) == -1
    ids = np.arange(1, 11, dtype=np.int32)
    ip = ids.ctypes.data_as(N.i32p)
    fresh = Engine(0)
    assert L.dm_cluster_tree_model(fresh._h, ip, 10, 3, 100, 1e-4, 1, cp, None, None) == -3            # nothing loaded
    assert L.dm_get_leaf_embeddings(fresh._h, ip, 10, xp) == -3
    t, _ = _fixture_model(fresh)
    bad = np.array([int(t["leaf_ids"][0]), int(t["leaf_ids"].max()) + 1000], np.int32)
    assert L.dm_cluster_tree_model(fresh._h, bad.ctypes.data_as(N.i32p), 2, 3, 100, 1e-4, 1, cp, None, None) == -1
    assert b"not a leaf" in L.dm_last_error(fresh._h)
    assert L.dm_get_leaf_embeddings(fresh._h, None, 2, xp) == -1
    for v in (np.nan, -np.inf):                                   # a non-finite row is refused by both entry points, the row named
        bad_x = x.copy()
        bad_x[4, 2] = v
        assert call(bad_x.ctypes.data_as(N.f32p), 10, 16, 3, 100, 1e-4, 1, cp, None, None) == -1
        assert b"dm_cluster_tree: row 4 " in L.dm_last_error(eng._h)
        w = np.load(os.path.join(GOLDEN, "din_f32.npy")).copy()
        two = t["leaf_ids"][:2].astype(np.int32)
        w[int(t["leaf_codes"][1]) * 16 + 7] = v
        fresh.load_weights_din(w, 16, 8191)
        assert L.dm_cluster_tree_model(fresh._h, two.ctypes.data_as(N.i32p), 2, 3, 100, 1e-4, 1, cp, None, None) == -1
        assert b"dm_cluster_tree_model: row 1 (item id %d)" % two[1] in L.dm_last_error(fresh._h)
    fresh.close()
    good, _, _ = eng.cluster_tree(x, restarts=3, seed=1)          # the handle still works after the refused calls
    R.check_structure(good, 10)
