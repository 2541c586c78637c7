"""TDMClusterTree, host side (no GPU): the embeddings file, the numpy restatement's own invariants (the reference's ClusterTreeSpec),
the conditions the GPU tests put on their inputs, the ABI declarations and the task wiring."""
import json
import os
import re

import numpy as np
import pytest

import cluster_ref as R
from dismember_amd import _native as N
from dismember_amd import cluster, tasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_embeddings_file_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((40, 16)) * 0.05).astype(np.float32)
    x[0, :4] = [0.0, -1e-14, 123.5, -2.0]
    ids = rng.permutation(np.arange(5, 45)).astype(np.int32)
    p = str(tmp_path / "embed.csv")
    cluster.write_embeddings(p, ids, x)
    lines = open(p).read().splitlines()
    assert len(lines) == 40 and all(re.fullmatch(r"\d+(, -?\d+(\.\d{1,12})?){16}", l) for l in lines)      # no exponent, no grouping
    got_ids, got = cluster.read_embeddings(p)
    assert got_ids.tolist() == sorted(ids.tolist())
    want = x[np.argsort(ids)]
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 0.5e-12 + 2.0 ** -24 * np.abs(want).max()
    assert lines[0].startswith("5, ") and cluster._fmt(0.1234567890123) == "0.123456789012" and cluster._fmt(2.0) == "2"


def test_restatement_structure_on_uniform_data():
    x = np.random.default_rng(1).random((5000, 16)).astype(np.float32)          # ClusterTreeSpec: 5 000 x 16 uniform
    ids = np.arange(5000)
    codes = R.recursive_cluster(x, restarts=2, seed=1)
    assert len(ids) == len(codes)
    ml = R.max_level(5000)
    assert ml == 13 and (codes >= 2 ** (ml - 1) - 1).all()                      # getMinCode
    assert len(set(codes.tolist())) == 5000
    flat = R.flatten_leaves(codes, 2 ** ml - 1)
    assert ((flat >= 2 ** ml - 1) & (flat < 2 ** (ml + 1) - 1)).all()
    R.check_structure(codes, 5000)
    for n in (1, 2, 3, 255, 256, 257):
        R.check_structure(R.recursive_cluster(x[:n], restarts=1, seed=2), n)


@pytest.mark.parametrize("sigma", [0.0, 1e-4, 1e-3])
def test_planted_inputs_are_recoverable(sigma):
    """the condition G4 puts on its inputs: the restatement recovers planted levels 1..6 fully"""
    x, leaf = R.planted(10, 16, sigma, 7)
    codes = R.recursive_cluster(x, restarts=10, seed=3)
    assert [R.recovery(codes, leaf, 10, l) for l in range(1, 7)] == [1.0] * 6


def test_planted_nodes_are_two_separated_blobs():
    """the condition G3 puts on its inputs: at every planted node of three items or more the two children are blobs whose gap exceeds
    their spread, and Lloyd from ANY two seeds on opposite sides ends at the same pair of means"""
    x, leaf = R.planted(10, 16, 1e-4, 7)
    x64 = x.astype(np.float64)
    for level in range(0, 9):
        for g in range(0, 1 << level, max(1, (1 << level) // 4)):
            idx = np.flatnonzero((leaf >> (10 - level)) == g)
            side = (leaf[idx] >> (10 - level - 1)) & 1
            a, b = x64[idx][side == 0], x64[idx][side == 1]
            gap = np.sqrt(R.sqdist(a.mean(axis=0), b.mean(axis=0)))
            spread = max(np.sqrt(R.sqdist(a, a.mean(axis=0)).max()), np.sqrt(R.sqdist(b, b.mean(axis=0)).max()))
            assert gap > 1.3 * spread, (level, g, gap, spread)


def test_tolerance_file_is_what_numpy_gives():
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "cluster_tolerances.json")))
    for name, d in t["distance"].items():
        assert d["bound_rel"] == pytest.approx(4 * d["measured_rel"]) and 2.0 ** -24 < d["measured_rel"] < 1e-5
    c = t["centroid"]
    assert c["bound_abs"] == pytest.approx(4 * (c["measured_f32_mean_abs"] + c["f32_rounding_abs"]))
    x, _ = R.planted(10, 16, 1e-4, 7)
    assert R.f32_distance_error(x, x.mean(axis=0)) <= t["distance"]["planted_1024x16"]["bound_rel"]


def test_abi_declares_the_cluster_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    for name in ("dm_cluster_tree", "dm_cluster_tree_model", "dm_get_leaf_embeddings"):
        assert name in N.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert "dm_cluster_trace" in hdr and "dm_cluster_stats" in hdr
    assert len(N.SIGNATURES["dm_cluster_tree"][1]) == 11 and len(N.SIGNATURES["dm_cluster_tree_model"][1]) == 10


def test_spectral_is_refused_and_dispatcher_line_stays(tmp_path):
    with pytest.raises(ValueError):
        cluster.RecursiveCluster(None, [1, 2, 3], np.zeros((3, 4), np.float32), cluster_type="spectral")
    with pytest.raises(ValueError):
        cluster.RecursiveCluster(None, [1, 2, 3], np.zeros((3, 4), np.float32), cluster_type="dbscan")
    assert tasks.tdm_cluster_tree is cluster.tdm_cluster_tree
    from test_tasks import _conf
    assert tasks.main(["TDMClusterTree", "--tdmConfFile", _conf(tmp_path)]) == 3
    assert cluster.main([]) == 2
