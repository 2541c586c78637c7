"""tests/jtm_ref.py (the numpy restatement of the JTM child-weight pipeline) against the CPU oracle, before tests/test_gpu_jtm_scoring.py
lets it judge the kernels.  No device.

The oracle (oracle/dm_oracle.c: orc_jtm_child_weights) walks child -> parent per (item, child) and runs one forward over the item's
rows per step, summing in fp32; the restatement expands every (row, chain node) pair once and sums the same logits in the same order.
The bound on a weight is that of a sequential fp32 sum of its n = rows * gap terms, (n - 1) * 2^-24 * sum |logit| (jtm_ref.sum_bound_f32):
derived, not measured.  The oracle's forward of ONE row takes the reference's 1-D Linear path (bias first), so the logits are taken per
(item, chain node) in batches of the item's rows, as the oracle takes them."""
import numpy as np
import pytest

import jtm_ref
from dismember_amd import synth
from helpers import random_din_weights

DEPTH, ITEMS, E, L = 8, 120, 16, 10
NI = (1 << (DEPTH + 1)) - 1


@pytest.fixture(scope="module")
def problem(oracle):
    rng = np.random.default_rng(81)
    tree = synth.make_tree(ITEMS, DEPTH, rng)
    cat = jtm_ref.make_catalogue(rng, tree["leaf_ids"], tree["leaf_codes"], L, big=20)
    w = random_din_weights(rng, E, NI)
    otree = oracle.TdmTree(tree["codes"], tree["ids"], tree["is_leaf"], cat["map_ids"], cat["map_codes"], DEPTH)
    assert otree.non_leaf_offset == cat["non_leaf_offset"] and otree.max_code == cat["max_code"]
    return cat, otree, oracle.Din(w, E, L, NI)


def test_catalogue_has_the_edges_the_gpu_tests_rely_on():
    rng = np.random.default_rng(5)
    tree = synth.make_tree(300, 10, rng)
    for Lh in (1, 7, 10, 16):
        cat = jtm_ref.make_catalogue(rng, tree["leaf_ids"], tree["leaf_codes"], Lh, holes=2)
        nr = np.diff(cat["row_off"]); n = nr.size
        assert n == 298 and nr[0] == 0 and nr[-1] == 0 and (nr[20:23] == 0).all() and (nr == 1).sum() >= 5 and nr.max() == 40
        assert set(np.unique(nr).tolist()) == {0, 1, 2, 3, 4, 5, 40}
        rows, nlo, mc = cat["row_ids"], cat["non_leaf_offset"], cat["max_code"]
        for e in (0, nlo + 5, nlo + mc, nlo + mc + 1):
            assert (rows == e).any(), (Lh, e)
        assert (rows == 0).all(axis=1).any()
        assert cat["hole_ids"].size == 2 and not np.isin(rows, cat["hole_ids"]).any() and (cat["id_to_code"][cat["hole_ids"]] == -1).all()
        cd, m, bad = jtm_ref.id_to_code_with_mask(rows, cat["id_to_code"], nlo, mc, num_index=2047)
        assert not bad.any() and np.array_equal(m, rows == 0)
        assert (cd[rows == nlo + 5] == 5).all() and (cd[rows == nlo + mc] == mc).all()
        assert (cd[rows == nlo + mc + 1] == -1).all() and not m[rows == nlo + mc + 1].any()
        # a hole: the reference's lookup would fail on it
        cd, m, bad = jtm_ref.id_to_code_with_mask(cat["hole_ids"], cat["id_to_code"], nlo, mc, num_index=2047)
        assert bad.all() and (cd == -1).all() and not m.any()


def test_id_to_code_equals_the_oracle(problem, oracle):
    cat, otree, _ = problem
    ids = np.concatenate([cat["row_ids"].reshape(-1), np.arange(0, cat["non_leaf_offset"] + cat["max_code"] + 40, dtype=np.int32)])
    for level, hier, min_level in [(0, False, 0), (5, True, 6), (6, True, 6), (7, True, 6), (8, True, 0)]:
        cd, m, bad = jtm_ref.id_to_code_with_mask(ids, cat["id_to_code"], cat["non_leaf_offset"], cat["max_code"], level, hier, min_level)
        oc = np.empty_like(ids); om = np.empty_like(ids)
        nm = oracle.lib().orc_jtm_id_to_code_with_mask(otree.h, ids.ctypes.data_as(oracle.i32p), ids.size, level, int(hier), min_level,
                                                       oc.ctypes.data_as(oracle.i32p), om.ctypes.data_as(oracle.i32p))
        assert not bad.any() and np.array_equal(cd, oc) and np.array_equal(np.flatnonzero(m), om[:nm])


@pytest.mark.parametrize("use_mask", [True, False])
@pytest.mark.parametrize("hierarchical", [False, True])
@pytest.mark.parametrize("gap", [1, 2, 3])
def test_restatement_equals_the_oracle(problem, oracle, gap, hierarchical, use_mask):
    cat, otree, odin = problem
    old_level, level, min_level = 4, 4 + gap, 6
    item_node = jtm_ref.ancestor_at_level(cat["item_code"], old_level).astype(np.int32)
    w_ref = oracle.jtm_child_weights(otree, odin, cat["items"], cat["row_off"], cat["row_ids"], item_node, L, old_level, level,
                                     hierarchical=hierarchical, min_level=min_level, use_mask=use_mask)
    px = jtm_ref.expand_pairs(cat["row_off"], cat["row_ids"], item_node, L, old_level, level, cat["id_to_code"], cat["non_leaf_offset"],
                              cat["max_code"], hierarchical, min_level, use_mask, NI)
    assert not px["bad"]
    nchain = jtm_ref.nchain_of(gap)
    # bookkeeping of the pair order
    assert np.array_equal(px["row"], np.repeat(np.arange(cat["row_off"][-1]), nchain)) and np.array_equal(px["chain"], np.tile(np.arange(nchain), int(cat["row_off"][-1])))
    assert np.array_equal(px["item"], np.repeat(np.repeat(np.arange(cat["items"].size), np.diff(cat["row_off"])), nchain))
    if not use_mask:
        assert not px["mask"].any()
    # the oracle's forward, one batch per (item, chain node) over the item's rows
    logits = np.empty(px["codes"].size, np.float32)
    for i in range(cat["items"].size):
        a, b = int(cat["row_off"][i]), int(cat["row_off"][i + 1])
        for x in range(nchain):
            q = np.arange(a, b) * nchain + x
            if q.size:
                logits[q] = odin.forward(px["codes"][q], px["seqs"][q], jtm_ref.pad_flat(px["mask"][q]))
    w = jtm_ref.sum_weights_f32(logits, cat["row_off"], gap)
    seen = np.diff(cat["row_off"]) > 0
    assert (w[~seen] == np.float32(-1e6)).all() and (w_ref[~seen] == np.float32(-1e6)).all()
    bound = jtm_ref.sum_bound_f32(logits, cat["row_off"], gap)
    err = np.abs(w.astype(np.float64) - w_ref.astype(np.float64))
    print("gap %d hierarchical %d use_mask %d: max |restatement - oracle| = %.3g, smallest bound %.3g" % (gap, hierarchical, use_mask, err[seen].max(), bound[seen].min()))
    assert w_ref.dtype == np.float32 and (err[seen] <= bound[seen]).all()
    # chain-node codes: the oracle's children of the item's node, level by level
    first = (item_node.astype(np.int64) << gap) + (1 << gap) - 1
    deepest = px["codes"].reshape(-1, nchain)[:, (1 << gap) - 2:]
    assert np.array_equal(deepest, (first[px["item"].reshape(-1, nchain)[:, 0]])[:, None] + np.arange(1 << gap)[None, :])
