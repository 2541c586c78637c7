"""The conditions tests/test_gpu_deepfm_jtm.py rests on, proved on the CPU (no device, no library):

(a) on every (E, L, old_level, level) case the GPU file scores, the reference's own float32 arithmetic (deepfm_ref.forward, float32: the
    FM buffer row by row, sequential dot products) stays within the project's fp32 contract 1e-5 + 1e-4 |f64| of float64 over all pairs
    of jtm_ref.expand_pairs(..., use_mask=False, num_index=2047), and expand_pairs reports no bad code: the contract is one a correct
    fp32 implementation can meet on these inputs;
(b) the per-history form of dfm_jtm_ref.pairs_forward — every pair with its own history, through seq_div — equals deepfm_ref.forward to
    1e-12 in float64, for shared (seq_div = chain nodes per row) and replicated (seq_div = 1) histories;
(c) the catalogue has the structure the kernels' tiling can go wrong on: at 2, 6 and 14 chain nodes per row some 16-pair tile holds two
    or more histories, some tile lies inside one item (the 40-row item), the last tile is partial; and the inputs hold a -1 node code's
    neighbours: the all-pad history and the unmasked -1 key."""
import numpy as np
import pytest

import deepfm_ref
import dfm_jtm_ref as D
import jtm_ref

_id = lambda c: "E%d-L%d-%dto%d" % c


@pytest.mark.parametrize("case", D.scorer_cases(), ids=_id)
def test_reference_float32_is_inside_the_contract(case):
    """(a)"""
    E, L, old_level, level = case
    px = D.pairs(L, old_level, level)
    assert not px["bad"] and px["codes"].max() < D.NI and px["codes"].min() >= 0
    codes, seqs, ref = D.scorer_inputs(E, L, old_level, level)            # (the same pairs, one node code set to -1)
    assert codes[5] == -1 and np.array_equal(np.delete(codes, 5), np.delete(px["codes"], 5)) and seqs is px["seqs"]
    f32 = deepfm_ref.forward(D.weights(E, L), E, L, D.NI, codes, seqs, np.float32)
    assert f32.dtype == np.float32 and np.isfinite(ref).all()
    ratio = np.abs(f32.astype(np.float64) - ref) / D.tolerance(ref)
    print("E=%d L=%d %d->%d: %d pairs, float32 error / tolerance: max %.3f" % (E, L, old_level, level, ref.size, ratio.max()))
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("case", D.scorer_cases(), ids=_id)
def test_per_history_form_equals_the_graph(case):
    """(b), histories shared by the chain nodes of a row"""
    E, L, old_level, level = case
    px = D.pairs(L, old_level, level)
    ref = D.ref64(E, L, old_level, level)
    w = D.weights(E, L)
    nchain = jtm_ref.nchain_of(level - old_level)
    codes, seqs, sref = D.scorer_inputs(E, L, old_level, level)
    assert np.abs(D.pairs_forward(w, E, L, D.NI, codes, seqs[::nchain], nchain) - sref).max() <= 1e-12      # a -1 node code is a zero row
    own = D.pairs_forward(w, E, L, D.NI, px["codes"], px["seqs"], 1)
    assert np.abs(own - ref).max() <= 1e-12
    per_row = px["seqs"].reshape(-1, nchain, L)                # every chain node of a row has the row's history: read it once per row
    assert (per_row == per_row[:, :1]).all()
    shared = D.pairs_forward(w, E, L, D.NI, px["codes"], px["seqs"][::nchain], nchain)
    assert np.abs(shared - ref).max() <= 1e-12
    for P in (1, 17):                                          # a prefix of the pairs reads a prefix of the histories
        got = D.pairs_forward(w, E, L, D.NI, px["codes"][:P], px["seqs"][::nchain][:-(-P // nchain)], nchain)
        assert np.abs(got - ref[:P]).max() <= 1e-12


@pytest.mark.parametrize("E,L", D.PIPELINE_EL)
@pytest.mark.parametrize("gap", [1, 2, 3])
def test_per_history_form_equals_the_graph_hierarchical(E, L, gap):
    """(b), the hierarchical pipeline cases (min_level 6 over old_level 4): one history per pair"""
    px = D.pairs(L, 4, 4 + gap, True, 6)
    assert not px["bad"]
    own = D.pairs_forward(D.weights(E, L), E, L, D.NI, px["codes"], px["seqs"], 1)
    assert np.abs(own - D.ref64(E, L, 4, 4 + gap, True, 6)).max() <= 1e-12


@pytest.mark.parametrize("L", sorted({L for _, L in D.SCORER_EL}))
def test_catalogue_structure(L):
    """(c)"""
    cat = D.catalogue(L)
    assert int(cat["row_off"][-1]) == 943 and cat["items"].size == D.LEAVES - 2
    nrows = np.diff(cat["row_off"])
    assert (nrows == 0).sum() >= 5 and (nrows == 1).any() and (nrows == 40).sum() == 1
    for nchain in (2, 6, 14):
        multi, inside, tail = D.tile_structure(cat["row_off"], nchain)
        assert multi > 0 and inside > 0 and 0 < tail < 16, (nchain, multi, inside, tail)
    codes, pad, bad = jtm_ref.id_to_code_with_mask(cat["row_ids"], cat["id_to_code"], cat["non_leaf_offset"], cat["max_code"], num_index=D.NI)
    assert not bad.any()
    assert (codes == -1).all(axis=1).any()                     # the all-pad history
    assert ((codes == -1) & ~pad).any()                        # the unmasked -1 key: a zero row that is no padding id


def test_hierarchical_cases_lift_some_levels_only():
    """min_level 6 on old_level 4: the level-5 pairs keep the leaf codes, deeper ones are lifted — the hierarchical pipeline cases differ
    from the flat ones and need one history per pair"""
    for L in (10, 15):
        flat, hier = D.pairs(L, 4, 7), D.pairs(L, 4, 7, True, 6)
        a, b = hier["seqs"].reshape(-1, 14, L), flat["seqs"].reshape(-1, 14, L)
        assert np.array_equal(a[:, :2], b[:, :2]) and (a[:, 2:] != b[:, 2:]).any() and not hier["bad"]
