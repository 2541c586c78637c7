"""CPU checks of tests/dfm_otm_tree_ref.py, the restatement tests/test_gpu_deepfm_otm_tree.py holds the device to: the reference's own
float32 arithmetic meets the bound on every case, the bound sees three mistakes a kernel could make, the segmented sum is strict row
order up to a segment's length, and the unit list covers every (item, chain tile, row) once."""
import numpy as np
import pytest

import dfm_otm_tree_ref as D


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_float32_restatement_meets_the_bound(c):
    E, L, old_level, gap, rows, n_items, seg = c
    row_off, h, node, lg64, w64, b = D.case_ref(c)
    w32 = D.weights_from_logits(D.pair_logits(E, L, row_off, h, node, gap, np.float32), row_off, gap, seg)
    has = np.diff(row_off) > 0
    assert (w32[~has] == -1e6).all() and (w64[~has] == -1e6).all()
    ratio = (np.abs(w32 - w64)[has] / b[has]).max()
    print("%s: float32 restatement uses %.4f of the bound" % (D.case_id(c), ratio))
    assert ratio <= 1.0


MUTATIONS = {
    "last row dropped": dict(drop_last=True),
    "upper depths left out": dict(depths=None),          # filled in per case: only d = gap
    "sibling's parent": dict(parent=lambda idx: (idx >> 1) ^ 1),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
@pytest.mark.parametrize("c", [c for c in D.CASES if c[3] >= 2 and c[4] == D.ROWS_SMALL], ids=D.case_id)
def test_the_bound_sees_a_mutation(c, name):
    """at least 90 % of the weights of items that have rows leave the bound (the project's 90 % convention)"""
    E, L, old_level, gap, rows, n_items, seg = c
    row_off, h, node, lg64, w64, b = D.case_ref(c)
    kw = dict(MUTATIONS[name])
    if "depths" in kw:
        kw["depths"] = (gap,)
    lg32 = D.pair_logits(E, L, row_off, h, node, gap, np.float32)
    bad = D.weights_from_logits(lg32, row_off, gap, seg, **kw)
    has = np.diff(row_off) > (1 if name == "last row dropped" else 0)          # (an item's only row dropped: nothing left to compare)
    caught = (np.abs(bad - w64)[has] > b[has]).mean()
    print("%s, %s: caught on %.3f of the weights" % (D.case_id(c), name, caught))
    assert caught >= 0.9


def test_segmented_sum_is_row_order_up_to_a_segment():
    rng = np.random.default_rng(9)
    row_off = np.array([0, 255, 511, 768, 768, 769], np.int64)
    lg = rng.standard_normal((769, 6)) * 3          # (full double mantissas: sums of float32 logits are mostly exact in double, in any order)
    strict = D.weights_from_logits(lg, row_off, 2, seg=1 << 40)
    native = D.weights_from_logits(lg, row_off, 2)
    assert native[[0, 1, 3, 4]].tobytes() == strict[[0, 1, 3, 4]].tobytes()          # 255, 256, 0 and 1 rows
    assert native[2].tobytes() == strict[2].tobytes()          # 257 rows: the second segment is one row, p + (0 + l) = p + l
    wide = D.weights_from_logits(lg, np.array([0, 769], np.int64), 2)
    assert wide.tobytes() != D.weights_from_logits(lg, np.array([0, 769], np.int64), 2, seg=1 << 40).tobytes()          # four segments
    assert np.abs(wide - D.weights_from_logits(lg, np.array([0, 769], np.int64), 2, seg=1 << 40)).max() < 1e-9
    short = D.weights_from_logits(lg, row_off, 2, seg=4)
    assert short[[3, 4]].tobytes() == strict[[3, 4]].tobytes() and short[0].tobytes() != strict[0].tobytes()


@pytest.mark.parametrize("gap", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("seg", [1, 4, 256])
def test_unit_list_covers_every_item_tile_row_once(gap, seg):
    row_off = np.array([0, 0, 1, 4, 8, 13, 24, 24, 281, 537, 792], np.int64)
    nchain = (2 << gap) - 2
    ntiles = (nchain + 15) // 16
    seen = np.zeros((int(row_off[-1]), ntiles), np.int32)
    for item, tile, r0, nr in D.units(row_off, gap, seg):
        assert 1 <= nr <= seg and 0 <= tile < ntiles and row_off[item] <= r0 and r0 + nr <= row_off[item + 1]
        assert (r0 - row_off[item]) % seg == 0
        seen[r0:r0 + nr, tile] += 1
    assert (seen == 1).all()
    assert ntiles * 16 - nchain < 16 and D.chain_codes([5], gap).shape == (1, nchain)


def test_chain_codes_are_the_descendants_in_level_order():
    codes = D.chain_codes([0, 6], 3)
    assert codes[0].tolist() == list(range(1, 15))
    assert codes[1].tolist() == [13, 14, 27, 28, 29, 30, 55, 56, 57, 58, 59, 60, 61, 62]
