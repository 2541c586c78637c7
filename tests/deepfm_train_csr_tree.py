"""A small tree with leaves on TWO levels, for the tests of the ragged DeepFM training path (tests/test_deepfm_train_csr_host.py,
tests/test_gpu_deepfm_train_csr.py).  Test infrastructure only.  The heap is complete down to level 5; the first 16 nodes of level 5 have
both children on level 6 (32 leaves), the other 16 are leaves themselves: 48 items, and a target's row count depends on its leaf's level.
"""
import numpy as np

DEPTH = 6
N_ITEMS = 48
NUM_INDEX = (1 << (DEPTH + 1)) - 1
START_LEVEL = 1
NEG = np.array([0, 1, 2, 3, 4, 4, 4], np.int32)
L = 10
T_TARGETS = 40


def leaf_codes():
    return np.concatenate([np.arange(63, 95), np.arange(47, 63)]).astype(np.int32)


def tree():
    """dict like helpers.synthetic_tree's"""
    lc = leaf_codes()
    leaf_ids = (np.random.default_rng(5).permutation(N_ITEMS) + 1).astype(np.int32)
    codes = np.array(sorted(set(range(0, 63)) | set(lc.tolist())), np.int32)
    off = int(leaf_ids.max()) + 1
    lut = {int(c): int(i) for c, i in zip(lc, leaf_ids)}
    ids = np.array([lut.get(int(c), int(c) + off) for c in codes], np.int32)
    is_leaf = np.array([int(c) in lut for c in codes], np.uint8)
    return dict(codes=codes, ids=ids, is_leaf=is_leaf, leaf_ids=leaf_ids, leaf_codes=lc, max_level=np.int32(DEPTH))


def targets(seed=21):
    """(histories [T, L] of item ids with prefix padding, targets [T]): target 3 is padding, target 7 outside the tree, the rest leaves of
    both levels"""
    t = tree()
    rng = np.random.default_rng(seed)
    seq = rng.choice(t["leaf_ids"], (T_TARGETS, L)).astype(np.int32)
    for u, n in enumerate(rng.binomial(L, 0.15, T_TARGETS)):
        seq[u, :n] = 0
    seq[5] = 0                                                   # an all-padding history
    tgt = rng.choice(t["leaf_ids"], T_TARGETS).astype(np.int32)
    tgt[3] = 0
    tgt[7] = N_ITEMS + 500
    return seq, tgt


def expected_counts(tgt):
    """rows per target: sum over levels START_LEVEL .. the leaf's level of 1 + NEG[level]"""
    t = tree()
    level = {int(i): int(np.log2(int(c) + 1)) for i, c in zip(t["leaf_ids"], t["leaf_codes"])}
    per = lambda lv: int(sum(1 + NEG[l] for l in range(START_LEVEL, lv + 1)))
    return np.array([per(level[int(i)]) if int(i) in level else 0 for i in np.asarray(tgt)], np.int64)
