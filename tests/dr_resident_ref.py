"""Restatements for the resident Deep-Retrieval mapping and training set on Python integers, and the cases both the CPU
and the GPU tests walk: the shuffle's order, the path -> items CSR of an item -> paths table."""
import numpy as np

import cluster_ref

M64 = (1 << 64) - 1
SHUFFLE_SEEDS = (20240607, 3)
SHUFFLE_EPOCHS = (1, 7)


def shuffle_order(seed, epoch, n):
    """the sample indices sorted ascending by key(i) = splitmix(splitmix(seed ^ splitmix(epoch)) + i), stable"""
    sm = cluster_ref.splitmix
    base = sm((seed ^ sm(epoch & M64)) & M64)
    keys = [sm((base + i) & M64) for i in range(n)]
    return np.array(sorted(range(n), key=lambda i: keys[i]), np.int32)


def csr(item_paths, K):
    """-> (codes [P] ascending, item_off [P + 1], items): every distinct path code sum_d node_d K^(D-1-d) with its items in ascending
    id, an item that lists one path twice counted once"""
    buckets = {}
    for item, paths in enumerate(np.asarray(item_paths).tolist()):
        for path in paths:
            code = 0
            for node in path:
                code = code * K + node
            b = buckets.setdefault(code, [])
            if not b or b[-1] != item:
                b.append(item)
    codes = sorted(buckets)
    off, items = [0], []
    for c in codes:
        items += buckets[c]
        off.append(len(items))
    return np.array(codes, np.int64), np.array(off, np.int64), np.array(items, np.int32)


def decode(codes, K, D):
    codes = np.asarray(codes, np.int64)
    out = np.empty(codes.shape + (D,), np.int32)
    for d in range(D - 1, -1, -1):
        out[..., d] = codes % K
        codes = codes // K
    return out


def encode(paths, K):
    paths = np.asarray(paths, np.int64)
    code = np.zeros(paths.shape[:-1], np.int64)
    for d in range(paths.shape[-1]):
        code = code * K + paths[..., d]
    return code


# name: (num_item, J, K, D, kind).  4095 / 4096 / 4097 entries: one tile of the sort and the compaction, its edge, the second tile
MAPPING_CASES = {
    "j1": (64, 1, 16, 2, "random"),
    "j2": (64, 2, 16, 2, "random"),
    "j3": (64, 3, 16, 2, "random"),
    "d3-k7": (50, 2, 7, 3, "random"),
    "twice": (64, 3, 16, 2, "twice"),
    "one-path": (64, 2, 16, 2, "one-path"),
    "distinct": (64, 2, 16, 2, "distinct"),
    "one-item": (1, 2, 16, 2, "random"),
    "m4095": (1365, 3, 16, 2, "random"),
    "m4096": (2048, 2, 16, 2, "random"),
    "m4097": (4097, 1, 16, 2, "random"),
    "wide-codes": (300, 2, 1000, 4, "random"),        # K^D = 10^12: codes pass 2^32
}
# the entry counts at which the digit scan of the sort and the tile scan of the compaction take a second and a third chunk
# (tests/sort_ref.py: SORT_BIG_SIZES, SELECT_BIG_SIZES), J = 1
BIG_MAPPING_SIZES = (257 * 4096 + 5, 513 * 4096 + 1, 1025 * 4096 + 3, 2049 * 4096 + 1)


def mapping_case(name):
    ni, J, K, D, kind = MAPPING_CASES[name]
    rng = np.random.default_rng(sorted(MAPPING_CASES).index(name) + 11)
    p = rng.integers(0, K, size=(ni, J, D), dtype=np.int32)
    if kind == "twice":
        p[5, 2] = p[5, 0]                      # one item lists a path twice ...
        p[9, 1] = p[9, 0]; p[9, 2] = p[9, 0]   # ... and one three times
        p[6, 0] = p[5, 0]                      # a neighbour shares it
    elif kind == "one-path":
        p[:] = np.array([3, 11], np.int32)
    elif kind == "distinct":
        p = decode(rng.permutation(K ** D)[:ni * J].reshape(ni, J), K, D)
    return np.ascontiguousarray(p, np.int32), K, D


def big_mapping_case(m, K=1000, D=2):
    rng = np.random.default_rng(m)
    return rng.integers(0, K, size=(m, 1, D), dtype=np.int32), K, D
