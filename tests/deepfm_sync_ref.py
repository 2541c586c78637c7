"""numpy restatement of the DeepFM gradient exchange (dismember_amd/csrc/dfm_train_sync.hip.inc; reference:
tdm/.../optim/LocalOptimizer.scala:164-187 minus the division) and the batches tests/test_gpu_deepfm_sync.py runs.  Test infrastructure only.

A rank contributes (rows, grads, tail): its sorted unique table rows, their gradient rows [n, E] and the dense tail
[l1.W ; l1.b ; l2.W ; l2.b].  After the exchange every replica holds, for every row any rank reached, ((0 + g_0) + g_1) + ... in float32
and in rank order, ranks that did not reach the row skipped, and the same rank-ordered sum of the tails.  That equals the dense float32
sum 0 + G_0 + G_1 + ... of the ranks' whole gradient vectors up to the sign of a zero (x + 0 == x), which np.array_equal does not see.
"""
import functools

import numpy as np

import deepfm_ref as R

NUM_INDEX = 8191
CASES = ("shared_w2", "shared_w3", "disjoint", "empty_rank", "one_row_and_513_identical", "embed_24", "seq_len_32", "tile_4095_4097")
EDGES = CASES[3:]


def tail_len(E, L):
    T = L + 1
    return T * T * E + 2 * T + 1


def batch_rows(codes, seqs, NI):
    """the sorted unique table rows a batch reaches (ids outside [0, NI) are padding)"""
    ids = np.concatenate([np.asarray(codes, np.int64).ravel(), np.asarray(seqs, np.int64).ravel()])
    return np.unique(ids[(ids >= 0) & (ids < NI)])


def split(g, rows, E, NI):
    """a rank's whole gradient vector (the model's own layout) -> its block (rows, grads [n, E], tail)"""
    g = np.asarray(g, np.float32)
    return np.asarray(rows, np.int64), g[:NI * E].reshape(NI, E)[rows].copy(), g[NI * E:].copy()


def exchange(blocks, E, NI):
    """blocks: per rank (rows, grads, tail) -> (union rows, summed rows [n, E], summed tail), float32, rank order"""
    union = np.unique(np.concatenate([b[0] for b in blocks])) if blocks else np.zeros(0, np.int64)
    acc = np.zeros((union.size, E), np.float32)
    tail = np.zeros_like(np.asarray(blocks[0][2], np.float32))
    for rows, grads, t in blocks:
        assert np.all(np.diff(rows) > 0), "a rank's rows are sorted and unique"
        pos = np.searchsorted(union, rows)
        acc[pos] = acc[pos] + np.asarray(grads, np.float32)          # rows are unique inside a rank: one add per row
        tail = tail + np.asarray(t, np.float32)
    return union, acc, tail


def assemble(union, acc, tail, E, NI):
    """the exchanged gradient as a whole vector: untouched rows are zero"""
    g = np.zeros(NI * E + tail.size, np.float32)
    g[:NI * E].reshape(NI, E)[union] = acc
    g[NI * E:] = tail
    return g


def dense_sum(gs):
    """0 + G_0 + G_1 + ... in float32"""
    want = np.zeros_like(np.asarray(gs[0], np.float32))
    for g in gs:
        want = want + np.asarray(g, np.float32)
    return want


def _shared_batch(rank, B, L, NI, vocab=400):
    rng = np.random.default_rng(700 + rank)
    codes = rng.integers(1, NI, B).astype(np.int32)
    seqs = rng.integers(0, vocab, (B, L)).astype(np.int32)            # a small history vocabulary: most rows are reached by every rank
    seqs[rng.random((B, L)) < 0.2] = -1
    y = (rng.random(B) < 0.3).astype(np.float32) * np.float32(37.0 ** rank)      # very different magnitudes per rank: the order is visible
    return codes, seqs, y


def _exact_rows_batch(rng, n_rows, L, NI):
    """a batch that reaches exactly n_rows different table rows: a permutation's head, cut into rows of L + 1 slots, the rest padding"""
    T = L + 1
    B = -(-n_rows // T)
    ids = np.full(B * T, -1, np.int32)
    ids[:n_rows] = rng.permutation(NI)[:n_rows]
    ids = ids.reshape(B, T)
    return ids[:, 0].copy(), ids[:, 1:].copy(), (rng.random(B) < 0.3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(E, L, NI, W, w, batches): batches[r] = (codes [B], seqs [B, L], y [B]) of rank r; B may be 0"""
    E, L, NI, W = 16, 10, NUM_INDEX, 2
    rng = np.random.default_rng(81000 + CASES.index(name))
    if name.startswith("shared_w"):
        W = int(name[-1])
        batches = [_shared_batch(r, 96, L, NI) for r in range(W)]
    elif name == "disjoint":
        batches = []
        for r in range(W):                                            # rank r draws every id from [4000 r, 4000 r + 4000)
            codes = rng.integers(4000 * r, 4000 * r + 4000, 96).astype(np.int32)
            seqs = rng.integers(4000 * r, 4000 * r + 4000, (96, L)).astype(np.int32)
            seqs[rng.random((96, L)) < 0.2] = -1
            batches.append((codes, seqs, (rng.random(96) < 0.3).astype(np.float32)))
    elif name == "empty_rank":
        batches = [_shared_batch(0, 96, L, NI), (np.zeros(0, np.int32), np.zeros((0, L), np.int32), np.zeros(0, np.float32))]
    elif name == "one_row_and_513_identical":
        c0, s0, y0 = _shared_batch(0, 1, L, NI)
        c1, s1, y1 = _shared_batch(1, 513, L, NI)
        c1[:] = c1[0]; s1[:] = s1[0]; s1[:, 4] = c1[0]      # 513 slots per destination (1026 for the item's own row)
        s1[:, 0] = 7; s0[0, 0] = 7                          # and one destination shared with rank 0's only row
        batches = [(c0, s0, y0), (c1, s1, y1)]
    elif name == "embed_24":
        E = 24
        batches = [_shared_batch(r, 96, L, NI) for r in range(W)]
    elif name == "seq_len_32":
        L = 32
        batches = [_shared_batch(r, 40, L, NI) for r in range(W)]
    elif name == "tile_4095_4097":
        batches = [_exact_rows_batch(rng, 4095, L, NI), _exact_rows_batch(rng, 4097, L, NI)]
    else:
        raise KeyError(name)
    w = R.random_deepfm_weights(rng, E, L, NI)
    for b in batches:
        for a in b:
            a.setflags(write=False)
    w.setflags(write=False)
    return dict(E=E, L=L, NI=NI, W=W, w=w, batches=batches)
