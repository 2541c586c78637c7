"""numpy restatement of the Deep-Retrieval gradient exchange (dismember_amd/csrc/dr_train_sync.hip.inc; reference:
deep-retrieval/.../optim/LocalOptimizer.scala:167-194 minus the division) and the cases tests/test_gpu_dr_sync.py runs.  Test
infrastructure only.

A rank contributes (rows, grads, tail): its sorted unique embedding rows (item rows and node rows), their gradient rows [n, E] and the
dense tail [W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}].  After the exchange every replica holds, for every row any rank reached,
((0 + g_0) + g_1) + ... in the model's dtype and in rank order, ranks that did not reach the row skipped, and the same rank-ordered sum
of the tails.  That equals the dense sum 0 + G_0 + G_1 + ... of the ranks' whole gradient vectors up to the sign of a zero (x + 0 == x),
which np.array_equal does not see.

The models are tests/dr_train_ref.py's small ones: K = 16, L = 4, E = 16, D = 2 or 3, num_item = 64 unless a case says otherwise.
"""
import functools

import numpy as np

from dismember_amd import synth
from dismember_amd.dr_train import pack_params

NP = {"f32": np.float32, "f64": np.float64}
K, L, E = 16, 4, 16

# name: (W, D, dtype, num_item, kind)
SPECS = {
    "shared_w2_f64": (2, 2, "f64", 64, "shared"),
    "shared_w2_f32": (2, 2, "f32", 64, "shared"),
    "shared_w3_f64": (3, 3, "f64", 64, "shared"),
    "shared_w3_f32": (3, 3, "f32", 64, "shared"),
    "disjoint_items_f64": (2, 3, "f64", 64, "disjoint"),             # item rows disjoint; node rows overlap by construction
    "identical_items_f32": (3, 2, "f32", 64, "identical"),           # every rank reaches the same item rows
    "all_padding_rank_f64": (2, 3, "f64", 64, "allpad"),             # -1 padding everywhere; rank 1's histories are nothing but padding
    "idle_middle_f64": (3, 2, "f64", 64, "idle1"),
    "idle_end_f32": (3, 3, "f32", 64, "idle2"),
    "one_row_and_513_identical_f64": (2, 2, "f64", 64, "one513"),
    "rows_odd_even_f64": (2, 2, "f64", 64, "parity01"),              # n_r odd on rank 0, even on rank 1: the alignment rule
    "rows_even_odd_f64": (2, 2, "f64", 64, "parity10"),
    "rows_odd_odd_even_f64": (3, 2, "f64", 64, "parity001"),
    "tile_4095_4096_4097_f64": (3, 2, "f64", 4200, "tile"),          # one below, at and one above the compaction's tile of 4096
    "adam_dense_f64": (2, 2, "f64", 64, "one513"),                   # one_row_and_513_identical_f64 again, run under DM_ADAM_DENSE=1
}
CASES = tuple(SPECS)
ENV = {"adam_dense_f64": {"DM_ADAM_DENSE": "1"}}
TWIN = {"adam_dense_f64": "one_row_and_513_identical_f64"}      # few rows: without the switch the Adam step takes the active-rows path
EXACT_ROWS = {"rows_odd_even_f64": (11, 12), "rows_even_odd_f64": (12, 11), "rows_odd_odd_even_f64": (9, 13, 10),
              "tile_4095_4096_4097_f64": (4095, 4096, 4097)}


def num_rows(dims):
    E_, L_, K_, D, NI = dims
    return NI + K_ * (D - 1)


def tail_len(dims):
    E_, L_, K_, D, NI = dims
    return sum(K_ * (L_ + d) * E_ + K_ for d in range(D))


def batch_rows(seq, paths, dims):
    """the sorted unique embedding rows a batch reaches: history ids (-1 = padding) and the node rows of positions t < D - 1"""
    E_, L_, K_, D, NI = dims
    seq, paths = np.asarray(seq, np.int64).reshape(-1, L_), np.asarray(paths, np.int64).reshape(-1, D)
    ids = [seq[seq >= 0].ravel()] + [NI + t * K_ + paths[:, t] for t in range(D - 1)]
    return np.unique(np.concatenate(ids)) if len(seq) else np.zeros(0, np.int64)


def block_bytes(n, dims, dtype):
    """a rank's block on the wire: n ids padded to an even count, n rows, the tail; a multiple of 8 bytes"""
    b = 4 * ((n + 1) // 2 * 2) + np.dtype(NP[dtype]).itemsize * (n * dims[0] + tail_len(dims))
    return (b + 7) // 8 * 8


def split(g, rows, dims):
    """a rank's whole gradient vector -> its block (rows, grads [n, E], tail)"""
    NR, E_ = num_rows(dims), dims[0]
    g = np.asarray(g)
    return np.asarray(rows, np.int64), g[:NR * E_].reshape(NR, E_)[rows].copy(), g[NR * E_:].copy()


def exchange(blocks, dims, dtype):
    """blocks: per rank (rows, grads, tail) -> (union rows, summed rows [n, E], summed tail) in `dtype`, rank order"""
    T = NP[dtype]
    union = np.unique(np.concatenate([b[0] for b in blocks]))
    acc = np.zeros((union.size, dims[0]), T)
    tail = np.zeros(tail_len(dims), T)
    for rows, grads, t in blocks:
        assert np.all(np.diff(rows) > 0), "a rank's rows are sorted and unique"
        assert np.asarray(grads).dtype == T and np.asarray(t).dtype == T
        pos = np.searchsorted(union, rows)
        acc[pos] = acc[pos] + grads                                  # rows are unique inside a rank: one add per row
        tail = tail + t
    return union, acc, tail


def assemble(union, acc, tail, dims):
    """the exchanged gradient as a whole vector: untouched rows are zero"""
    NR, E_ = num_rows(dims), dims[0]
    g = np.zeros(NR * E_ + tail.size, acc.dtype)
    g[:NR * E_].reshape(NR, E_)[union] = acc
    g[NR * E_:] = tail
    return g


def dense_sum(gs):
    """0 + G_0 + G_1 + ... in the vectors' own dtype"""
    want = np.zeros_like(np.asarray(gs[0]))
    for g in gs:
        assert np.asarray(g).dtype == want.dtype
        want = want + np.asarray(g)
    return want


# ---------------------------------------------------------------------------------------------------------------- batches
def _random(rng, B, D, NI, lo=0, hi=None, pad=0.2):
    seq = rng.integers(lo, NI if hi is None else hi, (B, L)).astype(np.int32)
    seq[rng.random((B, L)) < pad] = -1
    return seq, rng.integers(0, K, (B, D)).astype(np.int32)


def _exact_rows(rng, n, D, NI):
    """a batch (D = 2) that reaches exactly n embedding rows: min(n - 1, K) node rows, the rest item rows (a permutation's head, cut
    into histories of L, the remainder padding)"""
    assert D == 2
    n_nodes = min(n - 1, K)
    n_items = n - n_nodes
    assert 0 < n_items <= NI
    B = max(-(-n_items // L), n_nodes)
    seq = np.full(B * L, -1, np.int32)
    seq[:n_items] = rng.permutation(NI)[:n_items]
    paths = rng.integers(0, K, (B, D)).astype(np.int32)
    paths[:, 0] = np.arange(B) % n_nodes
    return seq.reshape(B, L), paths


def _empty(D):
    return np.zeros((0, L), np.int32), np.zeros((0, D), np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(dims, dtype, W, P, w, batches, env): batches[r] = (seq [B, L], paths [B, D]) of rank r, B = 0 for an idle rank; P = the
    ranks that ran a step (the Adam step's 1 / P); w = the flat weights as the device holds them, in float64"""
    if name in TWIN:
        return dict(case(TWIN[name]), env=ENV[name])
    W, D, dt, NI, kind = SPECS[name]
    rng = np.random.default_rng(91000 + CASES.index(name))
    if kind == "shared":                                             # batch sizes 7, 96, 300: gradients (means over B) of different magnitudes
        batches = [_random(rng, (7, 96, 300)[r], D, NI) for r in range(W)]
    elif kind == "disjoint":
        batches = [_random(rng, 64, D, NI, 32 * r, 32 * r + 32) for r in range(W)]
    elif kind == "identical":
        seq = _random(rng, 48, D, NI, pad=0.0)[0]
        batches = [(seq.copy(), rng.integers(0, K, (48, D)).astype(np.int32)) for _ in range(W)]
    elif kind == "allpad":
        s0, p0 = _random(rng, 40, D, NI, pad=0.4)
        s1, p1 = _random(rng, 33, D, NI)
        s1[:] = -1
        batches = [(s0, p0), (s1, p1)]
    elif kind in ("idle1", "idle2"):
        idle = int(kind[-1])
        batches = [_empty(D) if r == idle else _random(rng, (7, 96, 40)[r], D, NI) for r in range(W)]
    elif kind == "one513":
        s0, p0 = _random(rng, 1, D, NI, pad=0.0)
        s1, p1 = _random(rng, 513, D, NI, pad=0.0)
        s1[:] = s1[0]; p1[:] = p1[0]                                 # 513 (and 1026, 1539 for a repeated id) slots per destination
        s1[:, 0] = 7; s0[0, 0] = 7                                   # and one destination shared with rank 0's only row
        batches = [(s0, p0), (s1, p1)]
    elif kind.startswith("parity") or kind == "tile":
        batches = [_exact_rows(rng, n, D, NI) for n in EXACT_ROWS[name]]
    else:
        raise KeyError(name)
    wd = synth.make_dr_model(NI, K, D, L, E, rng, scale=0.3)
    w = pack_params(wd, NP[dt]).astype(np.float64)
    for b in batches:
        for a in b:
            a.setflags(write=False)
    w.setflags(write=False)
    return dict(dims=(E, L, K, D, NI), dtype=dt, W=W, P=sum(1 for b in batches if len(b[0])), w=w, batches=batches, env=ENV.get(name, {}))
