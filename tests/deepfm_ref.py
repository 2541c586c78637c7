"""numpy restatement of the reference's DeepFM scorer, op for op (no GPU, no oracle library).

  tdm/src/main/scala/com/mass/tdm/model/DeepFM.scala:11-45   the graph
  scalann/src/main/scala/com/mass/scalann/nn/FM.scala:12-41   FM.updateOutput: running vAdd buffer, then two dots
  scalann/src/main/scala/com/mass/scalann/nn/Linear.scala:40-48   addmm(input, weight.t()) then addr(addBuffer, bias)

`dtype` is the arithmetic type of every intermediate (numpy float32 or float64).  The FM buffer adds the T feature rows one after the
other, as vAdd does.  The dots and the GEMM rows (ev.dot, addmm: BLAS calls in the reference, whose internal order is not stated) are
sequential chains in float32 — the plain reading, and the least favourable one for float32 — and numpy's own products in float64,
where the order moves the result by ~1e-16 relative, eleven orders of magnitude below the tolerance it is compared under.
"""
import numpy as np


def deepfm_param_count(E, L, num_index):
    T = L + 1
    return num_index * E + T * T * E + 2 * T + 1


def deepfm_offsets(E, L, num_index):
    """Block offsets of the compact vector in Graph.parameters order: emb, l1.W, l1.b, l2.W, l2.b, end."""
    T = L + 1
    o_emb = 0
    o_w1 = num_index * E
    o_b1 = o_w1 + T * T * E
    o_w2 = o_b1 + T
    o_b2 = o_w2 + T
    return dict(emb=o_emb, l1_w=o_w1, l1_b=o_b1, l2_w=o_w2, l2_b=o_b2, end=o_b2 + 1)


def random_deepfm_weights(rng, E, L, num_index, std=0.05):
    """Compact vector with the reference's initial distribution N(0, std) in every block (biases non-zero on purpose), float32."""
    return rng.normal(0.0, std, deepfm_param_count(E, L, num_index)).astype(np.float32)


def split(w, E, L, num_index, dtype):
    o = deepfm_offsets(E, L, num_index)
    T = L + 1
    w = np.asarray(w).astype(dtype)
    assert w.size == o["end"]
    return (w[o["emb"]:o["l1_w"]].reshape(num_index, E), w[o["l1_w"]:o["l1_b"]].reshape(T, T * E), w[o["l1_b"]:o["l2_w"]],
            w[o["l2_w"]:o["l2_b"]], w[o["l2_b"]])


def _dot(a, b, dtype):
    """sum_i a[..., i] * b[..., i]: float32 as a sequential chain, float64 through numpy."""
    if dtype is np.float64:
        return (a * b).sum(-1)
    acc = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], dtype)
    for i in range(a.shape[-1]):
        acc = acc + a[..., i] * b[..., i]
    return acc


def lookup(emb, idx):
    """EmbeddingShare with paddingIdx = -1: a zero row."""
    idx = np.asarray(idx)
    return np.where(idx[..., None] >= 0, emb[np.maximum(idx, 0)], emb.dtype.type(0))


def forward(w, E, L, num_index, codes, seqs, dtype=np.float64):
    """Module.forward(Table(item, seq)) -> logits [B] in `dtype`."""
    dtype = np.dtype(dtype).type
    emb, W1, b1, w2, b2 = split(w, E, L, num_index, dtype)
    codes = np.asarray(codes).reshape(-1)
    B, T = codes.size, L + 1
    seqs = np.asarray(seqs).reshape(B, L)
    item = lookup(emb, codes)                                   # itemFlatten [B, E]
    seq = lookup(emb, seqs).reshape(B, L * E)                   # seqFlatten  [B, L E]
    concat = np.concatenate([item, seq], axis=1).astype(dtype)  # Concat      [B, T E]
    feat = concat.reshape(B, T, E)                              # fmFeature
    # FM.updateOutput
    buf = np.zeros((B, E), dtype)
    for i in range(T):
        buf = (buf + feat[:, i, :]).astype(dtype)              # ev.vAdd into the buffer
    sum_square = _dot(buf, buf, dtype)
    square_sum = _dot(concat, concat, dtype)
    fm = ((sum_square - square_sum).astype(dtype) / dtype(2.0)).astype(dtype)
    # Linear(T E, T): addmm then addr(ones, bias); ReLU; Linear(T, 1); Add
    h = _dot(concat[:, None, :], W1[None, :, :], dtype) if dtype is np.float32 else concat @ W1.T      # addmm(input, weight.t())
    h = (h + b1[None, :]).astype(dtype)                                                                # addr(addBuffer, bias)
    h = np.maximum(h, dtype(0))
    out = (_dot(h, w2[None, :], dtype) + b2).astype(dtype)
    return (fm + out).astype(dtype)


def forward_restructured(w, E, L, num_index, codes, seq_codes, dtype=np.float64):
    """The per-user form the level kernel computes, for ONE history shared by all `codes`:
    s = sum_j k_j, c = (|s|^2 - sum_j |k_j|^2) / 2 + b2, a = W1s vec(K) + b1; logit = e.s + c + sum_t w2[t] relu(W1a[t].e + a[t])."""
    dtype = np.dtype(dtype).type
    emb, W1, b1, w2, b2 = split(w, E, L, num_index, dtype)
    K = lookup(emb, np.asarray(seq_codes).reshape(L))           # [L, E]
    s = K.sum(0, dtype=dtype)
    c = (np.dot(s, s) - (K * K).sum(dtype=dtype)) / dtype(2.0) + b2
    a = W1[:, E:] @ K.reshape(-1) + b1
    e = lookup(emb, np.asarray(codes).reshape(-1))              # [B, E]
    return (e @ s + c + np.maximum(e @ W1[:, :E].T + a[None, :], dtype(0)) @ w2).astype(dtype)


# ---- the inputs shared by tests/test_deepfm_host.py (CPU) and tests/test_gpu_deepfm.py
ROW_E = (16, 24, 128)
ROW_L = (1, 10, 14, 15, 30, 31, 32)
ROW_B = (1, 17, 777)
ROW_NUM_INDEX = 1023
SEARCH_E = (16, 128)
SEARCH_L = (10, 15, 32)
SEARCH_DEPTH = 9


def row_case(E, L):
    """(weights, codes [777], seqs [777, L]) of the row-forward tests: 20 % pads, row 5 an all-pad history, row 9 a -1 item.  The
    cases of B = 1 and 17 are the first rows of the same batch."""
    rng = np.random.default_rng(1000 * E + L)
    w = random_deepfm_weights(rng, E, L, ROW_NUM_INDEX)
    B = max(ROW_B)
    codes = rng.integers(0, ROW_NUM_INDEX, B).astype(np.int32)
    seqs = rng.integers(0, ROW_NUM_INDEX, (B, L)).astype(np.int32)
    seqs[rng.random((B, L)) < 0.2] = -1
    seqs[5] = -1
    codes[9] = -1
    return w, codes, seqs


SEARCH_U = 33


def search_case(E, L):
    """(tree, weights, seqs [33, L] item ids) of the search tests: helpers.synthetic_tree of depth 9 with missing nodes (389 of 512
    leaves), histories with prefix padding and 5 % unknown ids, user 1 all padding, user 2 with ancestor ids in the history."""
    from helpers import random_histories, synthetic_tree
    tree = synthetic_tree(np.random.default_rng(77), SEARCH_DEPTH, 389)
    rng = np.random.default_rng(7000 + 100 * E + L)
    w = random_deepfm_weights(rng, E, L, (1 << (SEARCH_DEPTH + 1)) - 1)
    seqs = random_histories(rng, tree["leaf_ids"], SEARCH_U, L, unknown_prob=0.05)
    seqs[1] = 0
    off = int(tree["leaf_ids"].max()) + 1
    seqs[2, -1] = off + 37                                       # an ancestor's id (TDMTree.scala:47-54): code 37
    return tree, w, seqs


def history_codes(tree, seqs):
    """TDMTree.idToCode without a mask: 0 / unknown -> -1 (a zero row); ids at or past nonLeafOffset are code + offset."""
    off, max_code = int(tree["leaf_ids"].max()) + 1, int(tree["leaf_codes"].max())
    lut = {int(i): int(c) for i, c in zip(tree["leaf_ids"], tree["leaf_codes"])}

    def one(i):
        i = int(i)
        if i == 0:
            return -1
        if i in lut:
            return lut[i]
        return i - off if 0 <= i - off <= max_code else -1
    return np.array([[one(i) for i in row] for row in np.atleast_2d(seqs)], np.int32)
