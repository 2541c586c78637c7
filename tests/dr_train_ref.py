"""A numpy restatement of one training step of the Deep-Retrieval LAYER model (dismember_amd/csrc/dr_train.hip.inc), and
the batches tests/test_gpu_dr_train.py runs.  Test infrastructure only; written from the formulas, fp64 unless told otherwise.

A batch is B rows (history seq[r][0..L) of internal ids, -1 = padding; path[r][0..D) of nodes).  Per layer d
  X_d[r] = [emb[seq[r][j]], j < L ; emb[num_item + t K + path[r][t]], t < d]      (a padding id is a zero row without gradient)
  Z_d = X_d W_d^T + b_d;  P_d = softmax rows;  loss_d = -(1/B) sum_r log P_d[r, path[r][d]];  G_d = (P_d - onehot(path[:, d])) / B
  dW_d = G_d^T X_d;  db_d = sum_r G_d[r];  dX_d = G_d W_d;  demb[id] += the E-wide slices of dX_d that row id fed
over the flat vector [emb ; W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}].

Beside the gradient g, step() returns A: the same accumulation over the ABSOLUTE values of every contribution (|G|^T |X| for dW, sum |G|
for db, |G| |W| for dX and, for an embedding row, the sum of the |G| |W| slices it collects) — the magnitude an element's rounding
error scales with, whatever cancels in g.  An element with A == 0 received nothing but exact zeros.  A_loss [D] is the loss's own:
the mean over the rows of (A of the target logit + the largest A of the row's logits + |the row's loss|).
"""
import functools
import zlib

import numpy as np

from dismember_amd import synth
from dismember_amd.dr_train import pack_params, param_sections

EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP = {"f32": np.float32, "f64": np.float64}
CLASSES = ("emb", "W", "b")            # the tensors a tolerance constant is kept for (plus "loss")


def tensor_class(name):
    return "emb" if name == "emb" else name[0]


def inputs(emb, seq, paths, d, num_item, K):
    """(ids [B, L+d], X_d [B, (L+d)E])"""
    ids = np.concatenate([seq] + [num_item + t * K + paths[:, t:t + 1] for t in range(d)], axis=1).astype(np.int64)
    rows = np.where(ids[..., None] >= 0, emb[np.maximum(ids, 0)], emb.dtype.type(0))
    return ids, rows.reshape(len(seq), -1)


def logits(w, dims, seq, paths, d, dtype=np.float64):
    """Z_d [B, K] in `dtype`"""
    E, L, K, D, NI = dims
    w = np.asarray(w, dtype)
    sec = param_sections(E, L, K, D, NI)
    emb = w[slice(*sec["emb"])].reshape(-1, E)
    _, X = inputs(emb, np.asarray(seq, np.int64), np.asarray(paths, np.int64), d, NI, K)
    return X @ w[slice(*sec["W%d" % d])].reshape(K, -1).T + w[slice(*sec["b%d" % d])]


def softmax_ce(z, targets):
    """rows of z [B, K], targets [B] (0-based) -> (mean of -log softmax(z)[target], its gradient [B, K], per-row losses)"""
    B = len(z)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    rows = (m[:, 0] + np.log(s[:, 0])) - z[np.arange(B), targets]
    g = e / s
    g[np.arange(B), targets] -= z.dtype.type(1)
    return rows.sum() / z.dtype.type(B), g / z.dtype.type(B), rows


def step(w, dims, seq, paths, dtype=np.float64, reverse=False, loss_only=False):
    """-> dict(loss [D], g, A, A_loss [D]) in `dtype`.  reverse: the rows are visited last to first (the same sums in another order)."""
    E, L, K, D, NI = dims
    T = np.dtype(dtype).type
    w = np.asarray(w, dtype)
    seq = np.asarray(seq, np.int64).reshape(-1, L)
    paths = np.asarray(paths, np.int64).reshape(-1, D)
    if reverse:
        seq, paths = seq[::-1], paths[::-1]
    B = len(seq)
    sec = param_sections(E, L, K, D, NI)
    emb = w[slice(*sec["emb"])].reshape(-1, E)
    g, A = np.zeros_like(w), np.zeros_like(w)
    g_emb, A_emb = g[slice(*sec["emb"])].reshape(-1, E), A[slice(*sec["emb"])].reshape(-1, E)
    loss, A_loss = np.zeros(D, dtype), np.zeros(D, dtype)
    for d in range(D):
        W = w[slice(*sec["W%d" % d])].reshape(K, -1)
        b = w[slice(*sec["b%d" % d])]
        ids, X = inputs(emb, seq, paths, d, NI, K)
        Z = X @ W.T + b
        loss[d], G, rows = softmax_ce(Z, paths[:, d])
        Az = np.abs(X) @ np.abs(W).T + np.abs(b)
        A_loss[d] = (Az[np.arange(B), paths[:, d]] + Az.max(axis=1) + np.abs(rows)).sum() / T(B)
        if loss_only:
            continue
        aG = np.abs(G)
        g[slice(*sec["W%d" % d])] = (G.T @ X).ravel()
        A[slice(*sec["W%d" % d])] = (aG.T @ np.abs(X)).ravel()
        g[slice(*sec["b%d" % d])] = G.sum(axis=0)
        A[slice(*sec["b%d" % d])] = aG.sum(axis=0)
        dX, adX = (G @ W).reshape(B, L + d, E), (aG @ np.abs(W)).reshape(B, L + d, E)
        keep = ids >= 0
        np.add.at(g_emb, ids[keep], dX[keep])              # unbuffered: duplicates are added one by one, in row order
        np.add.at(A_emb, ids[keep], adX[keep])
    return dict(loss=loss, g=g, A=A, A_loss=A_loss)


def class_ratios(got, ref, eps, dims):
    """per tensor class: max |got - ref| / (eps A) over the elements with A > 0, and whether every element with A == 0 is exactly 0"""
    E, L, K, D, NI = dims
    err = np.abs(np.asarray(got, ref["g"].dtype) - ref["g"]).astype(np.float64)
    A = ref["A"].astype(np.float64)
    out, zeros_exact = {c: 0.0 for c in CLASSES}, True
    for name, (a, b) in param_sections(E, L, K, D, NI).items():
        live = A[a:b] > 0
        if live.any():
            c = tensor_class(name)
            out[c] = max(out[c], float((err[a:b][live] / (eps * A[a:b][live])).max()))
        zeros_exact = zeros_exact and bool((np.asarray(got)[a:b][~live] == 0).all())
    return out, zeros_exact


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_dr_train.py (G1).  Tile and slab sizes of the kernels, each met from below, at and above:
#   forward GEMM (dr_gemm_kernel): 128 rows x 128 nodes, a 12-entry index cache per row (L + d = 13 at L = 10, D = 4)
#   backward GEMMs (drt_gemm_kernel): 64 x 64 tiles in B, K, L E, d E and (L + d) E + 1; the batch in slabs of 512 rows
#   softmax: rows of up to 1024 nodes live in registers, longer ones are read again; 4 rows per workgroup, at most 1024 workgroups
NUM_ITEM = 500
SHAPES = {      # name: (K, D, L, E, B, kind)
    "tiny": (7, 2, 1, 16, 1, "pad"),
    "one-node": (1, 3, 4, 16, 2, "pad"),                    # K = 1: P = 1, the gradient is exactly zero
    "all-pad-row": (100, 3, 4, 16, 127, "allpad"),          # (L + d) E = 64, 80, 96
    "cache-13": (129, 4, 10, 16, 128, "pad"),               # L + d = 13
    "no-pad": (64, 2, 4, 32, 129, "nopad"),
    "same-row": (63, 3, 1, 128, 300, "same"),               # every row names the same item and the same path
    "below-tile": (65, 3, 3, 16, 63, "pad"),                # (L + d) E = 48, 64, 80
    "at-tile": (128, 2, 10, 16, 64, "pad"),
    "above-tile": (127, 2, 4, 16, 65, "pad"),
    "slab-511": (7, 2, 4, 16, 511, "pad"),
    "slab-512": (7, 2, 4, 16, 512, "pad"),
    "slab-513": (7, 2, 4, 16, 513, "pad"),
    "row-1023": (1023, 2, 1, 16, 2, "pad"),
    "row-1024": (1024, 2, 1, 16, 2, "pad"),
    "row-1025": (1025, 2, 1, 16, 3, "pad"),
    "grid-4096": (7, 2, 1, 16, 4096, "pad"),                # 1024 workgroups of 4 rows: the last batch every wave sees one row of
    "grid-4097": (7, 2, 1, 16, 4097, "pad"),
    "c5-like": (100, 4, 10, 128, 129, "pad"),
}
CASES = {"%s-%s" % (n, dt): s + (dt,) for n, s in SHAPES.items() for dt in ("f32", "f64")}


def make_batch(rng, K, D, L, B, kind, num_item=NUM_ITEM):
    seq = rng.integers(0, num_item, size=(B, L)).astype(np.int32)
    paths = rng.integers(0, K, size=(B, D)).astype(np.int32)
    if kind in ("pad", "allpad"):
        seq[rng.random((B, L)) < 0.2] = -1
    if kind == "allpad":
        seq[B // 2, :] = -1
    if kind == "same":
        seq[:] = seq[0, 0]
        paths[:] = paths[0]
    return seq, paths


@functools.lru_cache(maxsize=None)
def make_case(name):
    K, D, L, E, B, kind, dt = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.rsplit("-", 1)[0].encode()))        # the same draw for both dtypes
    wd = synth.make_dr_model(NUM_ITEM, K, D, L, E, rng, scale=0.3)
    w = pack_params(wd, NP[dt]).astype(np.float64)           # the values the device holds
    seq, paths = make_batch(rng, K, D, L, B, kind)
    for a in (w, seq, paths):
        a.setflags(write=False)
    return dict(dims=(E, L, K, D, NUM_ITEM), B=B, kind=kind, dtype=dt, w=w, seq=seq, paths=paths)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = make_case(name)
    r = step(c["w"], c["dims"], c["seq"], c["paths"])
    for v in r.values():
        v.setflags(write=False)
    return r


def touched_rows(c):
    """embedding rows the batch names: history ids and the node rows of positions t < D - 1"""
    E, L, K, D, NI = c["dims"]
    t = np.zeros(NI + K * (D - 1), bool)
    t[c["seq"][c["seq"] >= 0]] = True
    for p in range(D - 1):
        t[NI + p * K + c["paths"][:, p]] = True
    return t


def unpack(vec, dims):
    """the flat vector -> dr_load_model's dict (rerank arrays not included)"""
    from dismember_amd.dr_train import split_params
    return split_params(vec, *dims)


# G5: a batch the model can learn — items that share a path also share their histories' items
def learning_problem(seed=5, K=16, D=2, L=4, E=16, num_item=64, B=256):
    rng = np.random.default_rng(seed)
    item_paths = rng.integers(0, K, size=(num_item, 1, D)).astype(np.int32)
    code = item_paths[:, 0, 0] * K + item_paths[:, 0, 1]
    targets = rng.integers(0, num_item, B)
    seqs = np.empty((B, L), np.int32)
    for r, tg in enumerate(targets):
        seqs[r] = rng.choice(np.flatnonzero(code == code[tg]), L)
    wd = synth.make_dr_model(num_item, K, D, L, E, rng)          # (std 0.3: Adam moves a weight by about lr per step, whatever the gradient's size)
    return dict(dims=(E, L, K, D, num_item), item_paths=item_paths, seqs=seqs, targets=targets, weights=wd, lr=3e-3, steps=20)


def adam_reference(w, grads_fn, steps, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """dense Adam (bias-corrected step size, epsilon after the square root) -> per-step losses"""
    w = w.copy()
    s, r, out = np.zeros_like(w), np.zeros_like(w), []
    for t in range(1, steps + 1):
        loss, g = grads_fn(w)
        out.append(loss)
        s = beta1 * s + (1 - beta1) * g
        r = beta2 * r + (1 - beta2) * g * g
        w += -(lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)) * (s / (np.sqrt(r) + eps))
    return np.array(out)
