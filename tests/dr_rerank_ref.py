"""A numpy restatement of one training step of the Deep-Retrieval RERANK model (dismember_amd/csrc/dr_rerank_train.hip.inc; DESIGN.md
§11), its negative sampler, its full-softmax loss, and the batches tests/test_gpu_dr_rerank.py runs.  Test infrastructure only; written
from the formulas, fp64 unless told otherwise.

A batch is B samples (history seq[r][0..L) of internal ids, -1 = padding; target[r]); S negatives per row.
  X[r] = [rerank_emb[seq[r][j]], j < L]  (a padding id is a zero row without gradient);  U = X rerank_w^T + rerank_b   [B x E]
  item[r][0] = target[r];  item[r][1..S] = the row's negatives
  z[r][s] = softmax_w[item[r][s]] . U[r] + softmax_b[item[r][s]];  loss = -(1/B) sum_r log softmax(z[r])[0];  G = (softmax(z) - onehot_0) / B
  dU[r] = sum_s G[r][s] softmax_w[item[r][s]];  g_smw[item[r][s]] += G[r][s] U[r];  g_smb[item[r][s]] += G[r][s]
  dW = dU^T X;  db = sum_r dU[r];  dX = dU rerank_w;  demb[id] += the E-wide slices of dX that row id fed

Beside every gradient g[name], step() returns A[name]: the same accumulation over the ABSOLUTE values of every contribution, carried
through the chain (A_U = |X| |W|^T + |b| stands for U, A_dU = |G| |softmax_w[item]| for dU) — the magnitude an element's rounding error
scales with, whatever cancels in g (|G| is (p + onehot_0) / B: the target's p - 1 cancels when the softmax saturates).  An element with A == 0 received nothing but exact zeros.  A_loss is the loss's own: the mean over
the rows of (A of the target logit + the largest A of the row's logits + |the row's loss|).

The sampler (sample_row) restates drr_sample_kernel in Python integers:
  key(row) = splitmix(splitmix(seed ^ splitmix(step)) ^ row * 0xD6E8FEB86659FD93 mod 2^64)
  draw(c)  = splitmix(key(row) + c mod 2^64),  c = k * MAX_DRAWS + attempt
  id       = ((draw >> 32) * num_item) >> 32           the high 32 bits scaled to [0, num_item)
Negative k is the first of its MAX_DRAWS draws that is neither the target nor held; if none is free, the ids after the last draw are
probed upward, cyclically, S + 1 of them at most.  The row is written in ascending order.
"""
import functools
import zlib

import numpy as np

import cluster_ref
from dismember_amd import synth

EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP = {"f32": np.float32, "f64": np.float64}
TENSORS = ("rerank_emb", "rerank_w", "rerank_b", "softmax_w", "softmax_b")
CLASSES = TENSORS + ("loss", "full_loss")
M64 = (1 << 64) - 1
MAX_DRAWS = 32


# ------------------------------------------------------------------------------------------------------------------ the step
def _cast(w, dtype):
    return {k: np.asarray(w[k], dtype) for k in TENSORS}


def user_vectors(w, seq, L, E):
    """(ids [B, L], X [B, L E], U [B, E], A_U) in w's dtype"""
    ids = np.asarray(seq, np.int64).reshape(-1, L)
    emb = w["rerank_emb"]
    X = np.where(ids[..., None] >= 0, emb[np.maximum(ids, 0)], emb.dtype.type(0)).reshape(len(ids), L * E)
    U = X @ w["rerank_w"].T + w["rerank_b"]
    A_U = np.abs(X) @ np.abs(w["rerank_w"]).T + np.abs(w["rerank_b"])
    return ids, X, U, A_U


def softmax0(z):
    """rows of z [B, S+1], the target in slot 0 -> (mean loss, G, per-row losses)"""
    B = len(z)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    rows = (m[:, 0] + np.log(s[:, 0])) - z[:, 0]
    g = e / s
    g[:, 0] -= z.dtype.type(1)
    return rows.sum() / z.dtype.type(B), g / z.dtype.type(B), rows


def step(w, dims, seq, targets, negatives, dtype=np.float64, reverse=False, loss_only=False):
    """-> dict(loss, A_loss, g {name: array}, A {name: array}, U, z, items) in `dtype`.  reverse: the rows are visited last to first."""
    E, L, NI = dims
    T = np.dtype(dtype).type
    w = _cast(w, dtype)
    seq = np.asarray(seq, np.int64).reshape(-1, L)
    items = np.concatenate([np.asarray(targets, np.int64).reshape(-1, 1), np.asarray(negatives, np.int64).reshape(len(seq), -1)], axis=1)
    if reverse:
        seq, items = seq[::-1], items[::-1]
    B = len(seq)
    ids, X, U, A_U = user_vectors(w, seq, L, E)
    smw, smb = w["softmax_w"][items], w["softmax_b"][items]                    # [B, S+1, E], [B, S+1]
    z = np.einsum("bse,be->bs", smw, U) + smb
    A_z = np.einsum("bse,be->bs", np.abs(smw), A_U) + np.abs(smb)
    loss, G, rows = softmax0(z)
    A_loss = (A_z[:, 0] + A_z.max(axis=1) + np.abs(rows)).sum() / T(B)
    out = dict(loss=loss, A_loss=A_loss, U=U, z=z, items=items)
    if loss_only:
        return out
    aG = np.abs(G)
    aG[:, 0] = (G[:, 0] + T(1) / T(B)) + T(1) / T(B)       # slot 0 is (p - 1) / B: |p| / B + |1| / B, whatever cancels when p is near 1
    g = {k: np.zeros_like(w[k]) for k in TENSORS}
    A = {k: np.zeros_like(w[k]) for k in TENSORS}
    flat = items.ravel()
    np.add.at(g["softmax_w"], flat, (G[..., None] * U[:, None, :]).reshape(-1, E))       # unbuffered: one by one, in (row, slot) order
    np.add.at(A["softmax_w"], flat, (aG[..., None] * A_U[:, None, :]).reshape(-1, E))
    np.add.at(g["softmax_b"], flat, G.ravel())
    np.add.at(A["softmax_b"], flat, aG.ravel())
    dU = np.einsum("bs,bse->be", G, smw)
    A_dU = np.einsum("bs,bse->be", aG, np.abs(smw))
    g["rerank_w"][:] = dU.T @ X
    A["rerank_w"][:] = A_dU.T @ np.abs(X)
    g["rerank_b"][:] = dU.sum(axis=0)
    A["rerank_b"][:] = A_dU.sum(axis=0)
    dX, A_dX = (dU @ w["rerank_w"]).reshape(B, L, E), (A_dU @ np.abs(w["rerank_w"])).reshape(B, L, E)
    keep = ids >= 0
    np.add.at(g["rerank_emb"], ids[keep], dX[keep])
    np.add.at(A["rerank_emb"], ids[keep], A_dX[keep])
    out.update(g=g, A=A, dU=dU)
    return out


def full_loss(w, dims, seq, targets, dtype=np.float64, reverse=False):
    """Evaluator.evaluateReRankModel's fullEvaluate -> (loss, A_loss): the softmax over ALL items"""
    E, L, NI = dims
    T = np.dtype(dtype).type
    w = _cast(w, dtype)
    seq = np.asarray(seq, np.int64).reshape(-1, L)
    tg = np.asarray(targets, np.int64)
    if reverse:
        seq, tg = seq[::-1], tg[::-1]
    _, _, U, A_U = user_vectors(w, seq, L, E)
    z = U @ w["softmax_w"].T + w["softmax_b"]
    A_z = A_U @ np.abs(w["softmax_w"]).T + np.abs(w["softmax_b"])
    B = len(z)
    m = z.max(axis=1)
    rows = (m + np.log(np.exp(z - m[:, None]).sum(axis=1))) - z[np.arange(B), tg]
    return rows.sum() / T(B), (A_z[np.arange(B), tg] + A_z.max(axis=1) + np.abs(rows)).sum() / T(B)


def ratios(got, ref, eps):
    """per tensor: max |got - ref| / (eps A) over the elements with A > 0, and whether every element with A == 0 is exactly 0"""
    out, zeros_exact = {}, True
    for k in TENSORS:
        A = ref["A"][k].astype(np.float64)
        err = np.abs(np.asarray(got[k], ref["g"][k].dtype) - ref["g"][k]).astype(np.float64)
        live = A > 0
        out[k] = float((err[live] / (eps * A[live])).max()) if live.any() else 0.0
        zeros_exact = zeros_exact and bool((np.asarray(got[k])[~live] == 0).all())
    return out, zeros_exact


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_update(w, g, s, r, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, lr_decay=0.0, grad_scale=1.0):
    """dm_adam_elem's operations in w's type, in its order (epsilon after the square root, bias corrections in the step size);
    t: the time step AFTER this update (1 for the first).  Updates w, s, r in place."""
    T = w.dtype.type
    clr = lr / (1 + (t - 1) * lr_decay)
    step = clr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    gi = g if grad_scale == 1.0 else g * T(grad_scale)
    s[:] = s * T(beta1) + T(1 - beta1) * gi
    r[:] = r * T(beta2) + T(1 - beta2) * (gi * gi)
    w += T(-step) * (s / (np.sqrt(r) + T(eps)))


def train(w, dims, batches, lr, steps=None, accumulate=True, graph=True, softmax_eps=1e-7, graph_eps=1e-8, graph_decay=0.0, dtype=np.float64):
    """steps 1-8 over `batches` [(seq, targets, negatives)] (cycled for `steps` steps) -> (weights, losses).  graph=False moves the
    softmax tables only (the reference's SampledSoftmaxLossTest)."""
    E, L, NI = dims
    w = {k: v.copy() for k, v in _cast(w, dtype).items()}
    mom = {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in w.items()}
    acc = {k: np.zeros_like(w[k]) for k in ("softmax_w", "softmax_b")}
    losses = []
    for t in range(1, (steps or len(batches)) + 1):
        seq, tg, neg = batches[(t - 1) % len(batches)]
        r = step(w, dims, seq, tg, neg, dtype=dtype)
        losses.append(float(r["loss"]))
        for k in ("softmax_w", "softmax_b"):
            acc[k] = acc[k] + r["g"][k] if accumulate else r["g"][k]
            adam_update(w[k], acc[k], mom[k][0], mom[k][1], t, lr, eps=softmax_eps)
        if graph:
            for k in ("rerank_emb", "rerank_w", "rerank_b"):
                adam_update(w[k], r["g"][k], mom[k][0], mom[k][1], t, lr, eps=graph_eps, lr_decay=graph_decay)
    return w, np.array(losses)


# ------------------------------------------------------------------------------------------------------------------ the sampler
def sample_row(seed, step, row, target, S, N):
    """-> (the row's S negatives, ascending; how many of them came from the fallback)"""
    sm = cluster_ref.splitmix
    key = sm(sm((seed ^ sm(step & M64)) & M64) ^ ((row * 0xD6E8FEB86659FD93) & M64))
    held, fallbacks = [], 0
    for k in range(S):
        ok, c = False, 0
        for a in range(MAX_DRAWS):
            c = ((sm((key + k * MAX_DRAWS + a) & M64) >> 32) * N) >> 32
            if c != target and c not in held:
                ok = True
                break
        if not ok:
            fallbacks += 1
            for _ in range(S + 1):
                c = 0 if c + 1 >= N else c + 1
                if c != target and c not in held:
                    ok = True
                    break
        assert ok
        held.append(c)
    return sorted(held), fallbacks


@functools.lru_cache(maxsize=None)
def sample(seed, step, targets, S, N):
    """targets: a tuple -> (negatives [B, S] int32, total fallbacks)"""
    rows = [sample_row(seed, step, r, int(t), S, N) for r, t in enumerate(targets)]
    out = np.array([r[0] for r in rows], np.int32).reshape(len(targets), S)
    out.setflags(write=False)
    return out, sum(r[1] for r in rows)


# name: (num_item, S, B): B rows, targets cycling through all ids
SAMPLER_CASES = {"n64-s8": (64, 8, 32768), "n500-s250": (500, 250, 500), "n3-s1": (3, 1, 50)}
SAMPLER_SEEDS = (20240607, 3)


def sampler_targets(name):
    N, S, B = SAMPLER_CASES[name]
    return tuple(int(i % N) for i in range(B))


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_dr_rerank.py.  Sizes at which the kernels take another path, each met from below, at and above:
#   forward GEMM (dr_gemm_kernel): 128 rows, a 12-entry index cache per row (L = 13)
#   backward GEMMs (drt_gemm_kernel): 64 x 64 tiles in B, E, L E and L E + 1; the batch in slabs of 512 rows
#   sampled softmax: lanes in groups of E / 4 rounded up to a power of two (E = 48: 12 of 16 lanes live); 64 / group slots per pass; at
#     most 16 passes stay in registers (S + 1 = 64 at E = 48 and S + 1 = 256 at E = 16: 16 passes; S + 1 = 65 at E = 64: 17); E > 256
#     takes more than one window of 256 elements (E = 272); four slots per lane (S + 1 = 64, 65, 256)
#   segment sums: the 64-position look-ahead and the 4-way unrolled loop's remainder (one destination with 513 contributions)
NUM_ITEM = 500
SHAPES = {      # name: (E, L, B, S, kind)
    "tiny": (16, 1, 1, 1, "pad"),
    "b63": (16, 10, 63, 4, "pad"),
    "b64": (48, 1, 64, 4, "pad"),
    "b65-s63": (64, 10, 65, 63, "pad"),                      # S + 1 = 64
    "l13-s64": (16, 13, 65, 64, "pad"),                      # S + 1 = 65, one past the index cache
    "b511": (16, 1, 511, 1, "pad"),
    "b512-allpad": (16, 10, 512, 4, "allpad"),
    "b513-same": (128, 1, 513, 4, "same"),                   # every row the same history, target and negatives
    "b1025": (16, 10, 1025, 4, "pad"),
    "cap-255": (128, 10, 63, 255, "pad"),                    # S + 1 = 256, 128 passes
    "cap-255-e16": (16, 1, 65, 255, "pad"),                  # 16 passes: the last count that stays in registers
    "e48-s63": (48, 10, 64, 63, "rephist"),                  # 16 passes, 12 of 16 lanes; a history that repeats an item
    "e64-s64": (64, 1, 63, 64, "pad"),                       # 17 passes: the first count that is read twice
    "e128-negdup": (128, 13, 64, 4, "negdup"),               # a negative repeated inside a row
    "e128-s63": (128, 10, 65, 63, "pad"),
    "negtgt": (64, 10, 130, 4, "negtgt"),                    # negatives that are other rows' targets (and one that is its own row's)
    "e272": (272, 1, 5, 4, "pad"),                           # two windows of 256 elements
}
CASES = {"%s-%s" % (n, dt): s + (dt,) for n, s in SHAPES.items() for dt in ("f32", "f64")}


def make_batch(rng, L, B, S, kind, num_item=NUM_ITEM):
    seq = rng.integers(0, num_item, size=(B, L)).astype(np.int32)
    tg = rng.integers(0, num_item, size=B).astype(np.int32)
    neg = rng.integers(0, num_item, size=(B, S)).astype(np.int32)
    if kind in ("pad", "allpad", "negdup", "negtgt") and L > 1:
        seq[rng.random((B, L)) < 0.2] = -1
    if kind == "allpad":
        seq[B // 2, :] = -1
    if kind == "rephist":
        seq[:, 1] = seq[:, 0]
        seq[0, :] = seq[0, 0]
    if kind == "same":
        seq[:], tg[:], neg[:] = seq[0], tg[0], neg[0]
    if kind == "negdup":
        neg[:, 1] = neg[:, 0]
        neg[0, :] = neg[0, 0]
    if kind == "negtgt":
        neg[:, 0] = np.roll(tg, 1)
        neg[:, 1] = np.roll(tg, -3)
        neg[5, 2] = tg[5]
    return seq, tg, neg


@functools.lru_cache(maxsize=None)
def make_case(name):
    E, L, B, S, kind, dt = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.rsplit("-", 1)[0].encode()))        # the same draw for both dtypes
    wd = synth.make_dr_model(NUM_ITEM, 4, 2, L, E, rng, scale=0.3)
    wd = {k: ([np.asarray(a, NP[dt]).astype(np.float64) for a in v] if isinstance(v, list) else np.asarray(v, NP[dt]).astype(np.float64))
          for k, v in wd.items()}                                                     # the values the device holds
    seq, tg, neg = make_batch(rng, L, B, S, kind)
    for a in [seq, tg, neg] + [wd[k] for k in TENSORS]:
        a.setflags(write=False)
    return dict(dims=(E, L, NUM_ITEM), layer=(4, 2), B=B, S=S, kind=kind, dtype=dt, weights=wd, seq=seq, targets=tg, negatives=neg)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = make_case(name)
    return step(c["weights"], c["dims"], c["seq"], c["targets"], c["negatives"])


# full-softmax loss: rows of 500 classes live in the softmax kernel's registers, rows of 2049 are read again
FULL_CASES = {"n500-b1": (500, 1), "n500-b130": (500, 130), "n2049-b1": (2049, 1), "n2049-b130": (2049, 130)}


@functools.lru_cache(maxsize=None)
def make_full_case(name, dt):
    NI, B = FULL_CASES[name]
    E, L = 16, 4
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    wd = synth.make_dr_model(NI, 4, 2, L, E, rng, scale=0.3)
    wd = {k: ([np.asarray(a, NP[dt]).astype(np.float64) for a in v] if isinstance(v, list) else np.asarray(v, NP[dt]).astype(np.float64))
          for k, v in wd.items()}
    seq, tg, _ = make_batch(rng, L, B, 1, "pad", num_item=NI)
    return dict(dims=(E, L, NI), layer=(4, 2), weights=wd, seq=seq, targets=tg)


# a batch the model can learn: the target is the item after the last one of the history
def learning_problem(seed=5, L=4, E=16, num_item=64, B=256, S=8):
    rng = np.random.default_rng(seed)
    seqs = rng.integers(0, num_item, size=(B, L)).astype(np.int32)
    targets = ((seqs[:, -1] + 1) % num_item).astype(np.int32)
    wd = synth.make_dr_model(num_item, 4, 2, L, E, rng)
    from dismember_amd.dr_train import init_rerank_weights
    wd.update(init_rerank_weights(num_item, L, E, rng))
    return dict(dims=(E, L, num_item), layer=(4, 2), seqs=seqs, targets=targets, weights=wd, S=S, lr=1e-2, steps=40, sampler_seed=11, fraction=0.25)
