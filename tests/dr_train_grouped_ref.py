"""A numpy restatement of the SAMPLE-GROUPED training step of the Deep-Retrieval layer model (dismember_amd/csrc/dr_train_grouped.hip.inc;
DESIGN.md §24), and the batches tests/test_gpu_dr_train_grouped.py runs.  Test infrastructure only; written from the formulas.

A batch is S samples (history seq[s][0..L), -1 = padding) with J paths each, paths[s][j][0..D); row r = s J + j, R = S J.  With Wh_d the
first L E columns of W_d and Wn_d the rest, Xs the gathered histories and Xn_d[r] the d node rows of path r:
  H_d[s] = Xs[s] Wh_d^T + b_d;  Z_d[r] = H_d[s(r)] + Xn_d[r] Wn_d^T  (d >= 1; Z_0 is H_0, the same for a sample's J rows)
  G_d = (softmax(Z_d) - onehot) / R  (d >= 1);  Gs_d[s] = sum_j G_d[sJ + j];  Gs_0[s] = (J softmax(H_0[s]) - sum_j onehot) / R
  dW_d[:, :LE] = Gs_d^T Xs;  db_d = sum_s Gs_d[s];  dW_d[:, LE:] = G_d^T Xn_d;  dXh = sum_d Gs_d Wh_d;  dXn = sum_d G_d Wn_d (d = D-1 first)
  demb[id] += the E-wide slices: the S L history slots first, then the R (D-1) node slots
This is tests/dr_train_ref.py's step on the expanded batch (np.repeat(seq, J), paths.reshape(-1, D)), re-associated: the yardstick of
every comparison stays THAT restatement (reference(), with its A), this one shows the algebra and measures what re-association costs."""
import functools
import zlib

import numpy as np

import dr_train_ref as R
from dismember_amd import synth
from dismember_amd.dr_train import pack_params, param_sections

EPS, NP, CLASSES = R.EPS, R.NP, R.CLASSES
NUM_ITEM = R.NUM_ITEM


def expand(seq, paths):
    """[S, L], [S, J, D] -> the row batch ([S J, L], [S J, D])"""
    S, J, D = paths.shape
    return np.repeat(seq, J, axis=0), paths.reshape(S * J, D)


def step(w, dims, seq, paths, dtype=np.float64, reverse_samples=False, reverse_paths=False, loss_only=False):
    """-> dict(loss [D], g) in `dtype`.  reverse_samples / reverse_paths: the samples, and the J paths of a sample, are visited last to
    first (the same sums in another order)."""
    E, L, K, D, NI = dims
    T = np.dtype(dtype).type
    w = np.asarray(w, dtype)
    seq = np.asarray(seq, np.int64).reshape(-1, L)
    S = len(seq)
    paths = np.asarray(paths, np.int64).reshape(S, -1, D)
    if reverse_samples:
        seq, paths = seq[::-1], paths[::-1]
    if reverse_paths:
        paths = paths[:, ::-1]
    J = paths.shape[1]
    Rn, LE = S * J, L * E
    rows = paths.reshape(Rn, D)
    sec = param_sections(E, L, K, D, NI)
    emb = w[slice(*sec["emb"])].reshape(-1, E)
    g = np.zeros_like(w)
    g_emb = g[slice(*sec["emb"])].reshape(-1, E)
    loss = np.zeros(D, dtype)
    ids_s, Xs = R.inputs(emb, seq, rows[:S], 0, NI, K)
    dXh = np.zeros((S, LE), dtype)
    dXn = np.zeros((Rn, (D - 1) * E), dtype)
    for d in range(D - 1, -1, -1):
        W = w[slice(*sec["W%d" % d])].reshape(K, -1)
        Wh, Wn, b = W[:, :LE], W[:, LE:], w[slice(*sec["b%d" % d])]
        H = Xs @ Wh.T + b
        tg = paths[:, :, d]                                        # [S, J]
        if d == 0:
            m = H.max(axis=1, keepdims=True)
            e = np.exp(H - m)
            s = e.sum(axis=1, keepdims=True)
            lse = m[:, 0] + np.log(s[:, 0])
            rl = np.zeros(S, dtype)
            cnt = np.zeros_like(H)
            for j in range(J):
                rl += lse - H[np.arange(S), tg[:, j]]
                cnt[np.arange(S), tg[:, j]] += T(1)
            loss[d] = rl.sum() / T(Rn)
            Gs = (T(J) * (e / s) - cnt) / T(Rn)
            G = Xn = None
        else:
            ids_n = (NI + np.arange(d) * K + rows[:, :d]).astype(np.int64)
            Xn = emb[ids_n].reshape(Rn, d * E)
            Z = np.repeat(H, J, axis=0) + Xn @ Wn.T
            loss[d], G, _ = R.softmax_ce(Z, rows[:, d])
            Gs = np.zeros_like(H)
            G3 = G.reshape(S, J, K)
            for j in range(J):
                Gs += G3[:, j]
        if loss_only:
            continue
        gW = g[slice(*sec["W%d" % d])].reshape(K, -1)
        gW[:, :LE] = Gs.T @ Xs
        g[slice(*sec["b%d" % d])] = Gs.sum(axis=0)
        dXh += Gs @ Wh
        if d:
            gW[:, LE:] = G.T @ Xn
            dXn[:, :d * E] += G @ Wn
    if not loss_only:
        keep = ids_s >= 0
        np.add.at(g_emb, ids_s[keep], dXh.reshape(S, L, E)[keep])
        if D > 1:
            ids_n = (NI + np.arange(D - 1) * K + rows[:, :D - 1]).astype(np.int64)
            np.add.at(g_emb, ids_n.ravel(), dXn.reshape(-1, E))
    return dict(loss=loss, g=g)


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_dr_train_grouped.py.  Tile and slab sizes, each met from below, at and above:
#   forward (dr_gemm_kernel): 128 rows, over S (history product) and over R (node products), a 12-entry index cache per row
#   backward (drt_gemm_kernel): 64-row tiles over S and R, slabs of 512 over S (history columns, bias) and over R (node columns)
#   softmax: rows of up to 1024 nodes live in registers, longer ones are read again; 4 samples per workgroup, at most 1024 workgroups
SHAPES = {      # name: (K, D, L, E, S, J, kind)
    "tiny": (7, 2, 1, 16, 1, 1, "pad"),
    "one-node": (1, 3, 4, 16, 2, 2, "pad"),                   # K = 1: P = 1, the gradient is exactly zero
    "j-1": (65, 3, 3, 16, 37, 1, "pad"),
    "j-2": (65, 3, 3, 16, 37, 2, "pad"),
    "j-3": (65, 3, 3, 16, 37, 3, "pad"),
    "j-5": (65, 3, 3, 16, 37, 5, "pad"),
    "dup-paths": (40, 3, 4, 16, 30, 3, "duppaths"),           # one sample's J paths are identical
    "same-sample": (63, 3, 1, 128, 100, 2, "same"),           # every sample names the same item and the same path
    "all-pad-sample": (100, 3, 4, 16, 67, 2, "allpad"),       # an all-padding history in the middle of the batch
    "s-63": (65, 3, 3, 16, 63, 2, "pad"),
    "s-64": (65, 3, 3, 16, 64, 2, "pad"),
    "s-65": (65, 3, 3, 16, 65, 2, "pad"),
    "slab-511": (7, 2, 4, 16, 511, 1, "pad"),
    "slab-512": (7, 2, 4, 16, 512, 1, "pad"),
    "slab-513": (7, 2, 4, 16, 513, 1, "pad"),
    "rows-513": (7, 3, 4, 16, 171, 3, "pad"),                 # R across the slab with S below it
    "rows-512": (7, 3, 4, 16, 256, 2, "pad"),
    "fwd-127": (64, 2, 4, 32, 127, 2, "nopad"),
    "fwd-129": (64, 2, 4, 32, 129, 2, "pad"),
    "row-1023": (1023, 2, 1, 16, 2, 2, "pad"),
    "row-1024": (1024, 2, 1, 16, 2, 2, "pad"),
    "row-1025": (1025, 2, 1, 16, 2, 2, "pad"),
    "cache-13": (129, 4, 10, 16, 40, 2, "pad"),               # L + D - 1 = 13 input positions
    "c5-like": (100, 4, 10, 128, 43, 3, "pad"),
    "grid-4096": (7, 2, 1, 16, 4096, 1, "pad"),               # 1024 workgroups of 4 samples
    "grid-4097": (7, 2, 1, 16, 4097, 1, "pad"),
}
CASES = {"%s-%s" % (n, dt): s + (dt,) for n, s in SHAPES.items() for dt in ("f32", "f64")}


def make_batch(rng, K, D, L, S, J, kind, num_item=NUM_ITEM):
    seq = rng.integers(0, num_item, size=(S, L)).astype(np.int32)
    paths = rng.integers(0, K, size=(S, J, D)).astype(np.int32)
    if kind in ("pad", "allpad", "duppaths"):
        seq[rng.random((S, L)) < 0.2] = -1
    if kind == "allpad":
        seq[S // 2, :] = -1
    if kind == "duppaths":
        paths[S // 2, :] = paths[S // 2, 0]
    if kind == "same":
        seq[:] = seq[0, 0]
        paths[:] = paths[0, 0]
    return seq, paths


@functools.lru_cache(maxsize=None)
def make_case(name):
    K, D, L, E, S, J, kind, dt = CASES[name]
    rng = np.random.default_rng(zlib.crc32(("grouped-" + name.rsplit("-", 1)[0]).encode()))        # the same draw for both dtypes
    wd = synth.make_dr_model(NUM_ITEM, K, D, L, E, rng, scale=0.3)
    w = pack_params(wd, NP[dt]).astype(np.float64)           # the values the device holds
    seq, paths = make_batch(rng, K, D, L, S, J, kind)
    for a in (w, seq, paths):
        a.setflags(write=False)
    return dict(dims=(E, L, K, D, NUM_ITEM), S=S, J=J, kind=kind, dtype=dt, w=w, seq=seq, paths=paths)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the ROW restatement on the expanded batch, fp64: loss, g, A, A_loss"""
    c = make_case(name)
    r = R.step(c["w"], c["dims"], *expand(c["seq"], c["paths"]))
    for v in r.values():
        v.setflags(write=False)
    return r


def loss_ratio(loss, ref, eps):
    """max over the layers of |loss - ref| / (eps A_loss)"""
    up = ref["loss"].dtype
    return float((np.abs(np.asarray(loss).astype(up) - ref["loss"]) / np.where(ref["A_loss"] > 0, eps * ref["A_loss"], 1.0)).max())
