"""numpy restatement of one training step of the DeepFM scorer (dismember_amd/csrc/dfm_train.hip.inc; reference:
tdm/.../optim/LocalOptimizer.scala:139-162 with the graph of tdm/.../model/DeepFM.scala:11-45, useMask = false), dense Adam, and the
batches tests/test_gpu_deepfm_train.py runs.  Test infrastructure only; the forward is tests/deepfm_ref.py's, restated so that the
intermediates are at hand.

  X[r]   = [emb[code] ; emb[seq_0] ; .. ; emb[seq_{L-1}]]          x_i = feature block i, i < T = L + 1; id -1 = a zero row
  buf    = sum_i x_i          fm = (|buf|^2 - sum_i |x_i|^2) / 2
  zpre   = l1.W vec(X) + l1.b     h = relu(zpre)     z = fm + l2.W.h + l2.b
  loss   = mean_r( max(z,0) - z y + log1p(exp(-|z|)) )              g_r = (sigmoid(z_r) - y_r) / B
  dh     = g_r l2.W [zpre > 0]
  g_l2b  = sum_r g_r     g_l2W = sum_r g_r h[r]     g_l1b = sum_r dh[r]     g_l1W = sum_r dh[r] (x) vec(X[r])
  dX_i[r]= (dh[r] l1.W)_block i + g_r (buf[r] - x_i[r])             g_emb[row] += dX_i[r] for every slot (r, i) that read `row`

Beside the gradient g, step() returns A: the same accumulation over ABSOLUTE values — the magnitude an element's rounding error scales
with, whatever cancels in g.  The logit's own accumulated magnitude A_z (|fm|'s is (|buf|^2 + sum |x|^2) / 2, a unit's is
|l1.W| |vec(X)| + |l1.b|) reaches every gradient through sigma' <= 1/4: wherever g uses g_r, A uses |g_r| + A_z[r] / (4 B).  An element
with A == 0 received nothing but exact zeros.
"""
import functools

import numpy as np

import deepfm_ref as R

TENSORS = ("emb", "l1.W", "l1.b", "l2.W", "l2.b")
EPS32 = 2.0 ** -24
MARGIN = 64 * EPS32            # rows whose nearest pre-activation is closer to the ReLU's kink than this are redrawn
MAX_REDRAWN = 0.03
MAX_ROUNDS = 4


def sections(E, L, NI):
    o = R.deepfm_offsets(E, L, NI)
    return {"emb": (o["emb"], o["l1_w"]), "l1.W": (o["l1_w"], o["l1_b"]), "l1.b": (o["l1_b"], o["l2_w"]), "l2.W": (o["l2_w"], o["l2_b"]),
            "l2.b": (o["l2_b"], o["end"])}


def _scatter_rows(dst, idx, vals):
    """dst[idx[i]] += vals[i], duplicates summed in slot order (entries with idx < 0 dropped)"""
    keep = idx >= 0
    idx, vals = idx[keep], vals[keep]
    if idx.size == 0:
        return
    order = np.argsort(idx, kind="stable")
    idx, vals = idx[order], vals[order]
    starts = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
    dst[idx[starts]] += np.add.reduceat(vals, starts, axis=0)


def step(w, E, L, NI, codes, seqs, y, dtype=np.float64, reverse=False, loss_only=False):
    """-> dict(loss, z [B], g, A, A_loss, relu_margin [B]); g, A in the compact layout of deepfm_ref.  dtype: the arithmetic type of
    every intermediate of g and loss (A is always float64).  reverse: the batch sums run over the rows last to first."""
    dt = np.dtype(dtype).type
    emb, W1, b1, w2, b2 = R.split(w, E, L, NI, dt)
    codes = np.asarray(codes, np.int64).ravel()
    B, T = codes.size, L + 1
    idx = np.concatenate([codes[:, None], np.asarray(seqs, np.int64).reshape(B, L)], axis=1)
    y = np.asarray(y).astype(dt).ravel()
    if reverse:
        idx, y = idx[::-1], y[::-1]
    X = R.lookup(emb, idx)                                        # [B, T, E]
    buf = np.zeros((B, E), dt)
    for i in range(T):
        buf = buf + X[:, i, :]
    Xf = X.reshape(B, T * E)
    fm = ((buf * buf).sum(-1, dtype=dt) - (Xf * Xf).sum(-1, dtype=dt)) / dt(2)
    zpre = Xf @ W1.T + b1
    h = np.maximum(zpre, dt(0))
    z = fm + (h @ w2 + b2)
    ez = np.exp(-np.abs(z))
    lrow = (np.maximum(z, dt(0)) - z * y) + np.log1p(ez)
    loss = float(lrow.sum(dtype=dt) / dt(B))
    # magnitudes (float64)
    aX = np.abs(Xf).astype(np.float64)
    aW1, aw2 = np.abs(W1).astype(np.float64), np.abs(w2).astype(np.float64)
    A_zpre = aX @ aW1.T + np.abs(b1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(A_zpre > 0, np.abs(zpre).astype(np.float64) / A_zpre, np.inf).min(axis=1)
    act = zpre > 0
    A_fm = ((buf.astype(np.float64) ** 2).sum(-1) + (aX ** 2).sum(-1)) / 2
    A_h = A_zpre * act
    A_z = A_fm + A_h @ aw2 + abs(float(b2))
    A_loss = float((np.abs(np.maximum(z, 0)).astype(np.float64) + np.abs(z * y).astype(np.float64) + np.log1p(ez).astype(np.float64) + A_z).sum() / B)
    out = dict(loss=loss, z=z[::-1] if reverse else z, A_loss=A_loss, relu_margin=margin[::-1] if reverse else margin)
    if loss_only:
        return out
    sig = np.where(z >= 0, dt(1) / (dt(1) + ez), ez / (dt(1) + ez)).astype(dt)
    gr = (sig - y) / dt(B)
    Ag = np.abs(gr).astype(np.float64) + A_z / (4.0 * B)
    dh = (gr[:, None] * w2[None, :] * act).astype(dt)
    A_dh = Ag[:, None] * aw2[None, :] * act
    dX = ((dh @ W1).reshape(B, T, E) + gr[:, None, None] * (buf[:, None, :] - X)).astype(dt)
    abuf = np.abs(X).astype(np.float64).sum(1)
    A_dX = (A_dh @ aW1).reshape(B, T, E) + Ag[:, None, None] * (abuf[:, None, :] + np.abs(X).astype(np.float64))
    sec = sections(E, L, NI)
    g, A = np.zeros(sec["l2.b"][1], dt), np.zeros(sec["l2.b"][1], np.float64)
    view = lambda v, name, shape: v[slice(*sec[name])].reshape(shape)
    _scatter_rows(view(g, "emb", (NI, E)), idx.reshape(-1), dX.reshape(-1, E))
    _scatter_rows(view(A, "emb", (NI, E)), idx.reshape(-1), A_dX.reshape(-1, E))
    view(g, "l1.W", (T, T * E))[...] = dh.T @ Xf
    view(A, "l1.W", (T, T * E))[...] = A_dh.T @ aX
    view(g, "l1.b", T)[...] = dh.sum(0, dtype=dt)
    view(A, "l1.b", T)[...] = A_dh.sum(0)
    view(g, "l2.W", T)[...] = gr @ h
    view(A, "l2.W", T)[...] = Ag @ A_h
    view(g, "l2.b", 1)[...] = gr.sum(dtype=dt)
    view(A, "l2.b", 1)[...] = Ag.sum()
    out.update(g=g, A=A)
    return out


def ratios(got, ref, A, E, L, NI):
    """per tensor class the worst |got - ref| / (eps32 A) over the elements with A > 0; elements with A == 0 must be exact zeros"""
    out = {}
    for name, (a, b) in sections(E, L, NI).items():
        d = np.abs(np.asarray(got[a:b], np.float64) - np.asarray(ref[a:b], np.float64))
        Aa = A[a:b]
        assert np.all(np.asarray(got[a:b])[Aa == 0] == 0), name + ": an element that received only exact zeros is not zero"
        out[name] = float((d[Aa > 0] / (EPS32 * Aa[Aa > 0])).max()) if (Aa > 0).any() else 0.0
    return out


def adam_update(w, g, s, r, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, lr_decay=0.0, grad_scale=1.0):
    """dm_adam_elem's operations in w's type, in its order (epsilon after the square root, bias corrections in the step size);
    t: the time step AFTER this update (1 for the first).  Updates w, s, r in place."""
    T = w.dtype.type
    clr = lr / (1 + (t - 1) * lr_decay)
    stp = clr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    gi = g if grad_scale == 1.0 else g * T(grad_scale)
    s[:] = s * T(beta1) + T(1 - beta1) * gi
    r[:] = r * T(beta2) + T(1 - beta2) * (gi * gi)
    w += T(-stp) * (s / (np.sqrt(r) + T(eps)))


def train(w, E, L, NI, batches, lr, steps, dtype=np.float64):
    """dense Adam over `batches` [(codes, seqs, y)] (cycled) -> (weights, losses)"""
    w = np.asarray(w).astype(dtype).copy()
    s, r, losses = np.zeros_like(w), np.zeros_like(w), []
    for t in range(1, steps + 1):
        c, q, y = batches[(t - 1) % len(batches)]
        o = step(w, E, L, NI, c, q, y, dtype=dtype)
        losses.append(o["loss"])
        adam_update(w, o["g"].astype(dtype), s, r, t, lr)
    return w, np.array(losses)


# ---------------------------------------------------------------------------------------------------------------- the GPU cases
NUM_INDEX = 1023
# (E, L, B): one sweep per axis at the smallest values of the others, plus E = 128 x L in {10, 32} x B = 777.  L = 15 | 16 and 31 | 32
# are the column-tile boundaries of dfm_train_rows_kernel (ceil((L + 1) / 16) tiles of 16 units); B = 16 | 17 its row tile,
# 512 | 513 the slab of the l1.W product.
SWEEP_E = (16, 24, 64, 128)
SWEEP_L = (1, 10, 14, 15, 16, 30, 31, 32)
SWEEP_B = (1, 15, 16, 17, 511, 512, 513, 1025)
SHAPES = tuple(dict.fromkeys([(e, 1, 1) for e in SWEEP_E] + [(16, l, 1) for l in SWEEP_L] + [(16, 1, b) for b in SWEEP_B] +
                             [(128, 10, 777), (128, 32, 777)]))
GRID_CASE = (16, 1, 200)       # with DM_DFM_TRAIN_GRID=2: 13 tiles over 8 waves, a second, partial round
STRUCTURES = ("all_pad_history", "item_minus_one", "item_in_own_history", "identical_rows_513", "labels_all_0", "labels_all_1", "saturated_pos", "saturated_neg")


def _draw(rng, E, L, B, w):
    codes = rng.integers(0, NUM_INDEX, B).astype(np.int32)
    seqs = rng.integers(0, NUM_INDEX, (B, L)).astype(np.int32)
    seqs[rng.random((B, L)) < 0.2] = -1
    y = (rng.random(B) < 0.3).astype(np.float32)
    return codes, seqs, y


def _clean(rng, w, E, L, codes, seqs, y, pinned=()):
    """redraw the item code of every row too close to the ReLU's kink; -> the share of rows ever redrawn"""
    B = codes.size
    ever = np.zeros(B, bool)
    for rounds in range(MAX_ROUNDS + 1):
        bad = step(w, E, L, NUM_INDEX, codes, seqs, y, loss_only=True)["relu_margin"] < MARGIN
        if not bad.any():
            break
        assert rounds < MAX_ROUNDS, "more than %d rounds of redraws" % MAX_ROUNDS
        assert not any(bad[p] for p in pinned if p < B), "a row whose structure the case names sits on the kink: change the seed"
        ever |= bad
        codes[bad] = rng.integers(0, NUM_INDEX, int(bad.sum()))
    assert ever.mean() <= MAX_REDRAWN, "%d of %d rows redrawn" % (ever.sum(), B)
    return float(ever.mean())


@functools.lru_cache(maxsize=None)
def shape_case(E, L, B):
    """(weights, codes [B], seqs [B, L], y [B], redrawn share): 20 % pads, 30 % positives"""
    rng = np.random.default_rng(50000 + 1000 * E + 40 * L + B)
    w = R.random_deepfm_weights(rng, E, L, NUM_INDEX)
    codes, seqs, y = _draw(rng, E, L, B, w)
    share = _clean(rng, w, E, L, codes, seqs, y)
    return w, codes, seqs, y, share


@functools.lru_cache(maxsize=None)
def structure_case(name, E=16, L=10):
    """the batches that carry one named structure each (B = 40 unless the structure says otherwise)"""
    rng = np.random.default_rng(60000 + STRUCTURES.index(name))
    w = R.random_deepfm_weights(rng, E, L, NUM_INDEX)
    B = 513 if name == "identical_rows_513" else 40
    codes, seqs, y = _draw(rng, E, L, B, w)
    pinned = ()
    if name == "all_pad_history":
        seqs[3] = -1; seqs[17] = -1; pinned = (3, 17)
    elif name == "item_minus_one":
        codes[0] = -1; codes[16] = -1; seqs[16] = -1; pinned = (0, 16)          # row 16: nothing but zero rows
    elif name == "item_in_own_history":
        seqs[5, 2] = codes[5]; seqs[5, 7] = codes[5]; seqs[21, 0] = codes[21]; pinned = (5, 21)
    elif name == "identical_rows_513":
        codes[:] = codes[0]; seqs[:] = seqs[0]; seqs[:, 4] = codes[0]; pinned = tuple(range(B))
    elif name == "labels_all_0":
        y[:] = 0
    elif name == "labels_all_1":
        y[:] = 1
    elif name.startswith("saturated"):
        w = w.copy()
        w[-1] = 50.0 if name == "saturated_pos" else -50.0                      # l2.b: |z| > 40 in every row, sigmoid(z) rounds to 1 / to e^z
    if name == "identical_rows_513":
        assert step(w, E, L, NUM_INDEX, codes, seqs, y, loss_only=True)["relu_margin"].min() >= MARGIN
        share = 0.0
    else:
        share = _clean(rng, w, E, L, codes, seqs, y, pinned)
    return w, codes, seqs, y, share


# ---- a problem it learns: labels from a teacher DeepFM on a depth-9 tree's codes
LEARN = dict(E=16, L=10, depth=9, B=512, lr=0.01, steps=20)


@functools.lru_cache(maxsize=None)
def learning_case():
    """(initial weights, [batch], num_index): one batch of 512 rows labelled by a teacher's sign"""
    E, L, NI = LEARN["E"], LEARN["L"], (1 << (LEARN["depth"] + 1)) - 1
    rng = np.random.default_rng(4242)
    teacher = R.random_deepfm_weights(rng, E, L, NI, std=0.3)
    w0 = R.random_deepfm_weights(rng, E, L, NI)
    o = R.deepfm_offsets(E, L, NI)
    w0[o["l1_b"]:o["l2_w"]] = 0
    w0[o["l2_b"]] = 0
    codes = rng.integers(0, NI, LEARN["B"]).astype(np.int32)
    seqs = rng.integers(0, NI, (LEARN["B"], L)).astype(np.int32)
    seqs[rng.random(seqs.shape) < 0.2] = -1
    y = (R.forward(teacher, E, L, NI, codes, seqs) > 0).astype(np.float32)
    return w0, [(codes, seqs, y)], NI
