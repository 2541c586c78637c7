"""numpy restatement of the user-grouped DeepFM training step (dismember_amd/csrc/dfm_train_grouped.hip.inc) and the
batches tests/test_gpu_deepfm_train_grouped.py runs.  Test infrastructure only.  The reference of every check is the ROW step of
tests/deepfm_train_ref.py on the expanded rows; this file restates the regrouping, so that its float32 rounding can be measured on the
CPU (tests/golden/make_deepfm_train_grouped_tolerances.py) and so that named faults can be shown to leave the bound.

A batch is U histories seq[u][0..L) and R candidate rows per user (codes[u][r], y[u][r]); B = U R, W1_i = block i of l1.W:
  per user   bufh = sum_j x_j      sqh = sum_j |x_j|^2      Hh = sum_j x_j W1_{1+j}^T
  per row    zpre = Hh + x_c W1_0^T + l1.b    buf = bufh + x_c    fm = (|buf|^2 - sqh - |x_c|^2) / 2    h, z, loss, g_r, dh_r as the row step
             dXc_r = dh_r W1_0 + g_r bufh
  per user   DH = sum_r dh_r    Gs = sum_r g_r    GBc = sum_r g_r x_c,r    dXh_j = DH W1_{1+j} + (Gs bufh + GBc) - Gs x_j
  g_l1W      block 0 = sum_r dh_r (x) x_c,r     blocks 1 + j = sum_u DH_u (x) x_j,u     g_l1b = sum_r dh_r
  g_emb      scatters dXc (B slots) and dXh (U L slots) to the rows they read
"""
import functools

import numpy as np

import deepfm_ref as R
import deepfm_train_ref as T

NUM_INDEX = T.NUM_INDEX
FAULTS = ("drop_gs_x", "fm_without_candidate", "dh_row_left_out", "blocks_0_1_swapped", "hh_of_neighbour")


def expand(seq, codes, y):
    """the batch as the row step takes it: (codes [B], seqs [B, L], y [B]), user-major"""
    seq, codes = np.asarray(seq), np.asarray(codes)
    return codes.reshape(-1), np.repeat(seq, codes.shape[1], axis=0), np.asarray(y).reshape(-1)


def step_grouped(w, E, L, NI, seq, codes, y, dtype=np.float64, reverse=False, fault=None):
    """-> dict(loss, g): the algebra above in `dtype`; the per-user row sums (and the slot order of the scatter) run first to last, or
    last to first with reverse.  fault: one of FAULTS, a deliberately wrong step (tests: the bound sees it)."""
    dt = np.dtype(dtype).type
    emb, W1, b1, w2, b2 = R.split(w, E, L, NI, dt)
    seq = np.asarray(seq, np.int64)
    codes = np.asarray(codes, np.int64)
    U, Rr = codes.shape
    B, Tt = U * Rr, L + 1
    y = np.asarray(y).astype(dt).reshape(U, Rr)
    W1b = W1.reshape(Tt, Tt, E)                                   # [unit][block][E]
    W1c, W1h = W1b[:, 0, :], W1b[:, 1:, :].reshape(Tt, L * E)
    if fault == "blocks_0_1_swapped":
        W1s = W1b.copy(); W1s[:, 0, :] = W1b[:, 1, :]; W1s[:, 1, :] = W1b[:, 0, :]
        W1c, W1h = W1s[:, 0, :], W1s[:, 1:, :].reshape(Tt, L * E)
    Xh = R.lookup(emb, seq)                                       # [U, L, E]
    Xc = R.lookup(emb, codes)                                     # [U, R, E]
    bufh = np.zeros((U, E), dt)
    for j in range(L):
        bufh = bufh + Xh[:, j, :]
    Xhf = Xh.reshape(U, L * E)
    sqh = (Xhf * Xhf).sum(-1, dtype=dt)
    Hh = Xhf @ W1h.T                                              # [U, T]
    if fault == "hh_of_neighbour":
        Hh = np.roll(Hh, -1, axis=0)
    zpre = Hh[:, None, :] + Xc @ W1c.T + b1
    buf = bufh[:, None, :] + Xc
    if fault == "fm_without_candidate":
        fm = ((bufh * bufh).sum(-1, dtype=dt) - sqh)[:, None] / dt(2) + np.zeros((U, Rr), dt)
    else:
        fm = ((buf * buf).sum(-1, dtype=dt) - sqh[:, None] - (Xc * Xc).sum(-1, dtype=dt)) / dt(2)
    h = np.maximum(zpre, dt(0))
    z = fm + (h @ w2 + b2)
    ez = np.exp(-np.abs(z))
    lrow = (np.maximum(z, dt(0)) - z * y) + np.log1p(ez)
    order = range(Rr - 1, -1, -1) if reverse else range(Rr)
    loss = float((lrow.reshape(-1)[::-1] if reverse else lrow.reshape(-1)).sum(dtype=dt) / dt(B))
    sig = np.where(z >= 0, dt(1) / (dt(1) + ez), ez / (dt(1) + ez)).astype(dt)
    gr = ((sig - y) / dt(B)).astype(dt)                           # [U, R]
    dh = (gr[:, :, None] * w2[None, None, :] * (zpre > 0)).astype(dt)
    dXc = (dh @ W1c + gr[:, :, None] * bufh[:, None, :]).astype(dt)
    DH, Gs, GBc = np.zeros((U, Tt), dt), np.zeros(U, dt), np.zeros((U, E), dt)
    for r in order:
        if not (fault == "dh_row_left_out" and r == Rr - 1):
            DH = DH + dh[:, r, :]
        Gs = Gs + gr[:, r]
        GBc = GBc + gr[:, r, None] * Xc[:, r, :]
    base = Gs[:, None] * bufh + GBc
    dXh = (DH @ W1h).reshape(U, L, E) + base[:, None, :]
    if fault != "drop_gs_x":
        dXh = dXh - Gs[:, None, None] * Xh
    dXh = dXh.astype(dt)
    sec = T.sections(E, L, NI)
    g = np.zeros(sec["l2.b"][1], dt)
    view = lambda name, shape: g[slice(*sec[name])].reshape(shape)
    idx = np.concatenate([codes.reshape(-1), seq.reshape(-1)])
    vals = np.concatenate([dXc.reshape(B, E), dXh.reshape(U * L, E)])
    if reverse:
        idx, vals = idx[::-1], vals[::-1]
    T._scatter_rows(view("emb", (NI, E)), idx, vals)
    dhf, Xcf = dh.reshape(B, Tt), Xc.reshape(B, E)
    gw = view("l1.W", (Tt, Tt, E))
    gw[:, 0, :] = (dhf[::-1].T @ Xcf[::-1]) if reverse else dhf.T @ Xcf
    gw[:, 1:, :] = ((DH[::-1].T @ Xhf[::-1]) if reverse else DH.T @ Xhf).reshape(Tt, L, E)
    view("l1.b", Tt)[...] = (dhf[::-1] if reverse else dhf).sum(0, dtype=dt)
    grf, hf = gr.reshape(B), h.reshape(B, Tt)
    view("l2.W", Tt)[...] = (grf[::-1] @ hf[::-1]) if reverse else grf @ hf
    view("l2.b", 1)[...] = (grf[::-1] if reverse else grf).sum(dtype=dt)
    return dict(loss=loss, g=g, z=z)


def row_reference(w, E, L, seq, codes, y, **k):
    """deepfm_train_ref.step on the expanded rows"""
    c, s, yy = expand(seq, codes, y)
    return T.step(w, E, L, NUM_INDEX, c, s, yy, **k)


def fault_seen(w, E, L, seq, codes, y, fault, ref, bound):
    """does the float64 step with `fault` leave |g - ref| <= bound[tensor] eps32 A (or the loss its bound) somewhere?"""
    o = step_grouped(w, E, L, NUM_INDEX, seq, codes, y, fault=fault)
    for name, (a, b) in T.sections(E, L, NUM_INDEX).items():
        if (np.abs(o["g"][a:b] - ref["g"][a:b]) > bound[name] * T.EPS32 * ref["A"][a:b]).any():
            return True
    return abs(o["loss"] - ref["loss"]) > bound["loss"] * T.EPS32 * ref["A_loss"]


# ---------------------------------------------------------------------------------------------------------------- the cases
# (E, L, U, R): one sweep per axis at the smallest values of the others.  L = 15 | 16 and 31 | 32 are the column-tile boundaries; R = 16 | 17
# the row tile and a tile that straddles users, 513 the slab of the l1.W product over the rows; U = 16 | 17 the user tile, 513 the slab of
# the l1.W product over the users (two slabs, the second with one user).  One user cannot show a row that reads another user's Hh (or a
# wrong row / R), so the E, L and R sweeps are run a second time with two users
SWEEP_E = (16, 24, 64, 128)
SWEEP_L = (1, 10, 15, 16, 31, 32)
SWEEP_R = (1, 15, 16, 17, 40, 513)
SWEEP_U = (1, 15, 16, 17, 33, 513)
SHAPES = tuple(dict.fromkeys([(e, 1, u, 1) for u in (1, 2) for e in SWEEP_E] + [(16, l, u, 1) for u in (1, 2) for l in SWEEP_L] +
                             [(16, 1, u, r) for u in (1, 2) for r in SWEEP_R] + [(16, 1, u, 1) for u in SWEEP_U] +
                             [(128, 10, 19, 41), (128, 32, 19, 41)]))
GRID_CASE = (16, 1, 200, 3)    # with DM_DFM_TRAIN_GRID=2: 13 user tiles and 38 row tiles over 8 waves, a partial last round for both
STRUCTURES = ("all_pad_history", "user_codes_minus_one", "candidate_in_own_history", "identical_histories", "id_twice_in_history",
              "long_segment", "labels_all_0", "labels_all_1", "saturated_pos", "saturated_neg")
# a fault counts as visible to a case when it moves some element by more than this share of its magnitude A (the committed bounds are
# k eps32 A with k of the order of 100, i.e. below 1e-5 A): the generator keeps the first drawing that sees every fault it can see
VISIBLE = 2.0 ** -10
MAX_DRAWINGS = 16


def _draw(rng, E, L, U, Rr):
    codes = rng.integers(0, NUM_INDEX, (U, Rr)).astype(np.int32)
    seq = rng.integers(0, NUM_INDEX, (U, L)).astype(np.int32)
    seq[rng.random((U, L)) < 0.2] = -1
    y = (rng.random((U, Rr)) < 0.3).astype(np.float32)
    return seq, codes, y


def _clean(rng, w, E, L, seq, codes, y, pinned=None):
    """redraw the candidate of every row too close to the ReLU's kink (evaluated on the expanded rows); -> the share of rows ever redrawn"""
    B = codes.size
    ever = np.zeros(B, bool)
    flat = codes.reshape(-1)                                       # a view: redraws land in codes
    for rounds in range(T.MAX_ROUNDS + 1):
        bad = row_reference(w, E, L, seq, codes, y, loss_only=True)["relu_margin"] < T.MARGIN
        if not bad.any():
            break
        assert rounds < T.MAX_ROUNDS, "more than %d rounds of redraws" % T.MAX_ROUNDS
        assert pinned is None or not (bad & pinned.reshape(-1)).any(), "a row whose structure the case names sits on the kink: change the seed"
        ever |= bad
        flat[bad] = rng.integers(0, NUM_INDEX, int(bad.sum()))
    assert ever.mean() <= T.MAX_REDRAWN, "%d of %d rows redrawn" % (ever.sum(), B)
    return float(ever.mean())


def applicable_faults(U):
    """hh_of_neighbour is the identity for one user: a case with U = 1 cannot see it, whatever it holds"""
    return tuple(f for f in FAULTS if not (f == "hh_of_neighbour" and U == 1))


def _sees_all(w, E, L, seq, codes, y):
    ref = row_reference(w, E, L, seq, codes, y)
    bound = dict.fromkeys(T.TENSORS + ("loss",), VISIBLE / T.EPS32)
    return all(fault_seen(w, E, L, seq, codes, y, f, ref, bound) for f in applicable_faults(codes.shape[0]))


@functools.lru_cache(maxsize=None)
def shape_case(E, L, U, Rr):
    """(weights, seq [U, L], codes [U, R], y [U, R], redrawn share): 20 % pads, 30 % positives; the first drawing (of at most MAX_DRAWINGS
    seeds) that is clean within the caps and to which every applicable fault is visible"""
    for k in range(MAX_DRAWINGS):
        rng = np.random.default_rng(70000 + 100000 * k + 1000 * E + 40 * L + 7 * U + Rr)
        w = R.random_deepfm_weights(rng, E, L, NUM_INDEX)
        seq, codes, y = _draw(rng, E, L, U, Rr)
        try:
            share = _clean(rng, w, E, L, seq, codes, y)
        except AssertionError:
            continue
        if _sees_all(w, E, L, seq, codes, y):
            return w, seq, codes, y, share
    raise AssertionError("no drawing of %r is clean and sees every fault" % ((E, L, U, Rr),))


@functools.lru_cache(maxsize=None)
def structure_case(name, E=16, L=10):
    """the batches that carry one named structure each (6 users x 7 rows unless the structure says otherwise)"""
    rng = np.random.default_rng(80000 + STRUCTURES.index(name))
    w = R.random_deepfm_weights(rng, E, L, NUM_INDEX)
    U, Rr = (3, 513) if name == "long_segment" else (6, 7)
    seq, codes, y = _draw(rng, E, L, U, Rr)
    pinned = np.zeros((U, Rr), bool)
    if name == "all_pad_history":
        seq[2] = -1
    elif name == "user_codes_minus_one":
        codes[1] = -1; pinned[1] = True
    elif name == "candidate_in_own_history":
        seq[3, 2] = codes[3, 4]; seq[3, 8] = codes[3, 4]; pinned[3, 4] = True
    elif name == "identical_histories":
        seq[4] = seq[0]
    elif name == "id_twice_in_history":
        seq[5, 1] = 77; seq[5, 6] = 77
    elif name == "long_segment":
        codes[:] = codes[0, 0]; pinned[:] = True
    elif name == "labels_all_0":
        y[:] = 0
    elif name == "labels_all_1":
        y[:] = 1
    elif name.startswith("saturated"):
        w = w.copy()
        w[-1] = 50.0 if name == "saturated_pos" else -50.0          # l2.b: |z| > 40 in every row
    share = _clean(rng, w, E, L, seq, codes, y, pinned)
    return w, seq, codes, y, share


@functools.lru_cache(maxsize=None)
def learning_case():
    """deepfm_train_ref.learning_case regrouped to 32 users x 16 rows: user u's rows take the history of the row case's row 16 u, and are
    labelled by the same teacher"""
    E, L, NI = T.LEARN["E"], T.LEARN["L"], (1 << (T.LEARN["depth"] + 1)) - 1
    rng = np.random.default_rng(4242)
    teacher = R.random_deepfm_weights(rng, E, L, NI, std=0.3)
    w0, batches, NI2 = T.learning_case()
    assert NI2 == NI
    codes, seqs, _ = batches[0]
    seq = np.ascontiguousarray(seqs[::16])
    codes = np.ascontiguousarray(codes.reshape(32, 16))
    c, s, _ = expand(seq, codes, np.zeros((32, 16), np.float32))
    y = (R.forward(teacher, E, L, NI, c, s) > 0).astype(np.float32).reshape(32, 16)
    return w0, (seq, codes, y), NI
