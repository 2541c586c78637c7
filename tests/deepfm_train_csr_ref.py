"""numpy restatement of the ragged (CSR) user-grouped DeepFM training step (dm_deepfm_train_forward_backward_csr_dev in
dismember_amd/csrc/dfm_train_grouped.hip.inc) and the batches tests/test_gpu_deepfm_train_csr.py runs.  Test
infrastructure only.  The reference of every check is the ROW step of tests/deepfm_train_ref.py on the expanded rows; this file restates
the regrouping of tests/deepfm_train_grouped_ref.py with a row count per user, so that its float32 rounding can be measured on the CPU
(tests/golden/make_deepfm_train_csr_tolerances.py) and so that named faults can be shown to leave the bound.

A batch is U histories seq[u][0..L), offsets row_off [U + 1] and B = row_off[U] candidate rows (codes[i], y[i]); rows
row_off[u] .. row_off[u + 1] are user u's.  The algebra is the grouped step's with sum_r over the user's own rows; a user without rows
reads as an all-pad history (the device never gathers it) and scatters nothing.
"""
import functools

import numpy as np

import deepfm_ref as R
import deepfm_train_ref as T
import deepfm_train_grouped_ref as G

NUM_INDEX = T.NUM_INDEX
# the grouped step's faults, and two that only a ragged batch can show
FAULTS = G.FAULTS + ("row_user_shifted", "last_row_of_user_dropped")


def offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def expand(seq, row_off, codes, y):
    """the batch as the row step takes it: (codes [B], seqs [B, L], y [B])"""
    cnt = np.diff(np.asarray(row_off, np.int64))
    return np.asarray(codes).reshape(-1), np.repeat(np.asarray(seq), cnt, axis=0), np.asarray(y).reshape(-1)


def step_csr(w, E, L, NI, seq, row_off, codes, y, dtype=np.float64, reverse=False, fault=None):
    """-> dict(loss, g, z): the grouped algebra in `dtype` over ragged users; every user's row sums (and the slot order of the scatter) run
    first to last, or last to first with reverse.  fault: one of FAULTS, a deliberately wrong step (tests: the bound sees it)."""
    dt = np.dtype(dtype).type
    emb, W1, b1, w2, b2 = R.split(w, E, L, NI, dt)
    row_off = np.asarray(row_off, np.int64)
    cnt = np.diff(row_off)
    U, B, Tt = cnt.size, int(row_off[-1]), L + 1
    assert row_off[0] == 0 and (cnt >= 0).all() and B >= 1
    seq = np.asarray(seq, np.int64).reshape(U, L).copy()
    seq[cnt == 0] = -1                                            # the history of a user without rows is never read
    codes = np.asarray(codes, np.int64).reshape(B)
    y = np.asarray(y).astype(dt).reshape(B)
    ru = np.repeat(np.arange(U), cnt)                             # row_user
    W1b = W1.reshape(Tt, Tt, E)
    W1c, W1h = W1b[:, 0, :], W1b[:, 1:, :].reshape(Tt, L * E)
    if fault == "blocks_0_1_swapped":
        W1s = W1b.copy(); W1s[:, 0, :] = W1b[:, 1, :]; W1s[:, 1, :] = W1b[:, 0, :]
        W1c, W1h = W1s[:, 0, :], W1s[:, 1:, :].reshape(Tt, L * E)
    Xh = R.lookup(emb, seq)                                       # [U, L, E]
    Xc = R.lookup(emb, codes)                                     # [B, E]
    bufh = np.zeros((U, E), dt)
    for j in range(L):
        bufh = bufh + Xh[:, j, :]
    Xhf = Xh.reshape(U, L * E)
    sqh = (Xhf * Xhf).sum(-1, dtype=dt)
    Hh = Xhf @ W1h.T                                              # [U, T]
    rh = ru                                                       # the user whose Hh a row starts from
    rall = ru                                                     # ... and whose Hh / bufh / sqh it reads
    if fault == "hh_of_neighbour":
        rh = (ru + 1) % U
    if fault == "row_user_shifted":
        pop = np.flatnonzero(cnt > 0)
        rall = ru.copy()
        rall[row_off[pop[1:]]] = pop[:-1]
        rh = rall
    zpre = Hh[rh] + Xc @ W1c.T + b1
    bh = bufh[rall]
    buf = bh + Xc
    if fault == "fm_without_candidate":
        fm = ((bh * bh).sum(-1, dtype=dt) - sqh[rall]) / dt(2)
    else:
        fm = ((buf * buf).sum(-1, dtype=dt) - sqh[rall] - (Xc * Xc).sum(-1, dtype=dt)) / dt(2)
    h = np.maximum(zpre, dt(0))
    z = fm + (h @ w2 + b2)
    ez = np.exp(-np.abs(z))
    lrow = (np.maximum(z, dt(0)) - z * y) + np.log1p(ez)
    loss = float((lrow[::-1] if reverse else lrow).sum(dtype=dt) / dt(B))
    sig = np.where(z >= 0, dt(1) / (dt(1) + ez), ez / (dt(1) + ez)).astype(dt)
    gr = ((sig - y) / dt(B)).astype(dt)                           # [B]
    dh = (gr[:, None] * w2[None, :] * (zpre > 0)).astype(dt)
    dXc = (dh @ W1c + gr[:, None] * bh).astype(dt)
    DH, Gs, GBc = np.zeros((U, Tt), dt), np.zeros(U, dt), np.zeros((U, E), dt)
    for q in range(int(cnt.max())):                               # every user's q-th row (from its end with reverse), users in parallel
        us = np.flatnonzero(cnt > q)
        rows = (row_off[us + 1] - 1 - q) if reverse else (row_off[us] + q)
        last = rows == row_off[us + 1] - 1
        keep_all = ~last if fault == "last_row_of_user_dropped" else np.ones(us.size, bool)
        keep_dh = keep_all & (~last if fault == "dh_row_left_out" else True)
        DH[us[keep_dh]] = DH[us[keep_dh]] + dh[rows[keep_dh]]
        Gs[us[keep_all]] = Gs[us[keep_all]] + gr[rows[keep_all]]
        GBc[us[keep_all]] = GBc[us[keep_all]] + gr[rows[keep_all], None] * Xc[rows[keep_all]]
    base = Gs[:, None] * bufh + GBc
    dXh = (DH @ W1h).reshape(U, L, E) + base[:, None, :]
    if fault != "drop_gs_x":
        dXh = dXh - Gs[:, None, None] * Xh
    dXh = dXh.astype(dt)
    sec = T.sections(E, L, NI)
    g = np.zeros(sec["l2.b"][1], dt)
    view = lambda name, shape: g[slice(*sec[name])].reshape(shape)
    idx = np.concatenate([codes, seq.reshape(-1)])
    vals = np.concatenate([dXc, dXh.reshape(U * L, E)])
    if reverse:
        idx, vals = idx[::-1], vals[::-1]
    T._scatter_rows(view("emb", (NI, E)), idx, vals)
    gw = view("l1.W", (Tt, Tt, E))
    gw[:, 0, :] = (dh[::-1].T @ Xc[::-1]) if reverse else dh.T @ Xc
    gw[:, 1:, :] = ((DH[::-1].T @ Xhf[::-1]) if reverse else DH.T @ Xhf).reshape(Tt, L, E)
    view("l1.b", Tt)[...] = (dh[::-1] if reverse else dh).sum(0, dtype=dt)
    view("l2.W", Tt)[...] = (gr[::-1] @ h[::-1]) if reverse else gr @ h
    view("l2.b", 1)[...] = (gr[::-1] if reverse else gr).sum(dtype=dt)
    return dict(loss=loss, g=g, z=z)


def row_reference(w, E, L, seq, row_off, codes, y, **k):
    """deepfm_train_ref.step on the expanded rows"""
    c, s, yy = expand(seq, row_off, codes, y)
    return T.step(w, E, L, NUM_INDEX, c, s, yy, **k)


def fault_seen(w, E, L, seq, row_off, codes, y, fault, ref, bound):
    """does the float64 step with `fault` leave |g - ref| <= bound[tensor] eps32 A (or the loss its bound) somewhere?"""
    o = step_csr(w, E, L, NUM_INDEX, seq, row_off, codes, y, fault=fault)
    for name, (a, b) in T.sections(E, L, NUM_INDEX).items():
        if (np.abs(o["g"][a:b] - ref["g"][a:b]) > bound[name] * T.EPS32 * ref["A"][a:b]).any():
            return True
    return abs(o["loss"] - ref["loss"]) > bound["loss"] * T.EPS32 * ref["A_loss"]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _counts_1_3(n, seed):
    return tuple(int(v) for v in np.random.default_rng(seed).integers(1, 4, n))


def _counts_tdm(seed):
    c = [int(v) for v in np.random.default_rng(seed).choice([41, 47], 19)]
    c[0], c[1] = 41, 47                                           # both leaf levels, whatever the draw
    return tuple(c)


MIXED = (1, 16, 0, 17, 15, 0, 0, 2)
# name -> (E, L, rows per user).  Row tiles are 16 rows, user tiles 16 users, a slab of the l1.W products 512 rows / users
CASES = {
    "mixed8": (16, 1, MIXED),                                      # every row tile straddles users; empty users inside, none at the end
    "ends_empty": (16, 1, (0, 5, 0)),                              # the first and the last user have no rows
    "empty_tile": (16, 1, _counts_1_3(16, 1) + (0,) * 16 + _counts_1_3(16, 2)),      # the middle user tile is entirely empty
    "ones_then_513": (16, 1, (1,) * 16 + (513,)),                  # a row tile of 16 users; trip counts 1 and 513 in one user tile ...
    "single": (16, 1, (1,)),
    "only_last": (16, 1, (0,) * 16 + (3,)),                        # ... a second user tile whose only lane with rows is lane 0
    "u513": (16, 1, tuple(i % 4 for i in range(513))),             # two slabs of the users' product
    "tdm-E24-L15": (24, 15, _counts_tdm(3)),                       # the TDM shape: two leaf levels
    "tdm-E128-L10": (128, 10, _counts_tdm(4)),
    "tdm-E128-L32": (128, 32, _counts_tdm(5)),
    "grid200": (16, 1, MIXED * 25),                                # with DM_DFM_TRAIN_GRID=2: 13 user tiles and 80 row tiles over 8 waves
}
GRID_CASE = "grid200"
STRUCTURES = ("all_pad_history", "user_codes_minus_one", "candidate_in_own_history", "saturated_pos", "saturated_neg")
STRUCT_COUNTS = (7, 0, 5, 9, 3, 6, 0, 8)
VISIBLE = G.VISIBLE
MAX_DRAWINGS = G.MAX_DRAWINGS


def applicable_faults(counts):
    """hh_of_neighbour is the identity for one user; row_user_shifted moves nothing unless two users have rows (ends_empty, single and
    only_last have one populated user by construction)"""
    pop = sum(1 for c in counts if c > 0)
    return tuple(f for f in FAULTS if not (f == "hh_of_neighbour" and len(counts) == 1) and not (f == "row_user_shifted" and pop < 2))


def _draw(rng, E, L, counts):
    U, B = len(counts), int(sum(counts))
    codes = rng.integers(0, NUM_INDEX, B).astype(np.int32)
    seq = rng.integers(0, NUM_INDEX, (U, L)).astype(np.int32)
    seq[rng.random((U, L)) < 0.2] = -1
    y = (rng.random(B) < 0.3).astype(np.float32)
    return seq, offsets(counts), codes, y


def _clean(rng, w, E, L, seq, row_off, codes, y, pinned=None):
    """redraw the candidate of every row too close to the ReLU's kink (evaluated on the expanded rows); -> the share of rows ever redrawn"""
    B = codes.size
    ever = np.zeros(B, bool)
    for rounds in range(T.MAX_ROUNDS + 1):
        bad = row_reference(w, E, L, seq, row_off, codes, y, loss_only=True)["relu_margin"] < T.MARGIN
        if not bad.any():
            break
        assert rounds < T.MAX_ROUNDS, "more than %d rounds of redraws" % T.MAX_ROUNDS
        assert pinned is None or not (bad & pinned).any(), "a row whose structure the case names sits on the kink: change the seed"
        ever |= bad
        codes[bad] = rng.integers(0, NUM_INDEX, int(bad.sum()))
    assert ever.mean() <= T.MAX_REDRAWN, "%d of %d rows redrawn" % (ever.sum(), B)
    return float(ever.mean())


def _sees_all(w, E, L, seq, row_off, codes, y, counts):
    ref = row_reference(w, E, L, seq, row_off, codes, y)
    bound = dict.fromkeys(T.TENSORS + ("loss",), VISIBLE / T.EPS32)
    return all(fault_seen(w, E, L, seq, row_off, codes, y, f, ref, bound) for f in applicable_faults(counts))


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(weights, E, L, seq [U, L], row_off [U + 1], codes [B], y [B], redrawn share): 20 % pads, 30 % positives; the first drawing (of at
    most MAX_DRAWINGS seeds) that is clean within the caps and to which every applicable fault is visible"""
    E, L, counts = CASES[name]
    for k in range(MAX_DRAWINGS):
        rng = np.random.default_rng(90000 + 100000 * k + 1000 * list(CASES).index(name))
        w = R.random_deepfm_weights(rng, E, L, NUM_INDEX)
        seq, row_off, codes, y = _draw(rng, E, L, counts)
        try:
            share = _clean(rng, w, E, L, seq, row_off, codes, y)
        except AssertionError:
            continue
        if _sees_all(w, E, L, seq, row_off, codes, y, counts):
            return w, E, L, seq, row_off, codes, y, share
    raise AssertionError("no drawing of %r is clean and sees every fault" % (name,))


@functools.lru_cache(maxsize=None)
def structure_case(name, E=16, L=10):
    """the batches that carry one named structure each, on STRUCT_COUNTS rows per user (users 1 and 6 have none)"""
    rng = np.random.default_rng(95000 + STRUCTURES.index(name))
    w = R.random_deepfm_weights(rng, E, L, NUM_INDEX)
    seq, row_off, codes, y = _draw(rng, E, L, STRUCT_COUNTS)
    pinned = np.zeros(codes.size, bool)
    if name == "all_pad_history":
        seq[2] = -1
    elif name == "user_codes_minus_one":
        codes[row_off[3]:row_off[4]] = -1; pinned[row_off[3]:row_off[4]] = True
    elif name == "candidate_in_own_history":
        i = row_off[3] + 4
        seq[3, 2] = codes[i]; seq[3, 8] = codes[i]; pinned[i] = True
    elif name.startswith("saturated"):
        w = w.copy()
        w[-1] = 50.0 if name == "saturated_pos" else -50.0          # l2.b: |z| > 40 in every row
    share = _clean(rng, w, E, L, seq, row_off, codes, y, pinned)
    return w, E, L, seq, row_off, codes, y, share


def all_cases():
    """name -> (weights, E, L, seq, row_off, codes, y)"""
    out = {n: shape_case(n)[:7] for n in CASES}
    out.update({n: structure_case(n)[:7] for n in STRUCTURES})
    return out
