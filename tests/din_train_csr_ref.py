"""numpy restatement of the ragged (CSR) user-grouped DIN training step (dm_train_forward_backward_csr_dev in
dismember_amd/csrc/train_grouped_csr.hip.inc) and the batches tests/test_gpu_din_train_csr.py runs.  Test infrastructure
only.  The reference of every check is the float64 ROW step of tests/train_ref.py on the expanded rows; this file restates the regrouping
in any float type, so that its float32 rounding can be measured on the CPU (tests/golden/make_din_train_csr_tolerances.py) and so that
named faults can be shown to leave the bound.

A batch is U histories seq[u][0..L) with a mask word each (bit j = position j masked; None = nothing masked), offsets row_off [U + 1] and
B = row_off[U] candidate rows (codes[i], y[i]); rows row_off[u] .. row_off[u + 1] are user u's.  Per user T_j = att.W k_j, G_j = W1b T_j;
per row the attention over the user's keys, z = W1a q + sum_j p_j G_j + b1; per user dG_j = sum_r p_j dz, dT_j = W1b^T dG_j,
dk_j = sum_r ds_j q + att.W^T dT_j (train_ref.py's header has the row formulas).  A user without rows reads as an all-pad history (the
device never gathers it) and scatters nothing.
"""
import functools

import numpy as np

import train_ref as R
from helpers import random_din_weights

NUM_INDEX = 1023
EPS32 = R.EPS["f32"]
MARGIN = 64 * EPS32                 # tests/test_train_host.py's threshold for an f32 case's relu_margin
VISIBLE = 2.0 ** -10                # a fault counts as visible where it moves an element by more than this times its A
MAX_DRAWINGS = 16
FAULTS = ("mask_ignored_in_ds", "g_of_previous_user", "last_row_of_user_dropped", "attT_dT_dropped", "dq_without_ds_k", "scale_of_padded_E")


def offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def padded_E(E):
    """the embed size the device computes with: the table is zero-padded to the next kernel instance"""
    return next(e for e in (16, 32, 64, 128) if e >= E)


def mask_bits(umask, U, L):
    """[U, L] bool from the mask words (None: nothing masked)"""
    if umask is None:
        return np.zeros((U, L), bool)
    return ((np.asarray(umask, np.uint32).reshape(U, 1) >> np.arange(L, dtype=np.uint32)[None, :]) & 1).astype(bool)


def pad_mask(seq):
    """the mask words the sampler gives with use_mask: every -1 position"""
    seq = np.asarray(seq)
    return ((seq == -1).astype(np.uint32) << np.arange(seq.shape[1], dtype=np.uint32)[None, :]).sum(1).astype(np.uint32)


def expand(seq, umask, row_off, codes, y):
    """the batch as the row step takes it: (codes [B], seqs [B, L], pad_flat, y [B])"""
    seq = np.asarray(seq)
    U, L = seq.shape
    cnt = np.diff(np.asarray(row_off, np.int64))
    seqs = np.repeat(seq, cnt, axis=0)
    masked = np.repeat(mask_bits(umask, U, L), cnt, axis=0)
    return np.asarray(codes).reshape(-1), seqs, np.flatnonzero(masked.reshape(-1)).astype(np.int32), np.asarray(y).reshape(-1)


def row_reference(w, E, L, seq, umask, row_off, codes, y):
    """train_ref.step (float64) on the expanded rows"""
    c, s, pad, yy = expand(seq, umask, row_off, codes, y)
    return R.step(w, E, L, NUM_INDEX, c, s, pad, yy)


def drop_rowless(seq, umask, row_off):
    """the same batch without its users that have no rows"""
    keep = np.diff(np.asarray(row_off, np.int64)) > 0
    return (np.ascontiguousarray(np.asarray(seq)[keep]), None if umask is None else np.ascontiguousarray(np.asarray(umask)[keep]),
            offsets(np.diff(row_off)[keep]))


def _lookup(emb, idx):
    idx = np.asarray(idx, np.int64)
    return np.where(idx[..., None] >= 0, emb[np.maximum(idx, 0)], emb.dtype.type(0))


def step_csr(w, E, L, NI, seq, umask, row_off, codes, y, dtype=np.float64, reverse=False, fault=None):
    """-> dict(loss, g): the grouped algebra in `dtype` over ragged users; every user's row sums, the contractions of the weight
    gradients and the slot order of the scatter run first to last, or last to first with reverse.  fault: one of FAULTS, a deliberately
    wrong step (tests: the bound sees it)."""
    assert fault is None or fault in FAULTS
    dt = np.dtype(dtype).type
    w = np.asarray(w).astype(dt)
    sec = R.sections(E, NI)
    emb = w[slice(*sec["table"])].reshape(NI, E)
    att = w[slice(*sec["att.W"])].reshape(E, E)
    W1 = w[slice(*sec["l1.W"])].reshape(E, 2 * E)
    W1a, W1b = W1[:, :E], W1[:, E:]
    b1, w2, b2 = w[slice(*sec["l1.b"])], w[slice(*sec["l2.W"])], w[sec["l2.b"][0]]
    row_off = np.asarray(row_off, np.int64)
    cnt = np.diff(row_off)
    U, B = cnt.size, int(row_off[-1])
    assert row_off[0] == 0 and (cnt >= 0).all() and B >= 1
    seq = np.asarray(seq, np.int64).reshape(U, L).copy()
    seq[cnt == 0] = -1                                            # the history of a user without rows is never read
    masked = mask_bits(umask, U, L)
    codes = np.asarray(codes, np.int64).reshape(B)
    y = np.asarray(y).astype(dt).reshape(B)
    ru = np.repeat(np.arange(U), cnt)                             # the user of a row
    rg = ru                                                       # ... and the user whose G it reads
    if fault == "g_of_previous_user":
        pop = np.flatnonzero(cnt > 0)
        rg = ru.copy()
        rg[row_off[pop[1:]]] = pop[:-1]
    sc = dt(1) / np.sqrt(dt(padded_E(E) if fault == "scale_of_padded_E" else E))
    K = _lookup(emb, seq)                                         # [U, L, E]
    Tm = K @ att.T
    G = Tm @ W1b.T
    q = _lookup(emb, codes)                                       # [B, E]
    mk = masked[ru]
    s = np.where(mk, dt(-R.FLT_MAX), np.einsum("be,ble->bl", q, K[ru]) * sc).astype(dt)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True, dtype=dt)).astype(dt)
    z = (q @ W1a.T + np.einsum("bl,ble->be", p, G[rg]) + b1).astype(dt)
    h = np.maximum(z, dt(0))
    x = (h @ w2 + b2).astype(dt)
    lrow = (np.maximum(x, dt(0)) + np.log1p(np.exp(-np.abs(x)))) - x * y
    loss = float((lrow[::-1] if reverse else lrow).sum(dtype=dt) / dt(B))
    gl = ((dt(1) / (dt(1) + np.exp(-x)) - y) / dt(B)).astype(dt)
    dz = ((z > 0) * gl[:, None] * w2[None, :]).astype(dt)
    dp = np.einsum("be,ble->bl", dz, G[rg]).astype(dt)
    ds = (p * (dp - (dp * p).sum(-1, keepdims=True, dtype=dt)) * sc).astype(dt)
    if fault != "mask_ignored_in_ds":
        ds = np.where(mk, dt(0), ds)
    dq = dz @ W1a
    if fault != "dq_without_ds_k":
        dq = dq + np.einsum("bl,ble->be", ds, K[ru])
    dq = dq.astype(dt)
    dG, dKs = np.zeros((U, L, E), dt), np.zeros((U, L, E), dt)
    for i in range(int(cnt.max())):                               # every user's i-th row (from its end with reverse), users in parallel
        us = np.flatnonzero(cnt > i)
        rows = (row_off[us + 1] - 1 - i) if reverse else (row_off[us] + i)
        if fault == "last_row_of_user_dropped":
            keep = rows != row_off[us + 1] - 1
            us, rows = us[keep], rows[keep]
        dG[us] = dG[us] + p[rows][:, :, None] * dz[rows][:, None, :]
        dKs[us] = dKs[us] + ds[rows][:, :, None] * q[rows][:, None, :]
    dT = (dG @ W1b).astype(dt)                                    # dT_j = W1b^T dG_j
    dk = dKs if fault == "attT_dT_dropped" else (dKs + dT @ att).astype(dt)
    g = np.zeros(sec["l2.b"][1], dt)
    view = lambda name, shape: g[slice(*sec[name])].reshape(shape)
    idx = np.concatenate([codes, seq.reshape(-1)])
    vals = np.concatenate([dq, dk.reshape(U * L, E)])
    flip = (lambda a: a[::-1]) if reverse else (lambda a: a)
    R._scatter_rows(view("table", (NI, E)), flip(idx), flip(vals))
    Kf, Tf, dGf, dTf = (a.reshape(U * L, E) for a in (K, Tm, dG, dT))
    view("att.W", (E, E))[...] = flip(dTf).T @ flip(Kf)
    gw = view("l1.W", (E, 2 * E))
    gw[:, :E] = flip(dz).T @ flip(q)
    gw[:, E:] = flip(dGf).T @ flip(Tf)
    view("l1.b", E)[...] = flip(dz).sum(0, dtype=dt)
    view("l2.W", E)[...] = flip(gl) @ flip(h)
    view("l2.b", 1)[...] = flip(gl).sum(dtype=dt)
    return dict(loss=loss, g=g)


def loss_bound(x):
    """tests/test_gpu_train_edges.py's bound of the loss"""
    return 1e-5 + 1e-4 * abs(x)


def fault_seen(case, fault, ref, k):
    """does the float64 step with `fault` leave |g - ref| <= k[tensor] eps32 A somewhere (or the loss its bound)?"""
    w, E, L, seq, umask, row_off, codes, y = case
    o = step_csr(w, E, L, NUM_INDEX, seq, umask, row_off, codes, y, fault=fault)
    scale = R.element_scale(ref["A"], E, NUM_INDEX)
    for name, (a, b) in R.sections(E, NUM_INDEX).items():
        if (np.abs(o["g"][a:b] - ref["g"][a:b]) > k[name] * EPS32 * scale[a:b]).any():
            return True
    return abs(o["loss"] - ref["loss"]) > loss_bound(ref["loss"])


# ---------------------------------------------------------------------------------------------------------------- the cases
def _counts_1_3(n, seed):
    return tuple(int(v) for v in np.random.default_rng(seed).integers(1, 4, n))


def _counts_tdm(seed):
    c = [int(v) for v in np.random.default_rng(seed).choice([41, 47], 19)]
    c[0], c[1] = 41, 47                                           # both leaf levels, whatever the draw
    return tuple(c)


MIXED = (1, 16, 0, 17, 15, 0, 0, 2)
# name -> (E, L, rows per user).  Row tiles are 16 rows of ONE user, a slab of the three products 512 rows / 32 users
CASES = {
    "mixed8": (16, 1, MIXED),                                      # full, over-full and partial tiles; empty users inside, none at the end
    "ends_empty": (16, 1, (0, 5, 0)),                              # the first and the last user have no rows
    "only_last": (16, 1, (0,) * 16 + (3,)),                        # 17 users of which only the last has rows
    "ones_then_513": (16, 1, (1,) * 16 + (513,)),                  # 16 one-row tiles, then 33 tiles of one user; two slabs of the rows' product
    "single": (16, 1, (1,)),
    "empty_tile": (16, 1, _counts_1_3(16, 1) + (0,) * 16 + _counts_1_3(16, 2)),      # the middle 16 users have no tile
    "E24-L15": (24, 15, MIXED),                                    # travels as E = 32; the softmax scale stays 1 / sqrt(24)
    "E32-L16": (32, 16, MIXED),                                    # every history position in use
    "E64-L10": (64, 10, MIXED),
    "tdm-E128-L10": (128, 10, _counts_tdm(4)),                     # the TDM shape: two leaf levels
    "tdm-E128-L16": (128, 16, _counts_tdm(5)),
    "grid200": (16, 1, MIXED * 25),                                # with DM_DIN_TRAIN_GRID=2: 200 users and 125 row tiles over 8 waves
}
GRID_CASE = "grid200"
STRUCTURES = ("all_pad_history", "all_masked_keys", "one_key_user", "user_codes_minus_one", "candidate_in_own_history", "id_twice_in_history", "unmasked_pads",
              "saturated_pos", "saturated_neg")
STRUCT_COUNTS = (7, 0, 5, 9, 3, 6, 0, 8)
STRUCT_E, STRUCT_L = 16, 10


def applicable_faults(E, seq, umask, row_off):
    """the faults a batch can show at all: the mask enters ds only where a masked position has p > 0 and a key, i.e. for a user with rows whose
    whole history is masked and not all padding; a previous populated user needs two; the key-side terms need a key that is not padding; ds itself is 0
    for a history of one position (its softmax is 1); the padded scale differs only where E is padded"""
    cnt = np.diff(row_off)
    pop = cnt > 0
    seq = np.asarray(seq)
    L = seq.shape[1]
    out = ["last_row_of_user_dropped"]
    if L >= 2 and umask is not None and (mask_bits(umask, *seq.shape).all(1) & (seq >= 0).any(1) & pop).any():
        out.append("mask_ignored_in_ds")
    if pop.sum() >= 2:
        out.append("g_of_previous_user")
    if (seq[pop] >= 0).any():
        out.append("attT_dT_dropped")
        if L >= 2:
            out.append("dq_without_ds_k")
            if padded_E(E) != E:
                out.append("scale_of_padded_E")
    return tuple(f for f in FAULTS if f in out)


def _draw(rng, E, L, counts):
    U, B = len(counts), int(sum(counts))
    codes = rng.integers(0, NUM_INDEX, B).astype(np.int32)
    seq = rng.integers(0, NUM_INDEX, (U, L)).astype(np.int32)
    seq[rng.random((U, L)) < 0.2] = -1
    y = (rng.random(B) < 0.3).astype(np.float32)
    return seq, offsets(counts), codes, y


def row_margins(w, E, L, seq, umask, row_off, codes):
    """train_ref.step's relu_margin per row (float64 forward of the expanded rows): min over units of |z| / (|l1.W| |[q ; a]| + |l1.b|)"""
    w = np.asarray(w, np.float64)
    sec = R.sections(E, NUM_INDEX)
    emb = w[slice(*sec["table"])].reshape(NUM_INDEX, E)
    att = w[slice(*sec["att.W"])].reshape(E, E)
    W1 = w[slice(*sec["l1.W"])].reshape(E, 2 * E)
    b1 = w[slice(*sec["l1.b"])]
    cd, sq, pad, _ = expand(seq, umask, row_off, codes, np.zeros(len(codes)))
    mk = np.zeros(sq.size, bool)
    mk[pad] = True
    q, k = _lookup(emb, cd), _lookup(emb, sq)
    s = np.where(mk.reshape(sq.shape), -R.FLT_MAX, np.einsum("be,ble->bl", q, k) / np.sqrt(float(E)))
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    qa = np.concatenate([q, np.einsum("bl,ble->be", p, k) @ att.T], -1)
    z = qa @ W1.T + b1
    zmag = np.abs(qa) @ np.abs(W1).T + np.abs(b1)
    return np.where(zmag > 0, np.abs(z) / np.where(zmag > 0, zmag, 1.0), np.inf).min(-1)


MAX_ROUNDS, MAX_REDRAWN = 8, 0.25


def _clean(rng, case, pinned=None):
    """redraw the candidate of every row too close to the ReLU's kink, as tests/deepfm_train_csr_ref.py does; False when a row whose
    structure the case names sits on the kink, or when the rounds or the share of redrawn rows run out"""
    w, E, L, seq, umask, row_off, codes, y = case
    ever = np.zeros(codes.size, bool)
    for rounds in range(MAX_ROUNDS + 1):
        bad = row_margins(w, E, L, seq, umask, row_off, codes) < MARGIN
        if not bad.any():
            return ever.mean() <= MAX_REDRAWN
        if rounds == MAX_ROUNDS or (pinned is not None and (bad & pinned).any()):
            return False
        ever |= bad
        codes[bad] = rng.integers(0, NUM_INDEX, int(bad.sum()))
    return False


def _accept(case):
    """the two conditions of a drawing: the margin from the ReLU's kink, and every applicable fault visible above VISIBLE A"""
    w, E, L, seq, umask, row_off, codes, y = case
    ref = row_reference(w, E, L, seq, umask, row_off, codes, y)
    if not ref["relu_margin"] >= MARGIN:
        return False
    k = dict.fromkeys(R.TENSORS, VISIBLE / EPS32)
    return all(fault_seen(case, f, ref, k) for f in applicable_faults(E, seq, umask, row_off))


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(weights, E, L, seq [U, L], umask [U], row_off [U + 1], codes [B], y [B]): 20 % pads, all of them masked (what the sampler gives
    with use_mask), 30 % positives, the candidates of rows too close to the ReLU's kink redrawn; the first drawing of at most
    MAX_DRAWINGS seeds that meets both conditions"""
    E, L, counts = CASES[name]
    for k in range(MAX_DRAWINGS):
        rng = np.random.default_rng(70000 + 100000 * k + 1000 * list(CASES).index(name))
        w = random_din_weights(rng, E, NUM_INDEX, std=0.2, bias_std=0.2)
        seq, row_off, codes, y = _draw(rng, E, L, counts)
        case = (w, E, L, seq, pad_mask(seq), row_off, codes, y)
        if _clean(rng, case) and _accept(case):
            return case
    raise AssertionError("no drawing of %r keeps the margin and sees every fault" % (name,))


@functools.lru_cache(maxsize=None)
def structure_case(name, with_mask):
    """the batches that carry one named structure each, on STRUCT_COUNTS rows per user (users 1 and 6 have none), with the pads masked
    or with no mask at all"""
    E, L = STRUCT_E, STRUCT_L
    for k in range(MAX_DRAWINGS):
        rng = np.random.default_rng(75000 + 100000 * k + 10 * STRUCTURES.index(name) + int(with_mask))
        w = random_din_weights(rng, E, NUM_INDEX, std=0.2, bias_std=0.2)
        seq, row_off, codes, y = _draw(rng, E, L, STRUCT_COUNTS)
        pinned = np.zeros(codes.size, bool)                             # rows whose candidate the structure names: never redrawn
        if name == "all_pad_history":
            seq[2] = -1
        elif name == "one_key_user":
            seq[2] = -1
            seq[2, L - 1] = rng.integers(0, NUM_INDEX)
        elif name == "user_codes_minus_one":
            codes[row_off[3]:row_off[4]] = -1
            pinned[row_off[3]:row_off[4]] = True
        elif name == "candidate_in_own_history":
            seq[3, 2] = seq[3, 8] = codes[row_off[3] + 4]
            pinned[row_off[3] + 4] = True
        elif name == "id_twice_in_history":
            seq[3, 1] = seq[3, 7] = rng.integers(0, NUM_INDEX)
        elif name.startswith("saturated"):
            w[-1] = 50.0 if name == "saturated_pos" else -50.0          # l2.b: |x| > 40 in every row
        umask = pad_mask(seq) if with_mask else None
        if name == "all_masked_keys" and umask is not None:
            assert (seq[4] >= 0).any()
            umask[4] = (1 << L) - 1                                     # the caller's mask covers real keys: p is uniform, ds stays 0
        if name == "unmasked_pads":
            seq[3, :4] = -1                                             # user 3's -1 entries take part in the softmax, masked or not
            if umask is not None:
                umask = pad_mask(seq)
                umask[3] = 0
        case = (w, E, L, seq, umask, row_off, codes, y)
        if _clean(rng, case, pinned) and _accept(case):
            return case
    raise AssertionError("no drawing of %r keeps the margin and sees every fault" % (name,))


def all_cases():
    """name -> (weights, E, L, seq, umask, row_off, codes, y)"""
    out = {n: shape_case(n) for n in CASES}
    for n in STRUCTURES:
        for m in (True, False):
            out["%s-%s" % (n, "masked" if m else "nomask")] = structure_case(n, m)
    return out
