"""A numpy restatement (fp64) of one training step of the DIN scorer, forward, BCE-with-logits and the full backward
(dismember_amd/csrc/train_kernel.hip.inc; reference: tdm/.../optim/LocalOptimizer.scala:139-162), written independently of the C
oracle, and the batches tests/test_gpu_train_edges.py runs.  Test infrastructure only.

The step, per row (q = table[code] or 0 for code -1, k_j = table[seq_j] or 0 for seq_j -1):
  s_j = q . k_j / sqrt(embedSize), -FLT_MAX where masked;  p = softmax(s);  c = sum_j p_j k_j;  a = att.W c
  z = l1.W [q ; a] + l1.b;  h = relu(z);  x = l2.W . h + l2.b;  loss = mean(max(x, 0) + log(1 + exp(-|x|)) - x y)
  gl = (sigmoid(x) - y) / B;  dz = [z > 0] gl l2.W;  dq = l1.Wq^T dz;  da = l1.Wa^T dz;  dc = att.W^T da
  dp_j = dc . k_j;  ds_j = p_j (dp_j - sum_i dp_i p_i) / sqrt(embedSize), 0 where masked
  dq += sum_j ds_j k_j;  dk_j = p_j dc + ds_j q
  table[code] += dq (code >= 0);  table[seq_j] += dk_j (seq_j >= 0);  att.W += da c^T;  l1.W += dz [q ; a]^T;  l1.b += dz;
  l2.W += gl h;  l2.b += gl
in the compact layout [emb ; att.W ; l1.W ; l1.b ; l2.W ; l2.b].

Beside the gradient g, step() returns A: the same accumulation over the ABSOLUTE values of every contribution (one |dq| per row, one
|dk_j| per row and position, one |outer-product term| per row) — the magnitude an element's rounding error scales with, whatever
cancels in g.  An element with A == 0 received nothing but exact zeros.
"""
import functools
import zlib

import numpy as np

from helpers import din_param_count, random_din_weights

TENSORS = ("table", "att.W", "l1.W", "l1.b", "l2.W", "l2.b")
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
FLT_MAX = float(np.finfo(np.float32).max)


def sections(E, NI):
    """name -> (start, stop) in the compact vector"""
    o, out = 0, {}
    for name, n in zip(TENSORS, (NI * E, E * E, 2 * E * E, E, E, 1)):
        out[name] = (o, o + n)
        o += n
    return out


def _scatter_rows(dst, idx, vals):
    """dst[idx[i]] += vals[i], duplicates summed in row order (entries with idx < 0 dropped)"""
    keep = idx >= 0
    idx, vals = idx[keep], vals[keep]
    if idx.size == 0:
        return
    order = np.argsort(idx, kind="stable")
    idx, vals = idx[order], vals[order]
    starts = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
    dst[idx[starts]] += np.add.reduceat(vals, starts, axis=0)


def step(w, E, L, NI, codes, seqs, pad_flat, y, embed_size=None, chunk=2048, loss_only=False):
    """-> dict(loss, g, A, g_dq, g_dk, A_dq, A_dk, touched, relu_margin).  w: compact vector of any float type (widened to fp64);
    pad_flat: flat indices into [B, L] of the masked positions, or None; embed_size: the model's own embed size when the table
    is zero-padded to E (the softmax scale stays 1 / sqrt(embed_size)).  g_dq / g_dk [NI, E]: the candidate and the key part of
    the table gradient (g[table] = g_dq + g_dk), A_dq / A_dk their magnitudes.  touched [NI]: rows named by a candidate or a
    history entry.  relu_margin: min over rows and units of |z| / (|l1.W| |[q ; a]| + |l1.b|), the distance of the nearest
    pre-activation from the ReLU's kink in units of its own accumulated magnitude."""
    w = np.asarray(w, np.float64)
    assert w.size == din_param_count(E, NI)
    sec = sections(E, NI)
    emb = w[slice(*sec["table"])].reshape(NI, E)
    att = w[slice(*sec["att.W"])].reshape(E, E)
    W1 = w[slice(*sec["l1.W"])].reshape(E, 2 * E)
    b1, w2, b2 = w[slice(*sec["l1.b"])], w[slice(*sec["l2.W"])], w[sec["l2.b"][0]]
    codes = np.asarray(codes, np.int64).ravel()
    B = codes.size
    seqs = np.asarray(seqs, np.int64).reshape(B, L)
    y = np.asarray(y, np.float64).ravel()
    masked = np.zeros(B * L, bool)
    if pad_flat is not None and len(pad_flat):
        masked[np.asarray(pad_flat, np.int64)] = True
    masked = masked.reshape(B, L)
    sc = 1.0 / np.sqrt(float(embed_size or E))
    g, A = np.zeros_like(w), np.zeros_like(w)
    g_dq, g_dk, A_dq, A_dk = (np.zeros((NI, E)) for _ in range(4))
    view = lambda v, name, shape: v[slice(*sec[name])].reshape(shape)
    loss, margin = 0.0, np.inf
    for r0 in range(0, B, chunk):
        rows = slice(r0, min(B, r0 + chunk))
        cd, sq, mk, yy = codes[rows], seqs[rows], masked[rows], y[rows]
        q = np.where(cd[:, None] >= 0, emb[np.maximum(cd, 0)], 0.0)
        k = np.where(sq[..., None] >= 0, emb[np.maximum(sq, 0)], 0.0)
        s = np.where(mk, -FLT_MAX, np.einsum("be,ble->bl", q, k) * sc)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        c = np.einsum("bl,ble->be", p, k)
        a = c @ att.T
        qa = np.concatenate([q, a], -1)
        z = qa @ W1.T + b1
        h = np.maximum(z, 0.0)
        x = h @ w2 + b2
        loss += float((np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))) - x * yy).sum())
        zmag = np.abs(qa) @ np.abs(W1).T + np.abs(b1)
        margin = min(margin, float((np.abs(z)[zmag > 0] / zmag[zmag > 0]).min()))
        if loss_only:
            continue
        gl = (1.0 / (1.0 + np.exp(-x)) - yy) / B
        dz = (z > 0) * gl[:, None] * w2
        dq = dz @ W1[:, :E]
        da = dz @ W1[:, E:]
        dc = da @ att
        dp = np.einsum("be,ble->bl", dc, k)
        ds = np.where(mk, 0.0, p * (dp - (dp * p).sum(-1, keepdims=True)) * sc)
        dq = dq + np.einsum("bl,ble->be", ds, k)
        dk = p[..., None] * dc[:, None, :] + ds[..., None] * q[:, None, :]
        for dst, val in ((g_dq, dq), (A_dq, np.abs(dq))):
            _scatter_rows(dst, cd, val)
        for dst, val in ((g_dk, dk), (A_dk, np.abs(dk))):
            _scatter_rows(dst, sq.reshape(-1), val.reshape(-1, E))
        view(g, "att.W", (E, E))[...] += da.T @ c
        view(A, "att.W", (E, E))[...] += np.abs(da).T @ np.abs(c)
        view(g, "l1.W", (E, 2 * E))[...] += dz.T @ qa
        view(A, "l1.W", (E, 2 * E))[...] += np.abs(dz).T @ np.abs(qa)
        view(g, "l1.b", E)[...] += dz.sum(0)
        view(A, "l1.b", E)[...] += np.abs(dz).sum(0)
        view(g, "l2.W", E)[...] += gl @ h
        view(A, "l2.W", E)[...] += np.abs(gl) @ h
        view(g, "l2.b", 1)[...] += gl.sum()
        view(A, "l2.b", 1)[...] += np.abs(gl).sum()
    loss /= B
    if loss_only:
        return loss
    view(g, "table", (NI, E))[...] = g_dq + g_dk
    view(A, "table", (NI, E))[...] = A_dq + A_dk
    touched = np.zeros(NI, bool)
    touched[codes[codes >= 0]] = True
    touched[seqs[seqs >= 0]] = True
    return dict(loss=loss, g=g, A=A, g_dq=g_dq, g_dk=g_dk, A_dq=A_dq, A_dk=A_dk, touched=touched, relu_margin=margin)


def element_scale(A, E, NI):
    """the A of the element bound |g - ref| <= k_T eps A: per element, and per ROW (its maximum) in the table, where the device
    adds a row's E elements with the same atomics in the same order"""
    out = A.copy()
    a, b = sections(E, NI)["table"]
    out[a:b] = np.repeat(A[a:b].reshape(NI, E).max(axis=1), E)
    return out


def tensor_ratios(got, ref, eps, E, NI):
    """per tensor: max |got - ref| / (eps A) over the elements with A > 0, and whether every element with A == 0 is exactly 0"""
    scale = element_scale(ref["A"], E, NI)
    err = np.abs(np.asarray(got, np.float64) - ref["g"])
    out, zeros_exact = {}, True
    for name, (a, b) in sections(E, NI).items():
        live = scale[a:b] > 0
        out[name] = float((err[a:b][live] / (eps * scale[a:b][live])).max()) if live.any() else 0.0
        zeros_exact = zeros_exact and bool((np.asarray(got)[a:b][~live] == 0).all())
    return out, zeros_exact


# ---------------------------------------------------------------------------------------------------------------------------
# The batches of tests/test_gpu_train_edges.py.  Every case is a dict(dtype, E, L, NI, w, batches = [dict(codes, seqs, pad, y,
# users)]); `users` [B] is the row's user where histories are replicated (None otherwise).
SHARED_ROWS = [16, 7, 20, 7, 7, 33, 16, 20, 33, 7, 16, 20, 20, 20, 7]       # rows per user; sum = 249 = 15 * 16 + 9
ALL_PAD_USER, ONE_KEY_USER, PAD_PAIR = 5, 6, (1, 2)                          # (users 1 and 2 fill tile 1 between them)


def _labels(rng, B):
    return (rng.random(B) < 0.3).astype(np.float32)


def _pads(seqs):
    return np.flatnonzero(np.asarray(seqs).reshape(-1) == -1).astype(np.int32)


def _user_histories(rng, U, L, lo, hi):
    seq = rng.integers(lo, hi, (U, L)).astype(np.int32)
    for u, npad in enumerate(rng.integers(0, 4, U)):            # prefix padding, as TreeInit writes histories
        seq[u, :npad] = -1
    return seq


def shared_batch(rng, ns, L, cand=(0, 511), keys=(0, 511), special=True):
    """user-major rows, every user's history replicated over its rows"""
    U = len(ns)
    seq = _user_histories(rng, U, L, *keys)
    if special:
        seq[ALL_PAD_USER] = -1
        seq[ONE_KEY_USER] = seq[ONE_KEY_USER, L - 1]
        for u in PAD_PAIR:
            seq[u, :3] = -1
            seq[u, 3:] = rng.integers(keys[0], keys[1], L - 3)
    users = np.repeat(np.arange(U), ns)
    seqs = seq[users]
    codes = rng.integers(cand[0], cand[1], users.size).astype(np.int32)
    return dict(codes=codes, seqs=seqs, pad=_pads(seqs), y=_labels(rng, users.size), users=users)


def independent_batch(rng, B, L, cand, keys, pad_p=0.2):
    codes = rng.integers(cand[0], cand[1], B).astype(np.int32)
    seqs = rng.integers(keys[0], keys[1], (B, L)).astype(np.int32)
    seqs[rng.random((B, L)) < pad_p] = -1
    return dict(codes=codes, seqs=seqs, pad=_pads(seqs), y=_labels(rng, B), users=None)


def wrap_batch(rng, B, L):
    """T3: replicated histories over B rows; candidates from [0, 400), keys from [400, 900) — rows reached only as a shared key —
    and the last user, whose rows end the batch (row B - 1 stands in for every dead row), alone on the keys [900, 911)"""
    ns = []
    while sum(ns) < B - 25:
        ns.append((16, 7, 20, 33)[len(ns) % 4])
    ns[-1] -= sum(ns) - (B - 25)
    ns.append(25)
    b = shared_batch(rng, ns, L, cand=(0, 400), keys=(400, 900), special=False)
    last = np.arange(900, 900 + L, dtype=np.int32)
    b["seqs"][-25:] = last
    b["pad"] = _pads(b["seqs"])
    return b


WAVES = {"f32": 8, "f64": 4}            # waves per workgroup of dm_train_rows_kernel (DM_BLOCK = 512; 256 threads in fp64)
MAX_CUS = 304                           # the widest Instinct part: the grid is capped at the CU count


def _case_list():
    out = {}
    for dt, Es in (("f32", (16, 32, 64, 128)), ("f64", (16, 128))):
        for E in Es:
            for L in (10, 20):
                out["T1-%s-E%d-L%d" % (dt, E, L)] = dict(kind="shared", dtype=dt, E=E, L=L, NI=511)
    for E in (128, 32):
        out["T2-f32-E%d" % E] = dict(kind="disjoint", dtype="f32", E=E, L=10, NI=511)
    out["T3-f32-E16"] = dict(kind="wrap", dtype="f32", E=16, L=10, NI=8191, B=16 * 8 * 304 + 89)
    for E in (128, 16):
        out["T3-f64-E%d" % E] = dict(kind="wrap", dtype="f64", E=E, L=10, NI=8191, B=16 * 4 * 304 + 41)
    for dt in ("f32", "f64"):
        for B in (1, 2, 15, 17, 127, 128, 129, 131):
            out["T4-%s-B%d" % (dt, B)] = dict(kind="ragged", dtype=dt, E=32, L=10, NI=8191, B=B)
        for what in ("same_candidate", "candidate_is_key", "no_candidate", "unmasked_pads"):
            out["T5-%s-%s" % (dt, what)] = dict(kind=what, dtype=dt, E=64, L=10, NI=8191, B=150)
    return out


CASES = _case_list()


# draws whose nearest pre-activation came within 64 roundings of the ReLU's kink are redrawn (tests/test_train_host.py asserts the margin)
REDRAW = {"T2-f32-E128": 5, "T3-f32-E16": 74}


def _seed(name):
    return zlib.crc32(("%s#%d" % (name, REDRAW[name])).encode() if name in REDRAW else name.encode())


@functools.lru_cache(maxsize=None)
def make_case(name):
    c = dict(CASES[name])
    rng = np.random.default_rng(_seed(name))
    E, L, NI, kind = c["E"], c["L"], c["NI"], c["kind"]
    c["w"] = random_din_weights(rng, E, NI, std=0.2, bias_std=0.2, dtype=np.float32 if c["dtype"] == "f32" else np.float64)
    if kind == "shared":
        batches = [shared_batch(rng, SHARED_ROWS, L)]
    elif kind == "disjoint":
        half = NI // 2
        batches = [shared_batch(rng, SHARED_ROWS, L, cand=(0, half), keys=(half, NI)),
                   independent_batch(rng, 249, L, (0, half), (half, NI))]
    elif kind == "wrap":
        batches = [wrap_batch(rng, c["B"], L)]
    elif kind == "ragged":
        batches = [independent_batch(rng, c["B"], L, (0, NI), (0, NI))]
    else:
        b = independent_batch(rng, c["B"], L, (0, NI), (0, NI))
        if kind == "same_candidate":
            b["codes"][:] = b["codes"][0]
        elif kind == "candidate_is_key":            # at a position that holds a key (not a pad): dq and dk land on the same row
            b["seqs"][:, L - 1] = rng.integers(0, NI, c["B"])
            pos = np.array([rng.choice(np.flatnonzero(row >= 0)) for row in b["seqs"]])
            b["codes"] = b["seqs"][np.arange(c["B"]), pos].copy()
            b["pad"] = _pads(b["seqs"])
        elif kind == "no_candidate":
            b["codes"][rng.choice(c["B"], max(1, c["B"] // 20), replace=False)] = -1
        elif kind == "unmasked_pads":
            b["pad"] = None
        batches = [b]
    c["batches"] = batches
    return c


@functools.lru_cache(maxsize=None)
def reference(name, batch=0):
    c = make_case(name)
    b = c["batches"][batch]
    return step(c["w"], c["E"], c["L"], c["NI"], b["codes"], b["seqs"], b["pad"], b["y"])


def tile_report(b):
    """what the 16-row tiles of a replicated-history batch look like: (tiles uniform at every position, tiles of two or more users,
    tiles of three or more users, tiles of exactly two users in which some position is uniform only because both users hold -1
    there while another position is not uniform)"""
    seqs, users = b["seqs"], b["users"]
    B = len(users)
    uniform_all = multi = triple = pad_only = 0
    for t0 in range(0, B, 16):
        sq, us = seqs[t0:t0 + 16], users[t0:t0 + 16]
        if len(us) < 16:                                          # (the partial tile is filled with copies of row B - 1)
            sq = np.vstack([sq, np.repeat(seqs[-1:], 16 - len(us), axis=0)])
        uni = (sq == sq[0]).all(axis=0)
        n_users = len(set(us.tolist()))
        uniform_all += bool(uni.all())
        multi += n_users >= 2
        triple += n_users >= 3
        pad_only += bool(n_users == 2 and (uni & (sq[0] == -1)).any() and not uni.all())
    return uniform_all, multi, triple, pad_only
