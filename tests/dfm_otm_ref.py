"""OTM with the DeepFM scorer: the cases and the numpy restatement shared by tests/test_dfm_otm_host.py (CPU) and
tests/test_gpu_deepfm_otm.py.

  otm/src/main/scala/com/mass/otm/model/CandidateSearcher.scala:58-80,109-122   beamSearch, buildBeamNodes
  otm/src/main/scala/com/mass/otm/tree/OTMTree.scala:27-63,67-91,104-212        targets, beamSearchNodes
  otm/src/main/scala/com/mass/otm/dataset/MiniBatch.scala:17-40                 batchTransform
  otm/src/main/scala/com/mass/otm/model/OTM.scala:14-22                         recommend (useMask = false for DeepFM)

The scorer is tests/deepfm_ref.py.  The replay takes the DEVICE's scores of level i - 1, orders them as the reference does (the oracle's
stable descending argsort of doubles) and asks for exactly the children of the kept nodes on level i; scores are compared with the
float64 restatement under the project's fp32 contract |gpu - ref64| <= 1e-5 + 1e-4 |ref64|.

Weights: N(0, 0.05) for the table and l2.b as in random_deepfm_weights, N(0, 0.3) for l1.W and l2.W, and l1.b = 0.3 + N(0, 0.3).  With
0.05 everywhere the deep part is ~1e-3 of a logit and a 5 % error in W1a hides below the tolerance on a third of the rows (condition (b)
of the host file); with the larger dense weights it does not, the positive bias keeps ~85 % of the hidden units active (at L = 1 there
are only two, and a row with none active cannot see W1a at all) while the rest still exercise the ReLU, and the float32 restatement
stays inside the tolerance (condition (a)): both are asserted on every case by tests/test_dfm_otm_host.py.
"""
import functools

import numpy as np

import deepfm_ref as R

RTOL, ATOL = 1e-4, 1e-5
EMB_STD, DENSE_STD, B1_SHIFT = 0.05, 0.3, 0.3
MAX_BEAM = 512


def close(a, b):
    """the fp32 contract; a NaN reference asks for a NaN"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(b), np.isnan(a), np.abs(a - b) <= ATOL + RTOL * np.abs(b))


def level_start(beam):
    """(first node of the start level, start level): OTMTree.initializeBeam"""
    s = int(beam).bit_length() - 1
    return (1 << s) - 1, s


def level_counts(beam, leaf_level):
    """candidates per user on the scored levels start + 1 .. leaf"""
    start, s = level_start(beam)
    out, n = [], start + 1
    for level in range(s, leaf_level):
        nb = n if level == s else min(beam, n)
        n = 2 * nb
        out.append(n)
    return out


def trace_cap(beam):
    return max(32, ((2 * beam + 15) // 16) * 16)


# ---- cases: (E, L, beam, leaf_level, U, kind); kind: "plain", "twins" (sibling pairs share a table row), "nan" (one table row NaN)
PLAIN = dict(E=16, L=10, beam=20, leaf_level=9, U=33)
NAN_CODE = 40             # a node of level 5: scored on the first level of beam 20, kept first, expanded
NAN_USER = 3              # this user's history holds NAN_CODE: every score NaN, the order is the position order


def _cases():
    c = []
    for beam in (3, 8, 9):                                   # one partial tile (start level 1); exactly one tile; a second, partial one
        c.append((16, 10, beam, 9, 33, "plain"))
    for beam in (33, 200, 256, 257, 512):                    # five tiles; pcap 512 not full / full; pcap 1024; the cap
        c.append((16, 10, beam, 10, 33, "plain"))
    c.append((16, 10, 20, 4, 33, "plain"))                   # leaf_level = s: the frontier, scores 0
    c.append((16, 10, 20, 5, 33, "plain"))                   # s + 1: one level, no sort
    for L in (1, 10, 14, 15, 30, 31, 32):                    # both sides of both column-tile boundaries of T + 1
        c.append((16, L, 20, 9, 33, "plain"))
    for E in (24, 128):                                      # 24 is padded to 32
        c.append((E, 10, 20, 9, 33, "plain"))
    c.append((128, 32, 200, 10, 33, "plain"))
    c.append((16, 10, 20, 9, 1, "plain"))
    c.append((16, 10, 21, 9, 33, "twins"))                   # an odd beam cuts every tied pair in two
    c.append((16, 10, 20, 9, 33, "nan"))
    return c


CASES = _cases()


def case_id(c):
    return "E%d-L%d-beam%d-leaf%d-U%d-%s" % c


def case_weights(rng, E, L, num_index):
    w = R.random_deepfm_weights(rng, E, L, num_index, std=EMB_STD)
    o = R.deepfm_offsets(E, L, num_index)
    T = L + 1
    w[o["l1_w"]:o["l1_b"]] = rng.normal(0.0, DENSE_STD, T * T * E)
    w[o["l1_b"]:o["l2_w"]] = B1_SHIFT + rng.normal(0.0, DENSE_STD, T)
    w[o["l2_w"]:o["l2_b"]] = rng.normal(0.0, DENSE_STD, T)
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def model(E, L, leaf_level_tree, kind="plain"):
    """(weights, num_index) of a complete tree whose leaf level is 9 or 10; read-only"""
    ni = (1 << (leaf_level_tree + 1)) - 1
    rng = np.random.default_rng(31000 + 100 * E + L + 7 * leaf_level_tree)
    w = case_weights(rng, E, L, ni)
    emb = w[:ni * E].reshape(ni, E)
    if kind == "twins":
        for c in range(31, (ni - 1) // 2):                   # every sibling pair below level 5 shares the left child's row
            emb[2 * c + 2] = emb[2 * c + 1]
    if kind == "nan":
        emb[NAN_CODE] = np.nan
    w.setflags(write=False)
    return w, ni


@functools.lru_cache(maxsize=None)
def histories(L, ni, U, kind="plain"):
    """[U, L] node codes: 20 % pads, user 1 all pads.  The 33 users' first is the user of the U = 1 cases."""
    rng = np.random.default_rng(5000 + L)
    seqs = rng.integers(0, ni, (33, L)).astype(np.int32)
    seqs[rng.random((33, L)) < 0.2] = -1
    seqs[1] = -1
    if kind == "nan":
        seqs[seqs == NAN_CODE] = NAN_CODE + 1
        seqs[NAN_USER, 0] = NAN_CODE
    seqs = np.ascontiguousarray(seqs[:U])
    seqs.setflags(write=False)
    return seqs


def case_inputs(c):
    E, L, beam, leaf_level, U, kind = c
    tree_leaf = 9 if leaf_level <= 9 else 10
    w, ni = model(E, L, tree_leaf, kind)
    return w, ni, histories(L, ni, U, kind)


def ref_scores(w, E, L, ni, codes, seq, dtype=np.float64):
    """logits of `codes` for ONE history"""
    codes = np.asarray(codes, np.int32).reshape(-1)
    return R.forward(w, E, L, ni, codes, np.tile(np.asarray(seq, np.int32), (codes.size, 1)), dtype)


def stable_argsort_desc(scores64):
    """sortBy(_.score)(Ordering[Double].reverse): the oracle's stable argsort under Double.compare"""
    from oracle import pyoracle as po
    sc = np.ascontiguousarray(scores64, np.float64)
    order = np.empty(sc.size, np.int32)
    po.lib().orc_stable_argsort_desc_f64(sc.ctypes.data_as(po.f64p), order.ctypes.data_as(po.i32p), sc.size)
    return order


def search(w, E, L, ni, seq, beam, leaf_level, dtype=np.float64, score_fn=None):
    """CandidateSearcher.beamSearch / OTMTree.beamSearchNodes for one user in `dtype`: [(codes, scores)] per scored level (expansion
    order).  leaf_level <= start level: [] (the frontier is the answer)."""
    start, s = level_start(beam)
    fn = score_fn or (lambda codes: ref_scores(w, E, L, ni, codes, seq, dtype))
    codes, scores = np.arange(start, 2 * start + 1, dtype=np.int32), np.zeros(start + 1, np.float64)
    out = []
    for level in range(s, leaf_level):
        keep = np.arange(codes.size) if level == s else stable_argsort_desc(scores.astype(np.float64))[:beam]
        kept = codes[keep]
        codes = np.stack([2 * kept + 1, 2 * kept + 2], 1).reshape(-1).astype(np.int32)
        scores = np.asarray(fn(codes))
        out.append((codes, scores))
    return out


def replay(seqs, beam, leaf_level, outs, trace, ref_fn):
    """The checks of the GPU file on one traced search.  outs = (ids [U, 2 beam], scores, counts), trace = (tc [U, levels, cap], ts, tn)
    of the device; ref_fn(u, codes) -> float64 logits.  Raises AssertionError; returns (worst error / tolerance, ties at a cut)."""
    ids, sc, cnt = outs
    tc, ts, tn = trace
    start, s = level_start(beam)
    counts = level_counts(beam, leaf_level)
    worst, cut_ties = 0.0, 0
    for u in range(np.asarray(seqs).shape[0]):
        prev_c, prev_s = np.arange(start, 2 * start + 1, dtype=np.int32), np.zeros(start + 1, np.float32)
        for it, n in enumerate(counts):
            assert int(tn[u, it]) == n, ("count", u, it, int(tn[u, it]), n)
            if it == 0:
                keep = np.arange(prev_c.size)
            else:
                order = stable_argsort_desc(prev_s.astype(np.float64))
                keep = order[:beam]
                if order.size > beam:
                    a, b = prev_s[order[beam - 1]], prev_s[order[beam]]
                    cut_ties += int(a == b or (np.isnan(a) and np.isnan(b)))
            kept = prev_c[keep]
            children = np.stack([2 * kept + 1, 2 * kept + 2], 1).reshape(-1)
            assert np.array_equal(tc[u, it, :n], children), ("codes", u, it)
            got = ts[u, it, :n]
            ref = ref_fn(u, children)
            ok = close(got, ref)
            with np.errstate(invalid="ignore"):
                e = np.abs(got.astype(np.float64) - ref) / (ATOL + RTOL * np.abs(ref))
            if np.isfinite(e).any():
                worst = max(worst, float(np.nanmax(e)))
            assert ok.all(), ("score", u, it, int(np.flatnonzero(~ok)[0]), float(np.nanmax(e)))
            prev_c, prev_s = tc[u, it, :n].copy(), ts[u, it, :n].copy()
        for it in range(len(counts), tn.shape[1]):
            assert tn[u, it] == 0, ("count past the leaf level", u, it)
        n = prev_c.size
        assert int(cnt[u]) == n, ("out count", u)
        assert ids[u, :n].tobytes() == prev_c.astype(np.int32).tobytes() and sc[u, :n].tobytes() == prev_s.astype(np.float32).tobytes(), ("outputs", u)
        assert (ids[u, n:] == -1).all() and (sc[u, n:] == 0).all(), ("output padding", u)
    return worst, cut_ties


def otm_finalize(ids, scores, node_to_item, topk):
    """OTM.recommend after the search (OTM.scala:14-22): mapped nodes only, stable sort by score descending, take topk, sigmoid"""
    ids = np.asarray(ids); scores = np.asarray(scores, np.float32)
    items = np.where((ids >= 0) & (ids < node_to_item.size), node_to_item[np.clip(ids, 0, node_to_item.size - 1)], -1)
    keep = items >= 0
    items, scores = items[keep], scores[keep]
    order = stable_argsort_desc(scores.astype(np.float64))[:topk]
    x = scores[order].astype(np.float32)
    return list(zip(items[order].tolist(), (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).tolist()))


# ---- targets (no forward: without a mask both forwards see the sibling tensor, so every node keeps its own label)
def pseudo_targets(target_nodes, beam, leaf_level, mode="pseudo"):
    """list over the levels start + 1 .. leaf of per-user [(node, label)] in list order.  "pseudo": parents grouped in first-appearance
    order with clip(sum of child labels, 0, 1); "normal": every target's ancestor, label 1, no grouping."""
    _, s = level_start(beam)
    cur = [[(int(t), 1.0) for t in tl] for tl in target_nodes]
    levels = [cur]
    for _ in range(leaf_level - 1, s, -1):
        nxt = []
        for nodes in cur:
            if mode == "normal":
                nxt.append([((n - 1) >> 1, 1.0) for n, _ in nodes])
                continue
            acc = {}
            for n, lab in nodes:
                acc[(n - 1) >> 1] = acc.get((n - 1) >> 1, 0.0) + lab
            nxt.append([(k, min(1.0, max(0.0, v))) for k, v in acc.items()])
        levels.insert(0, nxt)
        cur = nxt
    return levels


def level_batch(tc, tn, it, targets_level, seqs):
    """MiniBatch.batchTransform: the level's candidates of every user in user order, label = the first target with that id, else 0"""
    codes, rows, labels = [], [], []
    for u in range(seqs.shape[0]):
        first = {}
        for n, lab in targets_level[u]:
            first.setdefault(n, lab)
        for n in tc[u, it, :tn[u, it]].tolist():
            codes.append(n); rows.append(seqs[u]); labels.append(first.get(n, 0.0))
    return np.asarray(codes, np.int32), np.asarray(rows, np.int32).reshape(len(codes), -1), np.asarray(labels, np.float32)


RAGGED_TARGETS_LEAF = 9


def ragged_targets(U=70):
    """the batch of test_otm_targets_on_device_ragged_batch: no target, one target, sibling targets, a repeated target, and a long
    list at the right end (leaf level 9: nodes 511 .. 1022)"""
    rng = np.random.default_rng(99)
    lo, hi = (1 << RAGGED_TARGETS_LEAF) - 1, (2 << RAGGED_TARGETS_LEAF) - 2
    t = []
    for u in range(U):
        k = u % 5
        if k == 0:
            t.append([])
        elif k == 1:
            t.append([int(rng.integers(lo, hi + 1))])
        elif k == 2:
            a = int(rng.integers(lo, hi) // 2 * 2 + 1)
            t.append([a, a + 1, int(rng.integers(lo, hi + 1))])          # siblings 2c+1, 2c+2
        elif k == 3:
            a = int(rng.integers(lo, hi + 1))
            t.append([a, int(rng.integers(lo, hi + 1)), a])             # a repeated target
        else:
            t.append(rng.integers(lo, hi + 1, 4).tolist())
    t[-1] = rng.integers(lo, hi + 1, 23).tolist()
    return t
