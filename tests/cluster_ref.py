"""A numpy restatement (fp64, one node at a time) of the balanced recursive 2-means tree the library builds
(dismember_amd/csrc/cluster.hip.inc; reference: tdm/.../cluster/RecursiveCluster.scala:141-198).  Test infrastructure only.

Rules, as the library states them:
  * Lloyd iteration t: every item goes to the nearer centroid (ties to centroid 0); D_t = sum of squared distances to the assigned
    centroid; new centroid = mean of its items; an empty cluster is re-seeded at the item farthest from the other centroid (first on
    ties).  Stop after t when the summed squared movement of both centroids <= tol^2, or t >= 2 and |D_{t-1} - D_t| <= tol, or
    t = max_iter.  The restart's distortion is D_t; the lowest distortion wins (lowest restart index on ties).
  * centroid 0 is the cluster seeded first.  Items are ordered by squared distance to it (stable); the first n/2 go left.
  * a node of two items: first left, second right.  Recursion down to single items.
"""
import numpy as np


def sqdist(x, c):
    d = np.asarray(x, np.float64) - np.asarray(c, np.float64)
    return (d * d).sum(axis=-1)


def lloyd(x, s0, s1, max_iter=100, tol=1e-4):
    """x [n, E]; s0, s1: seed positions -> (c0, c1, assign, distortion, iterations)."""
    x = np.asarray(x, np.float64)
    c0, c1 = x[s0].copy(), x[s1].copy()
    prev, it = 0.0, 0
    while True:
        it += 1
        d0, d1 = sqdist(x, c0), sqdist(x, c1)
        a = d1 < d0
        dm = np.where(a, d1, d0)
        D = float(dm.sum())
        far = x[int(np.argmax(dm))]
        n0 = x[~a].mean(axis=0) if (~a).any() else far
        n1 = x[a].mean(axis=0) if a.any() else far
        moved = float(((n0 - c0) ** 2).sum() + ((n1 - c1) ** 2).sum())
        c0, c1 = n0, n1
        if moved <= tol * tol or (it >= 2 and abs(prev - D) <= tol) or it >= max_iter:
            return c0, c1, a, D, it
        prev = D


def seed_pair(x, rng):
    """k-means++ for k = 2: first seed uniform, second with probability proportional to D^2."""
    n = len(x)
    s0 = int(rng.integers(n))
    d = sqdist(x, x[s0])
    tot = d.sum()
    if not tot > 0:
        return s0, (s0 + 1) % n
    return s0, int(min(np.searchsorted(np.cumsum(d), rng.random() * tot, side="right"), n - 1))


def fit_node(x, rng, restarts=10, max_iter=100, tol=1e-4):
    best = None
    for _ in range(restarts):
        s0, s1 = seed_pair(x, rng)
        c0, c1, a, D, it = lloyd(x, s0, s1, max_iter, tol)
        if best is None or D < best[3]:
            best = (c0, c1, a, D, it, s0, s1)
    return best


def split_order(d):
    """stable order by distance; the first len // 2 positions are the left child"""
    return np.argsort(d, kind="stable")


def recursive_cluster(x, restarts=10, seed=0, max_iter=100, tol=1e-4):
    """-> codes [n] (before flattenLeaves)."""
    x = np.asarray(x, np.float64)
    rng = np.random.default_rng(seed)
    codes = np.zeros(len(x), np.int64)
    stack = [(0, np.arange(len(x)))]
    while stack:
        code, idx = stack.pop()
        if len(idx) == 1:
            codes[idx[0]] = code
            continue
        if len(idx) == 2:
            left, right = idx[:1], idx[1:]
        else:
            c0 = fit_node(x[idx], rng, restarts, max_iter, tol)[0]
            order = split_order(sqdist(x[idx], c0))
            h = len(idx) // 2
            left, right = idx[order[:h]], idx[order[h:]]
        stack.append((2 * code + 1, left))
        stack.append((2 * code + 2, right))
    return codes


def max_level(n):
    return int(n - 1).bit_length() if n > 1 else 0


def flatten_leaves(codes, min_code):
    out = np.asarray(codes, np.int64).copy()
    while (out < min_code).any():
        out = np.where(out < min_code, 2 * out + 1, out)
    return out


def expected_node_sizes(n):
    """{node code: items below it} of the balanced recursion over n items."""
    out, level = {}, [(0, n)]
    while level:
        nxt = []
        for c, s in level:
            out[c] = s
            if s > 1:
                nxt += [(2 * c + 1, s // 2), (2 * c + 2, s - s // 2)]
        level = nxt
    return out


def node_sizes(codes):
    """{node code: leaves at or below it} of a code assignment"""
    out = {}
    for c in np.asarray(codes, np.int64).tolist():
        while True:
            out[c] = out.get(c, 0) + 1
            if c == 0:
                break
            c = (c - 1) // 2
    return out


def check_structure(codes, n):
    """the invariants of ClusterTreeSpec plus the balanced split at every internal node"""
    codes = np.asarray(codes, np.int64)
    assert codes.shape == (n,)
    ml = max_level(n)
    assert len(set(codes.tolist())) == n, "codes are not distinct"
    assert (flatten_leaves(codes, 2 ** ml - 1) >= 2 ** ml - 1).all() and (codes < 2 ** (ml + 1) - 1).all()
    if ml > 0:
        assert (codes >= 2 ** (ml - 1) - 1).all(), "a leaf above level max_level - 1"
    flat = flatten_leaves(codes, 2 ** ml - 1)
    assert len(set(flat.tolist())) == n and ((flat >= 2 ** ml - 1) & (flat < 2 ** (ml + 1) - 1)).all()
    assert node_sizes(codes) == expected_node_sizes(n), "a split is not n/2 | n - n/2"


def planted(depth, E, sigma, seed):
    """A planted complete binary hierarchy of 2^depth items, shuffled: level l adds +- (a random unit vector per planted node) * 0.5^l,
    plus N(0, sigma) noise.  -> (x float32 [n, E], planted leaf index of every row)."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    x = np.zeros((n, E))
    leaf = np.arange(n)
    for l in range(1, depth + 1):
        parents = leaf >> (depth - l + 1)
        u = rng.standard_normal((1 << (l - 1), E))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        sign = np.where((leaf >> (depth - l)) & 1, 1.0, -1.0)
        x += sign[:, None] * u[parents] * 0.5 ** l
    x += rng.standard_normal((n, E)) * sigma
    p = rng.permutation(n)
    return x[p].astype(np.float32), leaf[p]


def recovery(codes, planted_leaf, depth, level):
    """fraction of the tree's nodes at `level` whose item set equals a planted node's item set"""
    codes = np.asarray(codes, np.int64)
    d = np.floor(np.log2(codes + 1)).astype(np.int64)
    anc = ((codes + 1) >> (d - level)) - 1
    want = {}
    for i, g in enumerate((planted_leaf >> (depth - level)).tolist()):
        want.setdefault(g, set()).add(i)
    want = set(frozenset(s) for s in want.values())
    got = {}
    for i, a in enumerate(anc.tolist()):
        got.setdefault(a, set()).add(i)
    return sum(frozenset(s) in want for s in got.values()) / float(1 << level)


def f32_distance_error(x, c):
    """max relative error of a plain float32 evaluation of ||x - c||^2 against fp64 (rows with a zero distance left out)"""
    x32, c32 = np.asarray(x, np.float32), np.asarray(c, np.float32)
    d32 = ((x32 - c32) ** 2).sum(axis=1, dtype=np.float32).astype(np.float64)
    d64 = sqdist(x32, c32)
    ok = d64 > 0
    return float((np.abs(d32 - d64)[ok] / d64[ok]).max())


def f32_mean_error(x):
    """max absolute error of a plain float32 column mean against fp64"""
    x32 = np.asarray(x, np.float32)
    return float(np.abs(x32.mean(axis=0, dtype=np.float32).astype(np.float64) - x32.astype(np.float64).mean(axis=0)).max())
