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


def lloyd(x, s0, s1, max_iter=100, tol=1e-4, margin=False):
    """x [n, E]; s0, s1: seed positions -> (c0, c1, assign, distortion, iterations) and, with margin=True, a sixth value: the minimum
    over iterations and items of |d0 - d1| / (d0 + d1), how far the nearest item ever was from the bisecting boundary (1 where both
    distances are zero: such an item sits on both centroids and the tie rule decides in every arithmetic)."""
    x = np.asarray(x, np.float64)
    c0, c1 = x[s0].copy(), x[s1].copy()
    prev, it, mg = 0.0, 0, 1.0
    while True:
        it += 1
        d0, d1 = sqdist(x, c0), sqdist(x, c1)
        a = d1 < d0
        if margin:
            tot = d0 + d1
            mg = min(mg, float(np.where(tot > 0, np.abs(d0 - d1) / np.where(tot > 0, tot, 1.0), 1.0).min()))
        dm = np.where(a, d1, d0)
        D = float(dm.sum())
        far = x[int(np.argmax(dm))]
        n0 = x[~a].mean(axis=0) if (~a).any() else far
        n1 = x[a].mean(axis=0) if a.any() else far
        moved = float(((n0 - c0) ** 2).sum() + ((n1 - c1) ** 2).sum())
        c0, c1 = n0, n1
        if moved <= tol * tol or (it >= 2 and abs(prev - D) <= tol) or it >= max_iter:
            return (c0, c1, a, D, it, mg) if margin else (c0, c1, a, D, it)
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


# ---- the library's counter RNG (dismember_amd/csrc/sampler.hip.inc, cluster.hip.inc), restated with Python integers mod 2^64 ----
M64 = (1 << 64) - 1


def splitmix(z):
    """dm_dev_splitmix"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_draw(seed, t, level, ctr, stream):
    """dm_sample_draw(seed, t, level, ctr, stream)"""
    inner = splitmix(((t & M64) * 64 + level + (stream << 40)) & M64)
    return splitmix((seed & M64) ^ inner ^ ((ctr * 0xD6E8FEB86659FD93) & M64))


def cl_uniform(seed, node, restart, ctr):
    """cl_uniform: stream 9, the top 53 bits as a double in [0, 1)"""
    return float(sample_draw(seed, node, restart, ctr, 9) >> 11) * 2.0 ** -53


def cl_first_seed(seed, node, restart, size):
    return min(int(cl_uniform(seed, node, restart, 0) * float(size)), size - 1)


def predict_seeds(x, seed, node, restart):
    """x: the node's rows in the node's position order -> (s0, candidate positions of the second seed).
    s0 is cl_first_seed.  The second seed is the D^2-weighted pick at u1 * total: d^2 to row s0 in float32 (float32 accumulation over
    E, as the device's distances are), accumulated in fp64 in position order; the device's fmaf order and numpy's differ by float32
    roundings, so every position whose cumulative interval comes within 1e-6 * total of the target is a candidate (normally one).
    total == 0 (every row on the first seed): the next position."""
    x32 = np.asarray(x, np.float32)
    size = len(x32)
    s0 = cl_first_seed(seed, node, restart, size)
    d = ((x32 - x32[s0]) ** 2).sum(axis=1, dtype=np.float32).astype(np.float64)
    cum = np.cumsum(d)
    total = float(cum[-1])
    if not total > 0.0:
        return s0, [(s0 + 1) % size]
    target = cl_uniform(seed, node, restart, 1) * total
    lo, eps = cum - d, 1e-6 * total
    cand = np.flatnonzero((d > 0) & (lo - eps <= target) & (target <= cum + eps))
    if cand.size == 0:                                            # the target beyond the last positive interval: the last such position
        cand = np.flatnonzero(d > 0)[-1:]
    return s0, [int(c) for c in cand]


def nodes(n, perm):
    """(code, level, items in final order) of every internal node"""
    level, sizes = 0, [n]
    while max(sizes) > 1:
        off = 0
        for j, s in enumerate(sizes):
            if s > 1:
                yield (1 << level) - 1 + j, level, perm[off:off + s]
            off += s
        sizes = [v for s in sizes for v in (s // 2, s - s // 2)]
        level += 1


def check_split_rule(x, tr, rel_bound, label="G2"):
    """the split rule on the device's own numbers: at every traced node the left child is a set of the n/2 smallest traced distances,
    and every traced distance is the squared distance to the traced centroid 0 within rel_bound -> nodes checked"""
    n = len(x)
    worst, checked = 0.0, 0
    for code, level, items in nodes(n, tr["perm"]):
        if len(items) < 3:
            assert np.isnan(tr["dist"][level, items]).all()
            continue
        d = tr["dist"][level, items].astype(np.float64)
        h = len(items) // 2
        assert d[:h].max() <= d[h:].min(), (code, "the left child is not a set of the n/2 smallest distances")
        want = sqdist(x[items], tr["centroid0"][code])
        err = np.abs(d - want) / np.maximum(want, 1e-300)
        err = err[want > 0]
        worst = max(worst, float(err.max()) if err.size else 0.0)
        checked += 1
    print("%s: %d nodes, worst relative distance error %.3g (bound %.3g)" % (label, checked, worst, rel_bound))
    assert worst <= rel_bound
    return checked


# ---- which nodes the multi-tile Lloyd comparison (G8) looks at, and the condition it puts on its input ----------------------------
_PATH_BITS = [(0x9E37 * (k + 1)) & 0xFFFF for k in range(8)]


def sampled_indices(level):
    """node indices inside `level` that G8 compares: every node down to level 4, below that eight per level, one fixed root-to-leaf
    path under each node of level 3 (so the set is closed under taking the parent)"""
    if level <= 4:
        return set(range(1 << level))
    d = level - 3
    return set((k << d) | (_PATH_BITS[k] >> (16 - d)) for k in range(8))


def margin_survey(x, restarts, seed, max_iter=100, tol=1e-4, device_rng=False):
    """The restatement's own tree over x, followed through the sampled nodes only -> [(level, size, margin)] of every sampled node of
    three items or more, margin being that of the winning restart's Lloyd run (see lloyd).  The seeds of a node come from a numpy
    generator seeded with `seed`, or with device_rng from the library's counter RNG keyed by (seed, node code, restart) as
    predict_seeds restates it: the tree the device is predicted to build for that seed."""
    x = np.asarray(x, np.float64)
    rng = np.random.default_rng(seed)
    out, stack = [], [(0, 0, np.arange(len(x)))]
    while stack:
        level, j, idx = stack.pop()
        if len(idx) < 3:
            continue
        best = None
        for r in range(restarts):
            if device_rng:
                s0, cand = predict_seeds(x[idx], seed, (1 << level) - 1 + j, r)
                s1 = cand[0]
            else:
                s0, s1 = seed_pair(x[idx], rng)
            c0, _, _, D, it, mg = lloyd(x[idx], s0, s1, max_iter, tol, margin=True)
            if best is None or D < best[0]:
                best = (D, c0, mg, it)
        out.append((level, len(idx), best[2], best[0], best[3]))
        order = split_order(sqdist(x[idx], best[1]))
        h = len(idx) // 2
        nxt = sampled_indices(level + 1)
        for cj, part in ((2 * j, idx[order[:h]]), (2 * j + 1, idx[order[h:]])):
            if cj in nxt:
                stack.append((level + 1, cj, part))
    return out


def margin_floor(E):
    """an item closer to the bisecting boundary than this (relative) may be assigned differently by float32 distances of E terms"""
    return 64 * E * 2.0 ** -24


def hierarchy(n, E, seed, top=4, ratio=0.1, below=0.6, scale=2.0 ** 20):
    """A planted hierarchy over n rows whose planted nodes have the sizes of the balanced recursion (n/2 | n - n/2), shuffled.  Planted
    level l adds +- (a random vector of length s_l per planted node).  Down to level `top`, s_l = scale * ratio^l and the vector lies
    in the first E/2 columns: every node of levels 0 .. top - 1 is two tight, far-apart blobs, so no item comes near a bisecting
    boundary whatever the two seeds are.  Under it, s_l = s_top * ratio * below^(l - top - 1) and the vector lies in the last E/2
    columns: blobs that overlap enough for Lloyd to need several iterations.  The two column sets keep float32 out of the way: the
    members of a node under `top` agree exactly in the first columns, so their mean is exact there and the rounding of a float32
    centroid (2^-24 of each coordinate) is relative to the small coordinates only.  scale = 2^20 puts the smallest distortion (a
    three-item node at the deepest level, 2 s_12^2 = 0.16) three orders above the default tol = 1e-4, so the distortion and
    iteration checks of G8 bind at every compared node (tests/test_cluster_host.py asserts it).  -> x float32 [n, E]."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, E))
    half = max(E // 2, 1)
    segs, level = [(0, n)], 0
    while max(s for _, s in segs) > 1:
        level += 1
        sl = scale * (ratio ** level if level <= top else ratio ** (top + 1) * below ** (level - top - 1))
        nxt = []
        for st, sz in segs:
            if sz < 2:
                nxt.append((st, sz))
                continue
            u = np.zeros(E)
            if level <= top:
                u[:half] = rng.standard_normal(half)
            else:
                u[E - half:] = rng.standard_normal(half)
            u *= sl / np.linalg.norm(u)
            h = sz // 2
            x[st:st + h] -= u
            x[st + h:st + sz] += u
            nxt += [(st, h), (st + h, sz - h)]
        segs = nxt
    return x[rng.permutation(n)].astype(np.float32)


def blobs(n, E, seed, k=12, sigma=0.01):
    """k tight Gaussian blobs (N(0, sigma) around N(0, 1) centres) of unequal sizes, rows interleaved at random: 2-means has many local
    optima on it (which blobs go together), far apart in distortion, and no item near a boundary.  -> x float32 [n, E]."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, E))
    which = rng.choice(k, size=n, p=np.arange(1, k + 1) / (k * (k + 1) / 2.0))
    return (centres[which] + rng.standard_normal((n, E)) * sigma).astype(np.float32)


def predict_winner(x, seed, node, restarts, max_iter=100, tol=1e-4):
    """every restart's predicted seed pair run through lloyd -> (winning restart, its (s0, s1), its distortion, the runner-up's
    distortion, True when every restart had a single second-seed candidate); lowest distortion wins, lowest index on ties"""
    runs, single = [], True
    for r in range(restarts):
        s0, cand = predict_seeds(x, seed, node, r)
        single = single and len(cand) == 1
        runs.append((lloyd(x, s0, cand[0], max_iter, tol)[3], r, s0, cand[0]))
    order = sorted(runs)
    D, r, s0, s1 = order[0]
    return r, (s0, s1), D, (order[1][0] if len(order) > 1 else np.inf), single


def distortion_tol(E, D, tol=1e-4):
    """G3's rule: the device sums float32 distances of E sequential terms (relative error <= E * 2^-24 each, twice that allowed), and
    the two may stop one iteration apart where |D_{t-1} - D_t| straddles the tolerance"""
    return tol + 2 * E * 2.0 ** -24 * D


def balanced_codes(n):
    """the codes of the balanced recursion over the identity order: row i is position i at every level"""
    out, stack = np.zeros(n, np.int64), [(0, 0, n)]
    while stack:
        code, st, sz = stack.pop()
        if sz == 1:
            out[st] = code
        else:
            stack += [(2 * code + 1, st, sz // 2), (2 * code + 2, st + sz // 2, sz - sz // 2)]
    return out


# ---- the cases of tests/test_gpu_cluster_edges.py whose input conditions tests/test_cluster_host.py proves on the CPU ---------------
N8, DATA_SEED, G8_SEED = 2500, {16: 9, 32: 5, 64: 1, 128: 20}, 30      # G8: g8_data(E) clustered with seed G8_SEED


def g8_data(E):
    return hierarchy(N8, E, DATA_SEED[E])


G9_SHAPES = [(200, 16), (300, 16), (1500, 16), (1500, 128)]
G9_WINNER_SEEDS = {(200, 16): [1, 3, 5, 11, 13, 23], (300, 16): [1, 5, 8, 26, 38, 39], (1500, 16): [3, 14, 18, 27, 35, 37],
                   (1500, 128): [2, 10, 12, 14, 16, 23]}   # G9 at 32 restarts, on blobs(n, E, 3)
