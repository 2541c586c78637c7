"""numpy restatements of the two device primitives of dismember_amd/csrc/dev_sort.hip.inc (stable LSD radix sort of (64-bit key,
32-bit value) pairs on a bit range; stable compaction by a byte flag), the case tables of tests/test_gpu_dev_sort.py and the inputs
of tests/test_gpu_rebalance_edges.py.  tests/test_dev_sort_host.py proves on the CPU that the generated inputs have the properties
the GPU tests rely on.  Test infrastructure only.

Geometry of the kernels: a tile is 4 096 elements (16 rounds of 256); the sort scans a digit's per-tile counts in chunks of 256
tiles with a running carry (dsort_digit_scan_kernel), the compaction scans its per-tile counts in chunks of 1 024 tiles
(dsort_scan_kernel)."""
import numpy as np

TILE = 4096
SORT_SCAN_CHUNK = 256        # tiles per chunk of the sort's digit scan
SELECT_SCAN_CHUNK = 1024     # tiles per chunk of the compaction's scan


def tiles(n):
    return (n + TILE - 1) // TILE


def chunks(n, per_chunk):
    return (tiles(n) + per_chunk - 1) // per_chunk


# ---------------------------------------------------------------------------------------------------------------- references
def sort_digits(keys, begin, end):
    keys = np.asarray(keys, np.uint64)
    bits = end - begin
    if bits <= 0:
        return np.zeros(keys.shape, np.uint64)
    mask = np.uint64((1 << bits) - 1)
    return (keys >> np.uint64(begin)) & mask


def sort_ref(keys, vals, begin, end):
    """stable sort by the key bits [begin, end): the whole 64-bit keys travel, bits outside the range included"""
    perm = np.argsort(sort_digits(keys, begin, end), kind="stable")
    return keys[perm], vals[perm]


def passes(m, begin, end):
    """8-bit passes the sort runs: none for fewer than two elements or an empty range"""
    return 0 if m <= 1 or end <= begin else (end - begin + 7) // 8


def select_ref(flag, inp=None, in2=None):
    idx = np.flatnonzero(flag)
    return (idx.astype(np.int32) if inp is None else inp[idx]), (None if in2 is None else in2[idx]), idx.size


# ---------------------------------------------------------------------------------------------------------------- sort cases
SMALL_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 3 * 4096 + 1]
SORT_BIG_SIZES = [257 * 4096 + 5, 513 * 4096 + 1]         # second / third chunk of the digit scan
SORT_RANGES = [(0, 1), (0, 8), (0, 16), (5, 14), (0, 33), (32, 41), (32, 57), (0, 54), (0, 64), (7, 7)]
SORT_BIG_RANGES = [(0, 64), (32, 57)]
SORT_DISTS = ["uniform", "equal", "two_runs", "tile_digit", "sorted", "reversed", "eight"]
RUN = 6001                   # run length of "two_runs": odd and longer than a tile, so every run straddles a tile boundary


def tile_digit(tile, byte):
    """the digit every key of `tile` carries in the even byte `byte` of the "tile_digit" keys"""
    return (tile * 37 + byte * 11) & 255


def sort_keys(dist, m, seed=0):
    rng = np.random.default_rng([seed, m, SORT_DISTS.index(dist)])
    uni = rng.integers(0, 1 << 64, m, dtype=np.uint64)
    if dist == "uniform":
        return uni
    if dist == "equal":
        return np.full(m, 0xA5C3_0F96_5A3C_F069, np.uint64)
    if dist == "two_runs":       # a > b in bytes 0, 2, 4 and 7, a < b in the others: the two values swap sides between passes
        a, b = np.uint64(0x9111_22F0_7703_EE80), np.uint64(0x1122_3344_5566_7708)
        run = RUN if m >= 2 * TILE else max(1, m // 3)
        return np.where((np.arange(m) // run) % 2 == 0, a, b).astype(np.uint64)
    if dist == "tile_digit":     # even bytes: one digit per tile (a per-tile count of 4 096 for that digit); odd bytes: uniform
        t = np.arange(m, dtype=np.int64) // TILE
        k = uni & np.uint64(0xFF00_FF00_FF00_FF00)
        for byte in (0, 2, 4, 6):
            k |= tile_digit(t, byte).astype(np.uint64) << np.uint64(8 * byte)
        return k
    if dist == "sorted":
        return np.sort(uni)
    if dist == "reversed":
        return np.sort(uni)[::-1].copy()
    if dist == "eight":
        return rng.integers(0, 1 << 64, 8, dtype=np.uint64)[rng.integers(0, 8, m)]
    raise KeyError(dist)


# ---------------------------------------------------------------------------------------------------------------- compaction cases
SELECT_BIG_SIZES = [1025 * 4096 + 3, 2049 * 4096 + 1]     # second / third chunk of dsort_scan_kernel
SELECT_FLAGS = ["none", "all", "half", "sparse", "first", "last", "truthy"]


def select_flags(kind, n, seed=0):
    rng = np.random.default_rng([seed, n, SELECT_FLAGS.index(kind)])
    f = np.zeros(n, np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "half":
        f[:] = rng.random(n) < 0.5
    elif kind == "sparse":
        f[:] = rng.random(n) < 0.001
    elif kind == "first":
        f[:1] = 1
    elif kind == "last":
        f[-1:] = 1
    elif kind == "truthy":       # set flags are 1, 2 or 255: the kernels test truth
        f[:] = np.where(rng.random(n) < 0.5, np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, n)], 0)
    elif kind != "none":
        raise KeyError(kind)
    return f


def select_inputs(n, seed=0):
    rng = np.random.default_rng([seed, n, 99])
    return rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32), rng.integers(0, 1 << 64, n, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- re-balance inputs
def asc_key(w):
    """the ascending Float.compare / Double.compare key of jtm_asc_key: one canonical NaN above +Inf, -0.0 below 0.0"""
    w = np.asarray(w)
    if w.dtype == np.float32:
        b = np.where(np.isnan(w), np.uint32(0x7FC00000), w.view(np.uint32))
        return np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    b = np.where(np.isnan(w), np.uint64(0x7FF8000000000000), w.view(np.uint64))
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(0x8000000000000000)).astype(np.uint64)


def first_choice(w):
    """sortNodeWeights + head: the heaviest child, the first one among equals (a stable descending sort)"""
    return np.argmax(asc_key(w), axis=1)


def recipe_weights(rng, n, C):
    """the re-balance tests' weights: six values, child 0 favoured — crowded ties and several rounds of overflow"""
    w = (rng.integers(0, 6, (n, C)).astype(np.float32) - 2.0) / 2.0
    w[:, 0] += 1.0
    return w


def wide_weights(rng, n, C, f64):
    """standard_normal weights scaled by powers of two drawn over the whole exponent range (per row, so that the heaviest child's
    weight — what the first round sorts — covers the range too, with a quarter of the rows negative), so that every byte of the
    weight key varies; then ±Inf, ±denormals, ±0.0 and NaNs of both signs with different payloads; for double also neighbouring
    rows (returned: the first row of each pair) that differ only below bit 32 of the key"""
    ft, ut, mant, emax = (np.float64, np.uint64, 52, 1000) if f64 else (np.float32, np.uint32, 23, 120)
    w = rng.standard_normal((n, C))
    neg = rng.random(n) < 0.25
    w[neg] = -np.abs(w[neg])                                                         # rows whose heaviest child is negative too
    e_row = np.where(rng.random(n) < 0.5, rng.integers(-emax, emax + 1, n), 0)      # half of the rows: one scale for the row ...
    e_one = np.where(rng.random((n, C)) < 0.1, rng.integers(-emax, emax + 1, (n, C)), e_row[:, None])      # ... a tenth of the weights: their own
    w = np.ldexp(w, e_one).astype(ft)
    sign = (rng.integers(0, 2, (n, C)).astype(ut) << ut(8 * ft().itemsize - 1))
    frac = rng.integers(1, 1 << mant, (n, C)).astype(ut)
    exp_all = ut(((1 << (8 * ft().itemsize - 1 - mant)) - 1) << mant)
    u = rng.random((n, C))
    bits = w.view(ut).copy()
    bits = np.where(u < 0.01, sign | exp_all, bits)                                  # ±Inf
    bits = np.where((u >= 0.01) & (u < 0.02), sign | frac, bits)                     # ±denormal
    bits = np.where((u >= 0.02) & (u < 0.03), sign, bits)                            # ±0.0
    bits = np.where((u >= 0.03) & (u < 0.05), sign | exp_all | frac, bits)           # NaN, either sign, any payload
    rows = np.zeros(0, np.int64)
    if f64:
        rows = np.sort(rng.choice(n // 2, n // 20, replace=False)) * 2               # disjoint pairs (r, r + 1)
        low = rng.integers(0, 1 << 32, (rows.size, C)).astype(ut)
        bits[rows + 1] = (bits[rows] & ut(0xFFFFFFFF00000000)) | low                 # equal above bit 32, different below
    return np.ascontiguousarray(bits).view(ft), rows


REBALANCE_CASES = {
    # name: (n, old_level, gap, slack or ("cap", max_assign)), float and double unless noted
    "wide_keys": (60_000, 3, 2, 1.02),
    "cap_zero": (8192, 1, 2, ("cap", 0)),
    "cap_huge": (8192, 2, 3, ("cap", 8192)),
    "threshold_4096": (4096, 2, 2, 1.0),
    "threshold_4097": (4097, 2, 2, 1.0),
    "outside_level": (40_000, 4, 2, 1.02),
    "deep_sparse": (30_000, 21, 1, 1.0),
    "many_tiles": (1025 * 4096 + 3, 10, 1, 1.02),
}
DEEP_SPARSE_PARENTS = 200


def rebalance_case(name, f64=False):
    """-> dict(w [n, C], old_node, item_node, n, old_level, level, gap, C, P, lo, max_assign)"""
    n, old_level, gap, slack = REBALANCE_CASES[name]
    rng = np.random.default_rng([sorted(REBALANCE_CASES).index(name), int(f64), 5])
    C, P = 1 << gap, 1 << old_level
    lo = P - 1
    occupied = P
    if name == "deep_sparse":
        parents = np.sort(rng.choice(P, DEEP_SPARSE_PARENTS, replace=False))
        item_node = (lo + parents[rng.integers(0, DEEP_SPARSE_PARENTS, n)]).astype(np.int32)
        occupied = DEEP_SPARSE_PARENTS
    else:
        item_node = (lo + rng.integers(0, P, n)).astype(np.int32)
    if name == "wide_keys":
        w, rows = wide_weights(rng, n, C, f64)
        item_node[rows + 1] = item_node[rows]                                         # such a pair sits under one parent: one sorted segment
    else:
        w = recipe_weights(rng, n, C)
        if f64:
            w = w.astype(np.float64) + rng.integers(0, 3, (n, C)) * 2.0 ** -40       # differences only a double holds
    n_in = n
    if name == "outside_level":          # a tenth of the items sit above or below the level, a few at codes below zero
        out = rng.random(n) < 0.1
        other = np.concatenate([np.arange(3, 7), np.arange(7, 15), np.arange(31, 63)])      # levels 2, 3 and 5
        item_node[out] = other[rng.integers(0, other.size, int(out.sum()))]
        neg = np.flatnonzero(out)[:6]
        item_node[neg] = [-1, -2, -7, -(1 << 20), -(1 << 31) + 1, -(1 << 31)]
        n_in = n - int(out.sum())
    first = (item_node.astype(np.int64) << gap) + C - 1
    old_node = (first + rng.integers(0, C, n)).astype(np.int64)
    old_node[rng.random(n) < 0.1] = -7                                              # items that sat elsewhere: "moved" for every child
    old_node = np.clip(old_node, -(1 << 31), (1 << 31) - 1).astype(np.int32)
    max_assign = slack[1] if isinstance(slack, tuple) else max(1, int(np.ceil(n_in / (occupied * C) * slack)))
    return dict(name=name, f64=f64, w=np.ascontiguousarray(w), old_node=old_node, item_node=np.ascontiguousarray(item_node), n=n,
                old_level=old_level, level=old_level + gap, gap=gap, C=C, P=P, lo=lo, max_assign=int(max_assign))


def in_level(case):
    nd = case["item_node"].astype(np.int64)
    return (nd >= case["lo"]) & (nd - case["lo"] < case["P"])


def round_one(case):
    """the first round of the greedy loop on the host -> (sizes [P, C] of the first-choice lists, the child each parent processes or
    -1, mask of the items in the processed lists): what the device compacts and sorts in round 1"""
    C, P = case["C"], case["P"]
    inl = in_level(case)
    fc = first_choice(case["w"])
    p = np.where(inl, case["item_node"].astype(np.int64) - case["lo"], 0)
    sizes = np.bincount((p * C + fc)[inl], minlength=P * C).reshape(P, C)
    best = np.where(sizes.max(axis=1) > case["max_assign"], sizes.argmax(axis=1), -1)         # getMaxNode: the first maximum
    return sizes, best, inl & (best[p] == fc)
