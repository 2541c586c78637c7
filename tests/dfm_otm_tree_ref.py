"""numpy restatement of OTM tree construction's child weights with the DeepFM scorer (dismember_amd/csrc/dfm_otm_tree.hip.inc) and the
cases shared by tests/test_dfm_otm_tree_host.py (CPU) and tests/test_gpu_deepfm_otm_tree.py.  Test infrastructure only: no device, no
library.

A weight is a sum of pair logits: item i sits in node item_node[i] of old_level; its chain holds the nodes of depth d = 1 .. gap below that
node, left to right (code (node << d) + (1 << d) - 1 + c, chain index x = (1 << d) - 2 + c); every history row of the item is scored
against every chain node (dfm_jtm_ref.pairs_forward: the per-history form of the DeepFM graph); per chain node the logits are added in
double over the item's rows in segments of `seg` rows (each from 0.0, left to right), the segment sums left to right from 0.0; child c gets
sum over d = gap .. 1 of score[(1 << d) - 2 + idx], idx = c, idx >>= 1.  An item without rows gets -1e6.  Histories hold NODE codes, -1 =
padding.  The model is dfm_jtm_ref.weights(E, L) over NI = 2047 nodes (levels 0 .. 10)."""
import functools

import numpy as np

import dfm_jtm_ref as J

NI = J.NI
SEG = 256                                  # DFM_OTM_TREE_SEG
ROWS_SMALL = (0, 1, 3, 4, 5, 11)           # rows per item of the small cases (DM_DFM_OTM_TREE_SEG=4: none, inside, one short, exact, one over, three segments)

# (E, L, old_level, gap, rows per item (cycled), items, segment length the case runs under)
CASES = [(E, L, J.OLD_LEVEL[(E, L)], gap, ROWS_SMALL, 13, 4) for E, L in J.SCORER_EL for gap in (1, 2, 3)]      # one tile: 2, 6, 14 live chain rows
CASES += [(128, 10, 2, 4, ROWS_SMALL, 7, 4),        # 30 chain nodes: two tiles, 14 live in the second
          (128, 15, 2, 5, ROWS_SMALL, 7, 4),        # 62: four tiles
          (16, 10, 2, 8, (2, 0, 5), 5, 4),          # 510: 32 tiles
          (16, 10, 4, 2, (255, 256, 257), 3, SEG)]  # the native segment: one short, exact, one over


def case_id(c):
    return "E%d-L%d-old%d-gap%d-%s-seg%d" % (c[0], c[1], c[2], c[3], "x".join(map(str, c[4])), c[6])


@functools.lru_cache(maxsize=None)
def catalogue(L, old_level, rows, n_items):
    """row_off [n + 1], rows [R, L] node codes, item_node [n]: the first history is all padding, the second has holes, the third repeats
    one code; the last item sits in the last node of old_level"""
    rng = np.random.default_rng(4242 + 131 * L + 17 * old_level + n_items)
    counts = np.array([rows[i % len(rows)] for i in range(n_items)], np.int64)
    row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(row_off[-1])
    h = rng.integers(0, NI, (R, L)).astype(np.int32)
    pad = rng.integers(0, L + 1, R)
    for r in range(R):
        h[r, :pad[r] // 2] = -1                                       # leading padding, as the reference's windows have it
    if R > 0:
        h[0, :] = -1
    if R > 1:
        h[1, ::2] = -1
    if R > 2:
        h[2, :] = h[2, -1]
    lo, hi = (1 << old_level) - 1, (2 << old_level) - 2
    node = rng.integers(lo, hi + 1, n_items).astype(np.int32)
    node[-1] = hi
    for a in (row_off, h, node):
        a.setflags(write=False)
    return row_off, h, node


def chain_codes(node, gap):
    """[n, nchain] codes in chain order"""
    node = np.asarray(node, np.int64).reshape(-1)
    cols = []
    for d in range(1, gap + 1):
        for c in range(1 << d):
            cols.append((node << d) + (1 << d) - 1 + c)
    return np.stack(cols, 1).astype(np.int32)


def pair_codes(row_off, node, gap):
    """[R * nchain] node codes in (row, chain node) order: pair i belongs to history i // nchain"""
    row_off = np.asarray(row_off, np.int64)
    item = np.repeat(np.arange(row_off.size - 1), np.diff(row_off))
    return np.ascontiguousarray(chain_codes(node, gap)[item].reshape(-1))


def pair_logits(E, L, row_off, rows, node, gap, dtype):
    """[R, nchain] logits of the restatement in `dtype`"""
    nchain = (2 << gap) - 2
    R = int(row_off[-1])
    if R == 0:
        return np.zeros((0, nchain), dtype)
    out = J.pairs_forward(J.weights(E, L), E, L, NI, pair_codes(row_off, node, gap), rows, seq_div=nchain, dtype=dtype)
    return out.reshape(R, nchain)


def left_to_right(x):
    """sum over axis 0 in double, strictly left to right from 0.0"""
    x = np.asarray(x, np.float64)
    return np.cumsum(np.concatenate([np.zeros((1,) + x.shape[1:]), x], 0), 0)[-1]


def child_of(idx):
    return idx >> 1


def weights_from_logits(logits, row_off, gap, seg=SEG, drop_last=False, depths=None, parent=child_of):
    """[n, 1 << gap] float64 from [R, nchain] logits of any float type.  drop_last / depths / parent: the mutations of the host test."""
    row_off = np.asarray(row_off, np.int64)
    n, nchild, nchain = row_off.size - 1, 1 << gap, (2 << gap) - 2
    out = np.empty((n, nchild), np.float64)
    for i in range(n):
        r0, r1 = int(row_off[i]), int(row_off[i + 1])
        if r1 == r0:
            out[i] = -1e6
            continue
        if drop_last:
            r1 -= 1
        parts = [left_to_right(logits[a:min(a + seg, r1)]) for a in range(r0, r1, seg)]
        score = left_to_right(np.stack(parts)) if parts else np.zeros(nchain)
        for c in range(nchild):
            w, idx = np.float64(0.0), c
            for d in range(gap, 0, -1):
                if depths is None or d in depths:
                    w = w + score[(1 << d) - 2 + idx]
                idx = parent(idx)
            out[i, c] = w
    return out


def bound(logits64, row_off, gap):
    """what a weight may differ from the float64 restatement by: the project's fp32 contract per logit (dfm_jtm_ref.ATOL, RTOL), summed
    over the pairs the weight adds up"""
    return weights_from_logits(J.tolerance(logits64), row_off, gap) * (np.diff(np.asarray(row_off))[:, None] > 0)


def units(row_off, gap, seg=SEG):
    """the kernel's unit list: (item, chain tile, first row, rows) per wave's unit, segment-major"""
    row_off = np.asarray(row_off, np.int64)
    ntiles = ((2 << gap) - 2 + 15) // 16
    out = []
    for i in range(row_off.size - 1):
        for a in range(int(row_off[i]), int(row_off[i + 1]), seg):
            for t in range(ntiles):
                out.append((i, t, a, min(seg, int(row_off[i + 1]) - a)))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(c):
    """(row_off, rows, node, logits64 [R, nchain], weights64 under the case's segment length, bound): computed once, shared, read-only"""
    E, L, old_level, gap, rows, n_items, seg = c
    row_off, h, node = catalogue(L, old_level, rows, n_items)
    lg = pair_logits(E, L, row_off, h, node, gap, np.float64)
    w = weights_from_logits(lg, row_off, gap, seg)
    b = bound(lg, row_off, gap)
    for a in (lg, w, b):
        a.setflags(write=False)
    return row_off, h, node, lg, w, b
