"""numpy restatement of the JTM child-weight pipeline (dismember_amd/csrc/jtm_host.hip.inc: dm_jtm_expand_kernel, dm_jtm_rowseq_kernel,
dm_jtm_codes_kernel, dm_jtm_sum_kernel) and the catalogue of tests/test_jtm_ref_host.py and tests/test_gpu_jtm_scoring.py.
tests/test_jtm_ref_host.py proves it against the CPU oracle before it judges a kernel.  Test infrastructure only: no device, no library.

Reference: JTMTree.idToCodeWithMask (jtm/.../tree/JTMTree.scala:86-113), TreeLearning.aggregateWeights (jtm/.../optim/TreeLearning.scala:
152-174).  Pair order: item, training row, chain node; chain nodes level-major (levels old_level + 1 .. level, left to right), so the
2^(gap+1) - 2 pairs of one training row are adjacent and pair q = row * nchain + x for the absolute row number."""
import numpy as np


def nchain_of(gap):
    return (2 << gap) - 2


def ancestor_at_level(codes, level):
    """JTMTree.getAncestorAtLevel (JTMTree.scala:36-43): the loop, not a closed form"""
    c = np.array(codes, np.int64, copy=True)
    lim = (1 << (level + 1)) - 1
    while True:
        up = c >= lim
        if not up.any():
            return c
        c[up] = (c[up] - 1) >> 1


def id_to_code_with_mask(row_ids, id_to_code, non_leaf_offset, max_code, level=0, hierarchical=False, min_level=0, num_index=None):
    """-> (codes int32, mask bool, bad bool), each of row_ids' shape.  mask holds ONLY the padding id 0; an id beyond
    non_leaf_offset + max_code becomes code -1 WITHOUT a mask bit; bad marks the ids whose code falls outside [-1, num_index)
    (num_index None: below -1), where the reference's embedding lookup would fail — their code is reported as -1."""
    ids = np.asarray(row_ids, np.int64)
    lut = np.asarray(id_to_code, np.int64)
    assert lut.size == non_leaf_offset
    pad = ids == 0
    inside = (ids > 0) & (ids < non_leaf_offset)
    leaf = np.where(inside, lut[np.where(inside, ids, 0)], -1)
    known = inside & (leaf >= 0)
    if hierarchical and level >= min_level:
        leaf = np.where(known, ancestor_at_level(np.where(known, leaf, 0), level), -1)
    other = ((ids - non_leaf_offset + (1 << 31)) % (1 << 32)) - (1 << 31)           # the subtraction wraps like the reference's Int
    other = np.where(other > max_code, -1, other)
    codes = np.where(pad, -1, np.where(known, leaf, other))
    bad = codes < -1
    if num_index is not None:
        bad |= codes >= num_index
    codes = np.where(bad, -1, codes)
    return codes.astype(np.int32), pad, bad


def expand_pairs(row_off, row_ids, item_node, L, old_level, level, id_to_code, non_leaf_offset, max_code, hierarchical=False, min_level=0,
                 use_mask=True, num_index=None):
    """Every (training row) x (chain node) pair of the items [0, n): dict(codes [P], seqs [P, L], mask [P, L] bool, item [P], row [P],
    chain [P], bad bool).  The chain node of depth d and offset c below the item's node is (node << d) + (1 << d) - 1 + c; hierarchical:
    the history of a pair is lifted to the pair's own level old_level + d when that level is >= min_level."""
    row_off = np.asarray(row_off, np.int64)
    n = row_off.size - 1
    gap = level - old_level
    nchain = nchain_of(gap)
    R = int(row_off[n] - row_off[0])
    rows = np.asarray(row_ids, np.int32).reshape(-1)[int(row_off[0]) * L:int(row_off[n]) * L].reshape(R, L)
    row_item = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_off))
    x = np.arange(nchain, dtype=np.int64)
    d = np.zeros(nchain, np.int64)
    for k in range(1, gap + 1):
        d[(1 << k) - 2:(2 << k) - 2] = k
    c = x - ((1 << d) - 2)
    node = np.asarray(item_node, np.int64)[row_item]
    codes = (node[:, None] << d[None, :]) + (1 << d[None, :]) - 1 + c[None, :]                          # [R, nchain]
    seqs = np.empty((R, nchain, L), np.int32)
    mask = np.zeros((R, nchain, L), bool)
    bad = False
    if hierarchical:
        for k in range(1, gap + 1):
            cd, m, b = id_to_code_with_mask(rows, id_to_code, non_leaf_offset, max_code, old_level + k, True, min_level, num_index)
            seqs[:, d == k, :] = cd[:, None, :]; mask[:, d == k, :] = m[:, None, :]; bad = bad or bool(b.any())
    else:
        cd, m, b = id_to_code_with_mask(rows, id_to_code, non_leaf_offset, max_code, num_index=num_index)
        seqs[:] = cd[:, None, :]; mask[:] = m[:, None, :]; bad = bool(b.any())
    if not use_mask:
        mask[:] = False
    P = R * nchain
    return dict(codes=codes.reshape(P).astype(np.int32), seqs=seqs.reshape(P, L), mask=mask.reshape(P, L),
                item=np.repeat(row_item, nchain), row=np.repeat(np.arange(R, dtype=np.int64) + row_off[0], nchain), chain=np.tile(x, R), bad=bad)


def pad_flat(mask):
    """flat positions of the mask bits, the form the DIN forwards take them in"""
    return np.flatnonzero(np.asarray(mask).reshape(-1)).astype(np.int32)


def sum_weights_f32(logits, row_off, gap):
    """[n, 2^gap] float32.  Per (item, chain node) the sum over the item's rows in row order (Tensor.sum), then the child -> parent
    chain from the deepest level up (TreeLearning.scala:163-171); every addition is one np.float32 addition, made in sequence.
    Items without rows get -1e6."""
    row_off = np.asarray(row_off, np.int64)
    n = row_off.size - 1
    nchild, nchain = 1 << gap, nchain_of(gap)
    lg = np.asarray(logits)
    assert lg.dtype == np.float32 and lg.size == int(row_off[n] - row_off[0]) * nchain
    lg = lg.reshape(-1, nchain)
    out = np.empty((n, nchild), np.float32)
    child = np.arange(nchild)
    for i in range(n):
        a, b = int(row_off[i] - row_off[0]), int(row_off[i + 1] - row_off[0])
        if a == b:
            out[i] = np.float32(-1e6)
            continue
        score = np.add.accumulate(np.concatenate([np.zeros((1, nchain), np.float32), lg[a:b]]), axis=0, dtype=np.float32)[-1]
        w = np.zeros(nchild, np.float32)
        for k in range(gap, 0, -1):
            w = w + score[(1 << k) - 2 + (child >> (gap - k))]
        out[i] = w
    return out


def sum_bound_f32(logits, row_off, gap):
    """[n, 2^gap] float64: (terms - 1) * 2^-24 * sum |logit| over the terms = rows * gap logits of a weight — the first-order bound of a
    sequential fp32 sum of that many terms (each of its additions rounds a partial sum no larger than sum |logit| by at most 2^-24
    relative)."""
    row_off = np.asarray(row_off, np.int64)
    n = row_off.size - 1
    nchild, nchain = 1 << gap, nchain_of(gap)
    lg = np.abs(np.asarray(logits, np.float64)).reshape(-1, nchain)
    out = np.zeros((n, nchild))
    child = np.arange(nchild)
    for i in range(n):
        a, b = int(row_off[i] - row_off[0]), int(row_off[i + 1] - row_off[0])
        col = lg[a:b].sum(axis=0)
        tot = sum(col[(1 << k) - 2 + (child >> (gap - k))] for k in range(gap, 0, -1))
        out[i] = max((b - a) * gap - 1, 0) * 2.0 ** -24 * tot
    return out


def chain_sum(per_pair, row_off, gap):
    """[n, 2^gap] float64: a per-pair quantity summed over the rows * gap pairs that feed one weight (tolerance budgets)"""
    row_off = np.asarray(row_off, np.int64)
    n = row_off.size - 1
    nchild, nchain = 1 << gap, nchain_of(gap)
    v = np.asarray(per_pair, np.float64).reshape(-1, nchain)
    out = np.zeros((n, nchild))
    child = np.arange(nchild)
    for i in range(n):
        col = v[int(row_off[i] - row_off[0]):int(row_off[i + 1] - row_off[0])].sum(axis=0)
        out[i] = sum(col[(1 << k) - 2 + (child >> (gap - k))] for k in range(gap, 0, -1))
    return out


# ---------------------------------------------------------------------------------------------------------------- the catalogue
def make_catalogue(rng, leaf_ids, leaf_codes, L, holes=0, big=40):
    """The catalogue both test files score.  leaf_ids / leaf_codes: the tree's leaves (dismember_amd.synth.make_tree); `holes` of them
    (never the largest id nor the largest code) are left out of the id map, which makes their ids holes below non_leaf_offset.
    -> dict(items ascending, item_code, map_ids, map_codes, id_to_code, non_leaf_offset, max_code, row_off, row_ids [R, L], hole_ids).

    Rows per item: none for the first item, the last item and a run of three consecutive items; 1 row for every seventh item; `big` rows
    for one item, so that whole 16-row scorer tiles lie inside one item; 2 .. 5 for the rest.
    Histories: known leaf ids with a prefix of pads (id 0, code -1 plus a mask bit), one all-pad history, and sprinkled over them
    non_leaf_offset + 5 (an internal node), non_leaf_offset + max_code (the last admissible code) and non_leaf_offset + max_code + 1
    (code -1 WITHOUT a mask bit: a zero key that takes part in the softmax).  No history holds a hole."""
    leaf_ids = np.asarray(leaf_ids, np.int32); leaf_codes = np.asarray(leaf_codes, np.int32)
    keep = np.ones(leaf_ids.size, bool)
    cand = np.flatnonzero((leaf_ids != leaf_ids.max()) & (leaf_codes != leaf_codes.max()))
    drop = rng.choice(cand, holes, replace=False) if holes else np.zeros(0, np.int64)
    keep[drop] = False
    map_ids, map_codes = leaf_ids[keep], leaf_codes[keep]
    order = np.argsort(map_ids)
    items, item_code = map_ids[order], map_codes[order]
    nlo, max_code = int(map_ids.max()) + 1, int(map_codes.max())
    lut = np.full(nlo, -1, np.int32)
    lut[map_ids] = map_codes
    n = items.size
    assert n >= 40
    nrows = rng.integers(2, 6, n)
    nrows[3::7] = 1
    nrows[n // 2] = big
    nrows[[0, n - 1, 20, 21, 22]] = 0
    row_off = np.zeros(n + 1, np.int64)
    np.cumsum(nrows, out=row_off[1:])
    R = int(row_off[n])
    rows = rng.choice(items, (R, L)).astype(np.int32)
    npad = rng.binomial(L, 0.2, R)
    rows[np.arange(L)[None, :] < npad[:, None]] = 0
    edge = np.array([nlo + 5, nlo + max_code, nlo + max_code + 1], np.int32)
    u = rng.random((R, L))
    for k, e in enumerate(edge):
        rows[(u >= 0.04 * k) & (u < 0.04 * (k + 1))] = e
    b0 = int(row_off[n // 2])                                  # the big item: every edge in its first tile, the all-pad history in its second
    rows[b0 + 1, 0], rows[b0 + 2, L - 1], rows[b0 + 3, L // 2], rows[b0 + 4, 0] = edge[0], edge[1], edge[2], 0
    rows[b0 + 17] = 0
    one = int(row_off[3])                                      # a 1-row item whose only history starts with the unmasked zero key
    rows[one, 0] = edge[2]
    return dict(items=items, item_code=item_code, map_ids=map_ids, map_codes=map_codes, id_to_code=lut, non_leaf_offset=nlo, max_code=max_code,
                row_off=row_off, row_ids=rows, hole_ids=leaf_ids[~keep])
