"""TEST INFRASTRUCTURE — models and rows at which the DIN attention is PEAKED, shared by the CPU file that proves the inputs
(test_attention_cases_host.py) and the GPU files that hold the kernels to the oracle on them (test_gpu_rows_attention.py,
test_gpu_beam_attention.py).

helpers.random_din_weights draws the embedding table at the reference's init scale, N(0, 0.05): q.k / sqrt(E) is then about 0.003 and
the softmax is uniform to three digits, so a kernel whose attention is wrong (softmax scale, a dropped position, an ignored mask bit)
stays inside 1e-5 + 1e-4 |ref|.  peaked_din_weights draws the table from N(0, 1): scores are O(1), and about sqrt(E) where a key
equals the query.  with_fault is the float64 numpy statement of the forward with one such fault switched on; the CPU file measures with
it that every fault moves the rows it concerns out of the tolerance at this scale.  numpy only: no device, no library."""
import functools

import numpy as np

from helpers import random_din_weights

FLT_MAX = float(np.finfo(np.float32).max)
ATOL, RTOL = 1e-5, 1e-4                          # the f32 contract of test_gpu_parity.py
NI = 1023
ROWS_B = 16 * 8 + 16 * 3 + 5                     # random rows of a GPU case: a block's eight tiles, three more, a ragged last one
F64_B = 300                                      # ... of an f64 case: at least 256 rows take the matrix-pipe forward, fewer the scalar kernel
SHARE_B = 2000                                   # random rows of the fault-sensitivity measurement

# (E, L) per kernel of the general-rows forward (dm_hip.hip: dm_din_forward -> din_rows_dev -> launch_rows_split_E)
MFMA_F32 = [(E, L) for E in (16, 32, 64, 128) for L in (1, 2, 5, 11, 13, 16)]       # set_scorer_mode("f32"): dm_din_rows_kernel<E>
SPLIT_GENERIC = [(E, L) for E in (32, 64, 128) for L in (1, 3, 7, 9, 12, 15)]       # default mode, no counted instance: dm_din_rows_split_kernel<E>
SPLIT_COUNTED = [(E, L) for E in (32, 64, 128) for L in (8, 10, 16)]                # dm_din_rows_split_l_kernel<E, L>
LONG = [(16, 17), (64, 24), (128, 32)]                                              # L = 17 .. 32: din_forward_t<float>
F64 = [(32, 16), (128, 7)]                                                          # f64 model: rows_fwd64 (>= 256 rows) / dm_din_forward_kernel<double>
# standard deviation of the embedding table per cell; a cell whose fault shares fall short of the bound gets a larger one here
EMB_STD = {}


def all_cells():
    """every (E, L, dtype) the GPU files run, once"""
    seen = []
    for E, L in MFMA_F32 + SPLIT_GENERIC + SPLIT_COUNTED + LONG:
        if (E, L, np.float32) not in seen:
            seen.append((E, L, np.float32))
    return seen + [(E, L, np.float64) for E, L in F64]


def peaked_din_weights(rng, E, NI, dtype=np.float32, emb_std=1.0):
    """Compact A0 vector: embedding table N(0, emb_std), att.W / l1.W / l2.W and the biases N(0, 0.05)."""
    w = random_din_weights(rng, E, NI, dtype=dtype)
    w[:NI * E] = rng.normal(0.0, emb_std, NI * E).astype(dtype)
    return w


def embedding(w, E, NI):
    return np.asarray(w[:NI * E], np.float64).reshape(NI, E)


def _named_rows(rng, E, L, NI, emb):
    """[(name, code, seq [L], mask [L] bool)]; a name is built only where L has room for what it says"""
    rows = []

    def live(n=L):
        return rng.integers(0, NI, n).astype(np.int32)

    def add(name, code, seq, mask):
        seq = np.asarray(seq, np.int32); mask = np.asarray(mask, bool)
        assert seq.shape == (L,) and mask.shape == (L,)
        rows.append((name, int(code), seq, mask))
    npad = min(2, L - 1)
    none = np.zeros(L, bool)
    if npad:
        s = live(); s[:npad] = -1
        add("pads_masked", rng.integers(0, NI), s, s < 0)
        s = live(); s[L - npad:] = -1
        add("pads_unmasked", rng.integers(0, NI), s, none)
        s = live(); m = none.copy(); m[0] = True                                  # the key at 0 is live and masked
        add("masked_live_key", rng.integers(0, NI), s, m)
    if L >= 3:
        s = live(); s[[0, L // 2]] = -1; m = none.copy(); m[0] = True            # pad 0 masked, pad L // 2 not
        add("unmasked_pad_beside_masked", rng.integers(0, NI), s, m)
    add("live_keys_all_masked", rng.integers(0, NI), live(), ~none)
    if L >= 2:
        s = live(); s[L // 2] = -1
        add("all_masked_one_pad", rng.integers(0, NI), s, ~none)
    add("all_pad_unmasked", rng.integers(0, NI), np.full(L, -1), none)
    add("all_pad_masked", rng.integers(0, NI), np.full(L, -1), ~none)
    add("code_minus_one", -1, live(), none)
    c = int(rng.integers(0, NI)); s = live(); s[s == c] = (c + 1) % NI; s[0] = c
    add("own_code_first", c, s, none)
    c = int(rng.integers(0, NI)); s = live(); s[s == c] = (c + 1) % NI; s[L - 1] = c
    add("own_code_last", c, s, none)
    c = int(rng.integers(0, NI)); s = rng.choice(NI, L, replace=False).astype(np.int32)
    order = np.argsort(emb[s] @ emb[c], kind="stable")
    add("scores_ascending", c, s[order], none)                                    # the running maximum moves at every step
    c = int(rng.integers(0, NI)); s = rng.choice(NI, L, replace=False).astype(np.int32)
    order = np.argsort(-(emb[s] @ emb[c]), kind="stable")
    add("scores_descending", c, s[order], none)                                   # ... or never after the first
    add("one_key_repeated", rng.integers(0, NI), np.full(L, rng.integers(0, NI)), none)
    s = live(); m = none.copy(); m[L - 1] = True                                   # bit L - 1 (bit 15 at L = 16) on a live key
    add("mask_bit_last", rng.integers(0, NI), s, m)
    if L >= 2:
        s = live(); s[L - 1] = -1; m = none.copy(); m[L - 1] = True
        add("mask_bit_last_on_pad", rng.integers(0, NI), s, m)
    return rows


class RowsCase(tuple):
    """(codes [B'], seqs [B', L], mask [B', L] bool); .names maps a named row's name to its index"""
    names = None


def rows_case(rng, E, L, NI, B, emb):
    """The named rows (first) and B random rows: 25 % pads, half of them masked, and one live key in twenty masked; one code in 37 is
    -1.  emb [NI, E]: the model's table, which the rows sorted by score are sorted with."""
    named = _named_rows(rng, E, L, NI, np.asarray(emb, np.float64))
    codes = rng.integers(0, NI, B).astype(np.int32); codes[5::37] = -1
    seqs = rng.integers(0, NI, (B, L)).astype(np.int32)
    pad = rng.random((B, L)) < 0.25
    seqs[pad] = -1
    mask = (pad & (rng.random((B, L)) < 0.5)) | (~pad & (rng.random((B, L)) < 0.05))
    out = RowsCase((np.concatenate([np.array([r[1] for r in named], np.int32), codes]),
                    np.ascontiguousarray(np.concatenate([np.stack([r[2] for r in named]), seqs])),
                    np.concatenate([np.stack([r[3] for r in named]), mask])))
    out.names = {r[0]: i for i, r in enumerate(named)}
    assert len(out.names) == len(named)
    return out


def pad_flat(mask):
    """flat positions of the mask bits, the form the DIN forwards take them in"""
    return np.flatnonzero(np.asarray(mask).reshape(-1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(E, L, dtype=np.float32, B=None):
    """dict(w, codes, seqs, mask, pad, names): the model and the rows of cell (E, L), the same arrays for the CPU and the GPU file.
    B random rows (default: ROWS_B, F64_B for an f64 model) behind the named ones."""
    default_b = F64_B if dtype == np.float64 else ROWS_B
    B = default_b if B is None else B
    rng = np.random.default_rng(52000 + 100 * E + L + (7 if dtype == np.float64 else 0) + (3 if B != default_b else 0))
    w = peaked_din_weights(rng, E, NI, dtype, EMB_STD.get((E, L), 1.0))
    case = rows_case(rng, E, L, NI, B, embedding(w, E, NI))
    codes, seqs, mask = case
    out = dict(w=w, codes=codes, seqs=seqs, mask=mask, pad=pad_flat(mask), names=case.names, E=E, L=L)
    for a in (w, codes, seqs, mask, out["pad"]):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the restatement
FAULTS = ("scale_x1.05", "unmasked_pad_not_counted", "last_position_dropped", "mask_ignored_upper_half", "sixteenth_position_leaks")


def with_fault(w, E, L, NI, codes, seqs, mask, fault=None):
    """helpers.numpy_din_forward (float64) on a mask [B, L], with one fault of FAULTS switched on:
    scale_x1.05               the softmax scale 1 / sqrt(E) times 1.05
    unmasked_pad_not_counted  an unmasked pad (zero key, score 0) gets no weight instead of exp(0 - max)
    last_position_dropped     position L - 1 gets no weight
    mask_ignored_upper_half   mask bits of the positions ceil(L / 2) .. L - 1 are not read
    sixteenth_position_leaks  L < 16: one more position with a zero key and score 0 is counted in the denominator"""
    assert fault is None or fault in FAULTS
    w = np.asarray(w, np.float64)
    emb = w[:NI * E].reshape(NI, E)
    o = NI * E
    att_w = w[o:o + E * E].reshape(E, E); o += E * E
    l1_w = w[o:o + 2 * E * E].reshape(E, 2 * E); o += 2 * E * E
    l1_b = w[o:o + E]; o += E
    l2_w = w[o:o + E]; o += E
    l2_b = w[o]
    codes = np.asarray(codes); seqs = np.asarray(seqs).reshape(len(codes), L)
    mask = np.array(mask, bool).reshape(len(codes), L)
    if fault == "mask_ignored_upper_half":
        mask[:, (L + 1) // 2:] = False
    q = np.where(codes[:, None] >= 0, emb[np.maximum(codes, 0)], 0.0)
    k = np.where(seqs[..., None] >= 0, emb[np.maximum(seqs, 0)], 0.0)
    s = np.einsum("be,ble->bl", q, k) / np.sqrt(E)
    if fault == "scale_x1.05":
        s = s * 1.05
    s = np.where(mask, -FLT_MAX, s)
    p = np.exp(s - s.max(-1, keepdims=True))
    if fault == "unmasked_pad_not_counted":
        p = np.where((seqs < 0) & ~mask, 0.0, p)
    if fault == "last_position_dropped":
        p[:, L - 1] = 0.0
    den = p.sum(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if fault == "sixteenth_position_leaks" and L < 16:
            den = den + np.exp(0.0 - s.max(-1, keepdims=True))          # (inf in a row whose positions are all masked: c = 0)
        p = p / den
    c = np.einsum("bl,ble->be", p, k)
    a = c @ att_w.T
    h = np.concatenate([q, a], -1) @ l1_w.T + l1_b
    h = np.maximum(h, 0)
    return h @ l2_w + l2_b


def concerned(fault, L, codes, seqs, mask):
    """bool [B]: the rows in which the fault changes a weight of a live key (decided from the structure of the row, not from values)"""
    codes = np.asarray(codes); seqs = np.asarray(seqs); mask = np.asarray(mask, bool)
    livekey = seqs >= 0
    open_ = ~mask                                                    # positions that take part in the softmax
    all_masked = mask.all(-1)
    has_open_live = (livekey & open_).any(-1)
    if fault == "scale_x1.05":
        # a query, and two open positions with different keys (a pad is the key -1)
        lo = np.where(open_, seqs, np.iinfo(np.int32).max).min(-1)
        hi = np.where(open_, seqs, np.iinfo(np.int32).min).max(-1)
        return (codes >= 0) & (open_.sum(-1) >= 2) & (lo != hi) & has_open_live
    if fault == "unmasked_pad_not_counted":
        return ((~livekey) & open_).any(-1) & has_open_live
    if fault == "last_position_dropped":
        return open_[:, L - 1] & (open_.sum(-1) >= 2) & has_open_live
    if fault == "mask_ignored_upper_half":
        up = np.arange(L) >= (L + 1) // 2
        lifted_live = (mask & up & livekey).any(-1)                  # a masked live key comes back
        lifted_pad = (mask & up & ~livekey).any(-1) & has_open_live  # a masked pad comes back beside open live keys
        return (lifted_live | lifted_pad) & ~all_masked
    if fault == "sixteenth_position_leaks":
        return has_open_live if L < 16 else np.zeros(len(codes), bool)
    raise ValueError(fault)


def outside(got, ref):
    """bool [B]: rows outside the f32 contract (a NaN is outside)"""
    return ~(np.abs(np.asarray(got, np.float64) - ref) <= ATOL + RTOL * np.abs(ref))
