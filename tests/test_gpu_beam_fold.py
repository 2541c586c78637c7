"""The folded attention-combine of the one-wave beam kernel (dm_beam_w_kernel<E, KQ, FOLD>, beam_kernel_w.hip.inc): for L <= 10
the product H^T += (G + b1)^T P^T is ONE v_mfma_f32_16x16x32_f16 per feature tile — the three terms p_hi G_hi, p_hi G_lo, p_lo G_hi
of every history position share its 32 contraction slots (dmw_fold_slot), the p_lo G_hi term of positions 8 and 9 through a
cross-lane exchange.  L = 11 .. 16 keep the two-MFMA product.

Every case is a small search (depth 11, 1 500 items, 12 users, split scorer, the kernel asserted by name) under the assertions of
test_gpu_precision.py::test_split_scorer_error_vs_exact, with that test's numbers:
  * every traced score within ATOL + RTOL |ref32| of the fp32 CPU oracle;
  * against the fp64 oracle on the same fp32 weights: split rms <= 1.25 x the fp32-input MFMA kernel's and <= 1.05 x the fp32 CPU
    oracle's own rms (a dropped or misplaced p_lo G_hi term is ~2^-12 relative: three orders above these bounds);
  * the reference's integer logic replayed on the device's own scores reproduces every level's candidates and the final list bit
    for bit.
The cases: the lengths around every change of path (FOLD without / with the exchange, unfolded inside KQ = 3, KQ = 4) at E = 128
(hand-placed tile) and E = 32 (generic tile); histories that single out the exchanged positions 8 and 9; beams that give 1, 2, 3 and
7 tiles per level (pair loop, odd last tile, clamped re-reads).  test_fold_cases_oracle_only runs the oracle-only part of every
case without a GPU: the inputs build, the searches score rows, and the fp32 oracle itself is inside the tolerance against fp64.
"""
import numpy as np
import pytest

from helpers import random_din_weights, random_histories, synthetic_tree

RTOL, ATOL = 1e-4, 1e-5
DEPTH, N_ITEMS, U = 11, 1500, 12
NI = (1 << (DEPTH + 1)) - 1

L_SWEEP = [(128, 4), (128, 8), (128, 9), (128, 10), (128, 11), (128, 12), (128, 16), (32, 8), (32, 10), (32, 12)]
PATTERN_LS = [9, 10]
TILE_BEAMS = [(8, 1), (16, 2), (24, 3), (50, 7)]          # (beam, 16-row tiles of a full level: 2 beam children)


def _kernel_name(E, L):
    return "dm_beam_w_kernel<%d, %d, %s>" % (E, (L + 3) // 4, "true" if 3 * L <= 32 else "false")


def _inputs(seed, E, L):
    rng = np.random.default_rng(seed)
    t = synthetic_tree(rng, DEPTH, N_ITEMS)
    w = random_din_weights(rng, E, NI, bias_std=0.01)
    seqs = random_histories(rng, t["leaf_ids"], U, L)
    return rng, t, w, seqs


def _pattern_histories(rng, leaf_ids, L):
    """Two users per pattern; positions 8 and 9 are the ones whose p_lo G_hi term crosses lanes."""
    item = lambda: int(rng.choice(leaf_ids))
    rows, names = [], []

    def add(name, fill):
        for _ in range(2):
            s = np.zeros(L, np.int32)
            fill(s)
            rows.append(s); names.append(name)
    add("all_pad", lambda s: None)
    add("only_8", lambda s: s.__setitem__(8, item()))
    last = L - 1                                  # 9 at L = 10; at L = 9 the last position is 8: the pair becomes {2, 8}
    if L == 10:
        add("only_9", lambda s: s.__setitem__(9, item()))

    def same(s, where):
        s[list(where)] = item()
    add("same_item_at_2_and_%d" % last, lambda s: same(s, (2, last)))          # p = 0.5 at both
    add("same_item_at_2_5_%d" % last, lambda s: same(s, (2, 5, last)))         # p = 1/3: p_lo != 0 at the exchanged slot

    def pads_at_end(s):
        s[:] = rng.choice(leaf_ids, L)
        s[8:] = 0
    add("pads_at_8_and_up", pads_at_end)
    rnd = random_histories(rng, leaf_ids, U - len(rows), L)
    for s in rnd:
        rows.append(s); names.append("random")
    return np.ascontiguousarray(np.stack(rows).astype(np.int32)), names


def _case_inputs(kind, E, L, beam):
    seed = {"sweep": 7100, "pattern": 7300, "tiles": 7500}[kind] + 10 * L + E + beam
    rng, t, w, seqs = _inputs(seed, E, L)
    names = ["random"] * U
    if kind == "pattern":
        seqs, names = _pattern_histories(rng, t["leaf_ids"], L)
    else:
        seqs[0] = 0
    assert seqs.shape == (U, L)
    return t, w, seqs, names


ALL_CASES = ([("sweep", E, L, 50) for E, L in L_SWEEP] + [("pattern", 128, L, 50) for L in PATTERN_LS] +
             [("tiles", 128, 10, b) for b, _ in TILE_BEAMS])


def _otree(oracle, t):
    return oracle.TdmTree(t["codes"], t["ids"], t["is_leaf"], t["leaf_ids"], t["leaf_codes"], t["max_level"])


def _rows_of(otree, seqs, levels_of_user):
    codes, hist, pads = [], [], []
    for u in range(seqs.shape[0]):
        sc, mask = otree.id_to_code(seqs[u])
        m = np.zeros(sc.size, bool); m[mask] = True
        for c in levels_of_user(u):
            if c.size:
                codes.append(c); hist.append(np.tile(sc, (c.size, 1))); pads.append(np.tile(m, (c.size, 1)))
    return np.concatenate(codes), np.concatenate(hist), np.flatnonzero(np.concatenate(pads).reshape(-1)).astype(np.int32)


def _errs(x, exact):
    d = x.astype(np.float64) - exact
    return float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())


def test_fold_cases_oracle_only(oracle):
    """No GPU: every case's inputs build, its searches score rows on the CPU oracle, the pattern histories decode to the pad
    patterns they are named for, and the fp32 oracle is inside ATOL + RTOL |s| of the fp64 oracle on those rows."""
    for kind, E, L, beam in ALL_CASES:
        t, w, seqs, names = _case_inputs(kind, E, L, beam)
        otree = _otree(oracle, t)
        o32, o64 = oracle.Din(w, E, L, NI), oracle.Din(w.astype(np.float64), E, L, NI)
        lv = [[c for c, _ in otree.recommend(o32, seqs[u], min(2 * beam, 200), beam, trace=True)[2]] for u in range(U)]
        codes, hist, pad = _rows_of(otree, seqs, lambda u: lv[u])
        assert codes.size > U * beam
        ref32, exact = o32.forward(codes, hist, pad), o64.forward(codes, hist, pad)
        assert (np.abs(ref32 - exact) <= ATOL + RTOL * np.abs(exact)).all(), (kind, E, L, beam)
        for u, nm in enumerate(names):
            _, mask = otree.id_to_code(seqs[u])
            live = sorted(set(range(L)) - set(mask.tolist()))
            if nm == "all_pad": assert live == []
            if nm == "only_8": assert live == [8]
            if nm == "only_9": assert live == [9]
            if nm.startswith("same_item_at_2_and"): assert live == [2, L - 1] and seqs[u, 2] == seqs[u, L - 1]
            if nm.startswith("same_item_at_2_5"): assert live == [2, 5, L - 1]
            if nm == "pads_at_8_and_up": assert live == list(range(8))
    # tiles per level of the tile-count cases: a full level has 2 beam children
    for beam, tiles in TILE_BEAMS:
        assert (2 * beam + 15) // 16 == tiles


def _replay_exact(otree, present, seqs, beam, topk, ids, sc, cnt, tc, ts, tn):
    """The reference's integer logic (level_step / finalize) on the DEVICE's scores: candidates of every level and the final list bit-exact."""
    start, level = (1 << (beam.bit_length() - 1)) - 1, beam.bit_length() - 1
    for u in range(seqs.shape[0]):
        cand = np.array([c for c in range(start, 2 * start + 1) if c in present], np.int32)
        preds = np.zeros(cand.size, np.float32)
        leaves = []
        n_iter = otree.max_level - level + 1
        for it in range(n_iter):
            lc, lp, children = otree.level_step(beam, cand, preds)
            leaves.insert(0, (lc, lp))
            n = int(tn[u, it])
            assert n == children.size, (u, it, n, children.size)
            assert np.array_equal(tc[u, it, :n], children), (u, it)
            cand, preds = children, ts[u, it, :n].copy()
        assert (tn[u, n_iter:] == 0).all()
        fi, fs = otree.finalize(np.concatenate([a for a, _ in leaves]), np.concatenate([b for _, b in leaves]), topk)
        assert cnt[u] == fi.size, (u, cnt[u], fi.size)
        assert np.array_equal(ids[u, :cnt[u]], fi), u
        assert np.array_equal(sc[u, :cnt[u]], fs), u


def _run_case(oracle, kind, E, L, beam):
    from dismember_amd import Engine
    t, w, seqs, names = _case_inputs(kind, E, L, beam)
    otree = _otree(oracle, t)
    present = set(t["codes"].tolist())
    exact_din = oracle.Din(w.astype(np.float64), E, L, NI)      # the exact value of the SAME fp32 weights
    o32 = oracle.Din(w, E, L, NI)
    eng = Engine(0)
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_din(w, E, NI)
    topk = min(2 * beam, 200)
    res = {}
    try:
        for mode in ("split_f16", "f32"):
            eng.set_scorer_mode(mode)
            ids, sc, cnt, tc, ts, tn = eng.tdm_beam_search_trace(seqs, beam, topk)
            if mode == "split_f16":
                assert eng.last_beam_kernel() == _kernel_name(E, L), eng.last_beam_kernel()
                _replay_exact(otree, present, seqs, beam, topk, ids, sc, cnt, tc, ts, tn)
            codes, hist, pad = _rows_of(otree, seqs, lambda u: [tc[u, it, :int(tn[u, it])] for it in range(tn.shape[1])])
            got = np.concatenate([ts[u, it, :int(tn[u, it])] for u in range(U) for it in range(tn.shape[1]) if int(tn[u, it])])
            exact = exact_din.forward(codes, hist, pad)
            ref32 = o32.forward(codes, hist, pad)
            res[mode] = dict(dev=_errs(got, exact), oracle32=_errs(ref32, exact), rows=int(codes.size))
            bad = np.flatnonzero(np.abs(got - ref32) > ATOL + RTOL * np.abs(ref32))
            print("fold case", kind, E, L, beam, mode, res[mode], "rows outside the tolerance:", bad.size)
            assert bad.size == 0, (mode, bad[:8], got[bad[:8]], ref32[bad[:8]])
    finally:
        eng.close()
    (rs, ms), (rf, mf) = res["split_f16"]["dev"], res["f32"]["dev"]
    ro, _ = res["split_f16"]["oracle32"]
    line = dict(kind=kind, E=E, L=L, beam=beam, rows=res["split_f16"]["rows"], split_rms=rs, split_max=ms, f32_mfma_rms=rf,
                f32_mfma_max=mf, cpu_oracle_f32_rms=ro)
    assert rs <= 1.25 * rf and ms <= 1.25 * mf + 1e-9, line       # no less accurate than the fp32-input MFMA tile
    assert rs <= ro * 1.05 and rf <= ro * 1.05, line                # and neither worse than the fp32 oracle's own rounding


@pytest.mark.gpu
@pytest.mark.parametrize("E,L", L_SWEEP)
def test_fold_length_sweep(oracle, E, L):
    _run_case(oracle, "sweep", E, L, 50)


@pytest.mark.gpu
@pytest.mark.parametrize("L", PATTERN_LS)
def test_fold_history_patterns(oracle, L):
    _run_case(oracle, "pattern", 128, L, 50)


@pytest.mark.gpu
@pytest.mark.parametrize("beam,tiles", TILE_BEAMS)
def test_fold_tile_counts(oracle, beam, tiles):
    _run_case(oracle, "tiles", 128, 10, beam)
