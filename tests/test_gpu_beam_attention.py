"""The beam-search kernels at PEAKED attention: the model scale of attention_cases.peaked_din_weights (embedding table N(0, 1)), at which
a wrong softmax scale, a dropped history position or an ignored mask bit leaves the tolerance (test_attention_cases_host.py), through
test_gpu_parity.replay_and_check — every traced score within 1e-5 + 1e-4 |ref| of the oracle scorer on the same (codes, history), the
reference's integer logic replayed exactly on the device's own scores.

A depth-9 tree with 400 items, beam 24, top-k 20, 16 users with the histories of test_gpu_g_table._histories (pads in front, in the
middle and at the back, an all-pad user, one item repeated, ancestor ids, unknown ids) and two more whose history holds an item the
search itself scores — a leaf among the user's best results — so that the q = k peak (score about sqrt(E), nearly all the weight on
one position) occurs inside the search.  The kernel of every case is asserted by name."""
import functools

import numpy as np
import pytest

import attention_cases as ac
from helpers import synthetic_tree
from test_gpu_g_table import _histories

pytestmark = pytest.mark.gpu
DEPTH, N_ITEMS, BEAM, TOPK, U = 9, 400, 24, 20, 16
assert (1 << (DEPTH + 1)) - 1 == ac.NI

W_CASES = [(E, L) for E in (32, 64, 128) for L in (3, 8, 10, 12, 16)]        # KQ = 1 .. 4, FOLD for L <= 10
LDS_CASES = [(16, 5), (64, 16), (128, 9), (32, 20)]                          # (32, 20): the two-key-tile instance


def _otree(oracle, t):
    return oracle.TdmTree(t["codes"], t["ids"], t["is_leaf"], t["leaf_ids"], t["leaf_codes"], t["max_level"])


@functools.lru_cache(maxsize=None)
def _world(E, L, dtype=np.float32):
    """tree, weights, the 16 + 2 histories and the planted (user, position, item id, leaf code) pairs"""
    from oracle import pyoracle as po
    po.build()
    rng = np.random.default_rng(8800 + 10 * E + L)
    t = synthetic_tree(rng, DEPTH, N_ITEMS)
    w = ac.peaked_din_weights(rng, E, ac.NI, dtype)
    seqs = _histories(rng, t, U, L)
    otree, odin = _otree(po, t), po.Din(w, E, L, ac.NI)
    code_of = dict(zip(t["leaf_ids"].tolist(), t["leaf_codes"].tolist()))
    extra, planted = [], []
    for base, pos in ((0, L - 1), (8, 0)):                  # users 0 and 8 keep random_histories' rows (test_gpu_g_table._histories)
        for cand in otree.recommend(odin, seqs[base], TOPK, BEAM)[0].tolist():
            h = seqs[base].copy()
            h[pos] = cand
            levels = otree.recommend(odin, h, TOPK, BEAM, trace=True)[2]
            if any(code_of[cand] in np.asarray(c).tolist() for c, _ in levels):
                extra.append(h); planted.append((U + len(planted), pos, cand, code_of[cand]))
                break
    assert len(planted) == 2, "no result of the base user stays in the search once it is in the history"
    seqs = np.ascontiguousarray(np.concatenate([seqs, np.stack(extra)]).astype(np.int32))
    for a in (w, seqs):
        a.setflags(write=False)
    return dict(tree=t, w=w, seqs=seqs, planted=planted)


def _engine(t, w, E, mode):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_din(w, E, ac.NI)
    eng.set_scorer_mode(mode)
    return eng


def _run(oracle, E, L, mode, kernel):
    from test_gpu_parity import replay_and_check
    wd = _world(E, L)
    t = wd["tree"]
    otree, odin = _otree(oracle, t), oracle.Din(wd["w"], E, L, ac.NI)
    eng = _engine(t, wd["w"], E, mode)
    try:
        replay_and_check(otree, odin, eng, wd["seqs"], BEAM, TOPK)
        assert eng.last_beam_kernel() == kernel, eng.last_beam_kernel()
        _, _, _, tc, _, tn = eng.tdm_beam_search_trace(wd["seqs"], BEAM, TOPK)
    finally:
        eng.close()
    for u, pos, item, code in wd["planted"]:
        assert wd["seqs"][u, pos] == item
        scored = np.concatenate([tc[u, it, :int(tn[u, it])] for it in range(tn.shape[1])])
        assert code in scored.tolist(), "user %d: the search never scores the item its history holds (code %d)" % (u, code)


@pytest.mark.parametrize("E,L", W_CASES)
def test_w_kernel(oracle, E, L):
    """split_f16 mode: plan_search -> the one-wave-per-SIMD kernel, launch_beam_w_E -> dm_beam_w_kernel<E, ceil(L / 4), 3 L <= 32>; users
    whose G + b1 leaves the fp16 range are scored by the LDS-fed split kernel in the second pass."""
    _run(oracle, E, L, "split_f16", "dm_beam_w_kernel<%d, %d, %s>" % (E, (L + 3) // 4, "true" if 3 * L <= 32 else "false"))


@pytest.mark.parametrize("E,L", LDS_CASES)
def test_lds_fed_kernel(oracle, E, L):
    """f32 mode: launch_beam_E<E, false> -> dm_beam_kernel<E, ceil(L / 4), false>, and for L = 20 its two-key-tile instance
    dm_beam_kernel<32, 4, false, 2>."""
    _run(oracle, E, L, "f32", "dm_beam_kernel<%d, %d, false%s>" % (E, 4 if L > 16 else (L + 3) // 4, ", 2" if L > 16 else ""))


def test_fp64_kernel(oracle):
    """f64 model, otm_beam_search_f64: dm_beam64_kernel<32, 3> (L = 10).  Histories of node codes, every -1 masked; node ids equal to
    oracle.otm_beam_search's, scores within 1e-10 / 1e-9."""
    from dismember_amd import Engine
    E, L = 32, 10
    wd = _world(E, L, np.float64)
    t, w = wd["tree"], wd["w"]
    assert w.dtype == np.float64
    otree, odin = _otree(oracle, t), oracle.Din(w, E, L, ac.NI)
    codes = np.stack([otree.id_to_code(s)[0] for s in wd["seqs"][:U]]).astype(np.int32)
    # the two users whose history holds a node the search scores: a leaf-level node of the base user's result
    extra = []
    for base, pos in ((0, L - 1), (8, 0)):
        for cand in oracle.otm_beam_search(odin, codes[base], DEPTH, BEAM)[0].tolist():
            h = codes[base].copy()
            h[pos] = cand
            if cand in oracle.otm_beam_search(odin, h, DEPTH, BEAM)[0].tolist():
                extra.append(h)
                break
    assert len(extra) == 2
    codes = np.ascontiguousarray(np.concatenate([codes, np.stack(extra)]))
    assert (codes < 0).any() and (codes[3] < 0).all()                      # pads, and the all-pad user
    eng = Engine(0)
    try:
        eng.load_weights_din(w, E, ac.NI)
        ids, sc, cnt = eng.otm_beam_search_f64(codes, BEAM, DEPTH)
        assert eng.last_beam_kernel() == "dm_beam64_kernel<32, 3>", eng.last_beam_kernel()
    finally:
        eng.close()
    assert sc.dtype == np.float64
    worst = 0.0
    for u in range(codes.shape[0]):
        oi, osc = oracle.otm_beam_search(odin, codes[u], DEPTH, BEAM)
        assert cnt[u] == oi.size == 2 * BEAM
        assert np.array_equal(ids[u], oi), u
        err = np.abs(sc[u] - osc) / (1e-10 + 1e-9 * np.abs(osc))
        worst = max(worst, float(err.max()))
        assert (err <= 1.0).all(), (u, float(err.max()))
    print("dm_beam64_kernel<32, 3>: max |err| / tolerance = %.3g" % worst)
