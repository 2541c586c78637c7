"""JTM child weights (dismember_amd/csrc/jtm_host.hip.inc: jtm_child_weights_impl), held to an exact restatement.

tests/test_gpu_rows_static.py asserts that a row's logit depends neither on its tile mates nor on its position in the tile, so the logits
the JTM scorer sees are, bit for bit, what Engine.din_forward returns for the same (code, history, mask) rows.  The whole pipeline —
the uncached expand path, the cached per-row path (histories read through seq_div = chain nodes per row), cached ranges, the chunk
loop — must then EQUAL jtm_ref.sum_weights_f32(din_forward(jtm_ref.expand_pairs(...))), which tests/test_jtm_ref_host.py proves against
the CPU oracle.  (b) holds the same weights to the oracle under the project's per-logit contract, (c) crosses the chunk boundaries
with DM_JTM_MAX_PAIRS, (d) puts a hole of the id map into a history.

Set-up: a depth-10 tree with 300 leaves, two of them left out of the id map (holes), the catalogue of jtm_ref.make_catalogue (about
1 000 training rows: none / 1 / 2 .. 5 / 40 per item) and load_weights_din_synthetic; no training state on any handle."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import jtm_ref
from dismember_amd import synth
from test_gpu_parity import ATOL, RTOL

pytestmark = pytest.mark.gpu
DEPTH, LEAVES, NI = 10, 300, 2047
DM_ERR_INDEX = -4


@functools.lru_cache(maxsize=None)
def _tree():
    return synth.make_tree(LEAVES, DEPTH, np.random.default_rng(77))


@functools.lru_cache(maxsize=None)
def _cat(L):
    """the same holes and the same rows per item for every history length (the generator is seeded alike and draws them first)"""
    t = _tree()
    return jtm_ref.make_catalogue(np.random.default_rng(1000), t["leaf_ids"], t["leaf_codes"], L, holes=2)


_ENGINES = {}


def _engine(E, mode="auto", f64=False):
    key = (E, mode, f64)
    if key not in _ENGINES:
        from dismember_amd import Engine
        t, cat = _tree(), _cat(10)
        eng = Engine(0)
        eng.load_tree(t["codes"], t["ids"], t["is_leaf"], DEPTH)
        eng.load_id_maps(cat["map_ids"], cat["map_codes"])
        if f64:
            eng.load_weights_din_synthetic_f64(E, NI, 9)
        else:
            eng.load_weights_din_synthetic(E, NI, 9, tree_depth=DEPTH, rho=0.9)
            if mode != "auto":
                eng.set_scorer_mode(mode)
            assert eng.scorer_mode()["mode"] == ("f32" if E == 16 or mode == "f32" else "split_f16")
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _case.cache_clear()


def _lib():
    from dismember_amd import _native as N
    return N, N.lib()


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _uncached(eng, cat, L, node, old_level, level, hier, min_level, use_mask, check=True):
    N, lib = _lib()
    n = cat["items"].size
    w = np.full((n, 1 << (level - old_level)), np.nan, np.float32)
    rc = lib.dm_jtm_child_weights(eng._h, _ptr(cat["row_off"], N.i64p), _ptr(cat["row_ids"], N.i32p), _ptr(node, N.i32p), n, L, old_level, level,
                                  int(hier), min_level, int(use_mask), _ptr(w, N.f32p))
    if check:
        eng._chk(rc)
        return w
    return rc


def _cache(eng, cat, L, lo=0, hi=None):
    N, lib = _lib()
    n = cat["items"].size
    eng._chk(lib.dm_jtm_cache_rows_range(eng._h, _ptr(cat["row_off"], N.i64p), _ptr(cat["row_ids"], N.i32p), n, L, lo, n if hi is None else hi))


def _uncache(eng, L):
    _, lib = _lib()
    eng._chk(lib.dm_jtm_cache_rows(eng._h, None, None, 0, L))


def _cached(eng, node, lo, hi, old_level, level, hier, min_level, use_mask, check=True):
    N, lib = _lib()
    sub = np.ascontiguousarray(node[lo:hi])
    w = np.full((hi - lo, 1 << (level - old_level)), np.nan, np.float32)
    rc = lib.dm_jtm_child_weights_cached(eng._h, _ptr(sub, N.i32p), lo, hi - lo, old_level, level, int(hier), min_level, int(use_mask), _ptr(w, N.f32p))
    if check:
        eng._chk(rc)
        return w
    return rc


def _cuts(n):
    return [(0, n // 3), (n // 3, n // 3 + 1), (n // 3 + 1, n)]


def _all_device_paths(eng, cat, L, node, old_level, level, hier, min_level, use_mask):
    """uncached call, cached call over the full range, three cached ranges on a handle that holds only that range"""
    n = cat["items"].size
    out = {"uncached": _uncached(eng, cat, L, node, old_level, level, hier, min_level, use_mask)}
    _cache(eng, cat, L)
    out["cached"] = _cached(eng, node, 0, n, old_level, level, hier, min_level, use_mask)
    parts = []
    for lo, hi in _cuts(n):
        _cache(eng, cat, L, lo, hi)
        parts.append(_cached(eng, node, lo, hi, old_level, level, hier, min_level, use_mask))
    out["ranges"] = np.concatenate(parts, axis=0)
    _uncache(eng, L)
    return out


@functools.lru_cache(maxsize=None)
def _case(E, mode, L, old_level, level, use_mask, hier):
    """every device path of one case and the restatement over din_forward of the same pairs; computed once, shared by (a), (b), (c)"""
    eng, cat = _engine(E, mode), _cat(L)
    min_level = 6 if hier else 0
    node = jtm_ref.ancestor_at_level(cat["item_code"], old_level).astype(np.int32)
    out = _all_device_paths(eng, cat, L, node, old_level, level, hier, min_level, use_mask)
    px = jtm_ref.expand_pairs(cat["row_off"], cat["row_ids"], node, L, old_level, level, cat["id_to_code"], cat["non_leaf_offset"], cat["max_code"],
                              hier, min_level, use_mask, NI)
    assert not px["bad"]
    logits = eng.din_forward(px["codes"], px["seqs"], jtm_ref.pad_flat(px["mask"]), L=L)
    assert logits.dtype == np.float32 and np.isfinite(logits).all()
    out.update(node=node, pairs=px, logits=logits, ref=jtm_ref.sum_weights_f32(logits, cat["row_off"], level - old_level), min_level=min_level)
    return out


GAPS = [(4, 5), (4, 6), (4, 7), (2, 7), (2, 10)]            # gap 1, 2, 3, 5 and 8: the widest allowed, 510 chain nodes, codes on the leaf level
CASES = ([(32, "auto", 10, a, b, True, False) for a, b in GAPS] +
         [(E, "auto", L, 4, lv, True, False) for E in (32, 16) for L in (1, 7, 8, 10, 16) for lv in (6, 7) if not (E == 32 and L == 10)] +
         [(128, "auto", 10, 4, 7, True, False), (32, "f32", 10, 4, 7, True, False),
          (32, "auto", 10, 4, 7, False, False),               # use_mask = 0: pads are zero keys that take part in the softmax
          (32, "auto", 10, 4, 7, True, True)])                # hierarchical, min_level 6: level 5 keeps the leaf codes, levels 6 and 7 lift
_id = lambda c: "E%d-%s-L%d-%dto%d-mask%d-hier%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_path_equals_the_restatement_bit_for_bit(case):
    """(a)"""
    E, mode, L, old_level, level, use_mask, hier = case
    r = _case(*case)
    cat = _cat(L)
    seen = np.diff(cat["row_off"]) > 0
    assert (r["ref"][~seen] == np.float32(-1e6)).all() and np.isfinite(r["ref"]).all()
    assert len(np.unique(r["ref"][seen])) > seen.sum()                       # the weights are not degenerate
    for name in ("cached", "ranges", "uncached"):
        got = r[name]
        differ = np.flatnonzero((got != r["ref"]).any(axis=1))
        assert np.array_equal(got, r["ref"]), "%s: %d items differ, first %s (rows %s)" % (
            name, differ.size, differ[:5].tolist(), np.diff(cat["row_off"])[differ[:5]].tolist())


def test_hierarchical_lifts_some_chain_levels_only():
    """the hierarchical case means what it says: with min_level 6 the level-5 pairs keep the leaf codes, the level-6 and -7 pairs do not"""
    r = _case(32, "auto", 10, 4, 7, True, True)
    flat = _case(32, "auto", 10, 4, 7, True, False)
    nchain = 14
    a, b = r["pairs"]["seqs"].reshape(-1, nchain, 10), flat["pairs"]["seqs"].reshape(-1, nchain, 10)
    assert np.array_equal(a[:, :2], b[:, :2]) and (a[:, 2:] != b[:, 2:]).any() and not np.array_equal(r["ref"], flat["ref"])


@functools.lru_cache(maxsize=None)
def _oracle_model(E, L):
    from oracle import pyoracle
    t, cat = _tree(), _cat(L)
    otree = pyoracle.TdmTree(t["codes"], t["ids"], t["is_leaf"], cat["map_ids"], cat["map_codes"], DEPTH)
    return otree, pyoracle.Din(_engine(E).download_weights(), E, L, NI)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_weights_against_the_oracle(oracle, case):
    """(b): |w - oracle.jtm_child_weights| <= sum over the weight's rows * gap logits of (ATOL + RTOL |logit_ref|), the per-logit contract
    of tests/test_gpu_parity.py; the reference logits are the oracle's forward of the expanded pairs.  The values are the ones the
    device holds (download_weights)."""
    E, mode, L, old_level, level, use_mask, hier = case
    r, cat = _case(*case), _cat(L)
    otree, odin = _oracle_model(E, L)
    w_ref = oracle.jtm_child_weights(otree, odin, cat["items"], cat["row_off"], cat["row_ids"], r["node"], L, old_level, level,
                                     hierarchical=hier, min_level=r["min_level"], use_mask=use_mask)
    px = r["pairs"]
    ref_logits = odin.forward(px["codes"], px["seqs"], jtm_ref.pad_flat(px["mask"]))
    bound = jtm_ref.chain_sum(ATOL + RTOL * np.abs(ref_logits.astype(np.float64)), cat["row_off"], level - old_level)
    seen = np.diff(cat["row_off"]) > 0
    for name in ("cached", "uncached"):
        err = np.abs(r[name].astype(np.float64) - w_ref.astype(np.float64))
        print("%s %s: max |w - oracle| = %.3g, max err / bound = %.3g, max |w| = %.3g" % (_id(case), name, err[seen].max(), (err[seen] / bound[seen]).max(),
                                                                                          np.abs(w_ref[seen]).max()))
        assert (r[name][~seen] == w_ref[~seen]).all() and (err[seen] <= bound[seen]).all()


class _MaxPairs:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        os.environ["DM_JTM_MAX_PAIRS"] = str(self.v)

    def __exit__(self, *a):
        del os.environ["DM_JTM_MAX_PAIRS"]


@pytest.mark.parametrize("old_level,level", [(4, 6), (2, 7)])
@pytest.mark.parametrize("cap", ["5nchain", "1"])
def test_chunked_scoring_equals_unchunked(old_level, level, cap):
    """(c): DM_JTM_MAX_PAIRS = 5 * nchain (items of 2 .. 5 rows share chunks, chunks grow and shrink, the 40-row item alone exceeds the
    cap) and = 1 (one item per chunk): every path, hierarchical (expand kernel on the cached arrays) included, bit for bit."""
    E, L = 32, 10
    eng, cat = _engine(E), _cat(L)
    n = cat["items"].size
    cap = 5 * jtm_ref.nchain_of(level - old_level) if cap == "5nchain" else 1
    for hier in (False, True):
        if hier and (old_level, level) != (4, 6):
            continue
        min_level = 5 if hier else 0
        node = jtm_ref.ancestor_at_level(cat["item_code"], old_level).astype(np.int32)
        whole = _case(E, "auto", L, old_level, level, True, False) if not hier else _all_device_paths(eng, cat, L, node, old_level, level, True, min_level, True)
        with _MaxPairs(cap):
            got = _all_device_paths(eng, cat, L, node, old_level, level, hier, min_level, True)
        for name in ("uncached", "cached", "ranges"):
            assert np.array_equal(got[name], whole[name]), (name, hier)
        assert np.array_equal(whole["cached"], whole["uncached"])


@pytest.mark.parametrize("old_level,level", [(4, 6), (2, 7)])
def test_chunked_resident_step_equals_unchunked_and_the_host_rebalance(old_level, level):
    """(c): dm_jtm_step_cached keeps the weight matrix in HBM and writes chunk i0's weights at d_weights_all + i0 * nchild; its only
    observable is the assignment."""
    N, lib = _lib()
    E, L = 32, 10
    eng, cat = _engine(E), _cat(L)
    n = cat["items"].size
    node = jtm_ref.ancestor_at_level(cat["item_code"], old_level).astype(np.int32)
    old_node = jtm_ref.ancestor_at_level(cat["item_code"], level).astype(np.int32)
    max_assign = 1 << (DEPTH - level)
    w = _case(E, "auto", L, old_level, level, True, False)["cached"]

    def step():
        out = np.full(n, -7, np.int32)
        eng._chk(lib.dm_jtm_step_cached(eng._h, _ptr(node, N.i32p), _ptr(old_node, N.i32p), n, old_level, level, 0, 0, 1, max_assign, _ptr(out, N.i32p)))
        return out
    _cache(eng, cat, L)
    try:
        whole = step()
        chunked = []
        for cap in (5 * jtm_ref.nchain_of(level - old_level), 1):
            with _MaxPairs(cap):
                chunked.append(step())
    finally:
        _uncache(eng, L)
    os.environ["DM_JTM_REBALANCE"] = "host"
    try:
        host = np.full(n, -7, np.int32)
        eng._chk(lib.dm_jtm_rebalance_all(eng._h, _ptr(w, N.f32p), _ptr(old_node, N.i32p), _ptr(node, N.i32p), n, old_level, level, max_assign, _ptr(host, N.i32p)))
    finally:
        del os.environ["DM_JTM_REBALANCE"]
    first = (node.astype(np.int64) << (level - old_level)) + (1 << (level - old_level)) - 1
    assert ((host >= first) & (host < first + (1 << (level - old_level))) | (host == node)).all() and (host != old_node).any()
    assert np.array_equal(whole, host)
    for c in chunked:
        assert np.array_equal(c, whole)


@pytest.mark.parametrize("f64", [True, False])
def test_otm_chunked_scoring_equals_unchunked(f64):
    """(c): dm_otm_child_weights (histories of node codes, double sums on the host) through the same knob.  The f64 case is the one that
    found the per-chunk kernel choice: chunks below 256 pairs took the one-wave-per-row kernel, larger ones the matrix-pipe forward, and the
    weights moved by 2.8e-17 with the chunk size; the kernel is now chosen for the whole call (din_forward_t: B_request)."""
    N, lib = _lib()
    E, L, old_level, level = 32, 10, 4, 6
    eng, cat = _engine(E, f64=f64), _cat(L)
    n = cat["items"].size
    node = jtm_ref.ancestor_at_level(cat["item_code"], old_level).astype(np.int32)
    row_codes, _, bad = jtm_ref.id_to_code_with_mask(cat["row_ids"], cat["id_to_code"], cat["non_leaf_offset"], cat["max_code"], num_index=NI)
    assert not bad.any()
    row_codes = np.ascontiguousarray(row_codes)

    def run():
        w = np.full((n, 1 << (level - old_level)), np.nan, np.float64)
        eng._chk(lib.dm_otm_child_weights(eng._h, _ptr(cat["row_off"], N.i64p), _ptr(row_codes, N.i32p), _ptr(node, N.i32p), n, L, old_level, level, 1,
                                          _ptr(w, C.POINTER(C.c_double))))
        return w
    whole = run()
    seen = np.diff(cat["row_off"]) > 0
    assert np.isfinite(whole).all() and (whole[~seen] == -1e6).all() and len(np.unique(whole[seen])) > seen.sum()
    for cap in (5 * jtm_ref.nchain_of(level - old_level), 1):
        with _MaxPairs(cap):
            got = run()
        assert np.array_equal(got, whole), (cap, np.abs(got - whole).max())
    if not f64:           # the f32 model's logits are din_forward's; OTM masks EVERY position that holds -1, the id beyond max_code included
        gap = level - old_level
        px = jtm_ref.expand_pairs(cat["row_off"], cat["row_ids"], node, L, old_level, level, cat["id_to_code"], cat["non_leaf_offset"], cat["max_code"],
                                  num_index=NI)
        logits = eng.din_forward(px["codes"], px["seqs"], jtm_ref.pad_flat(px["seqs"] == -1), L=L)
        diff = np.abs(whole - jtm_ref.chain_sum(logits, cat["row_off"], gap))[seen]
        assert (diff <= 1e-13 * jtm_ref.chain_sum(np.abs(logits), cat["row_off"], gap)[seen]).all()      # double sums of < 100 terms, any order


def test_invalid_max_pairs_falls_back_to_the_default():
    E, L = 32, 10
    eng, cat = _engine(E), _cat(L)
    r = _case(E, "auto", L, 4, 6, True, False)
    for v in ("0", "-3", "12x", ""):
        with _MaxPairs(v):
            assert np.array_equal(_uncached(eng, cat, L, r["node"], 4, 6, False, 0, True), r["uncached"])


def test_a_hole_of_the_id_map_is_an_index_error_and_is_not_cached():
    """(d): an id below non_leaf_offset that is no leaf item: the reference's lookup fails; the library answers DM_ERR_INDEX, and again on
    a retry, because the per-row codes built with that position cleared were dropped."""
    N, lib = _lib()
    E, L, old_level, level = 32, 10, 4, 6
    eng, cat = _engine(E), _cat(L)
    n = cat["items"].size
    good = _case(E, "auto", L, old_level, level, True, False)
    node = good["node"]
    bad_cat = dict(cat, row_ids=cat["row_ids"].copy())
    bad_cat["row_ids"][int(cat["row_off"][n // 2]) + 9, 3] = cat["hole_ids"][0]
    msg = b"history code outside the embedding table"
    assert _uncached(eng, bad_cat, L, node, old_level, level, False, 0, True, check=False) == DM_ERR_INDEX and msg in lib.dm_last_error(eng._h)
    _cache(eng, bad_cat, L)
    try:
        for _ in range(2):
            assert _cached(eng, node, 0, n, old_level, level, False, 0, True, check=False) == DM_ERR_INDEX and msg in lib.dm_last_error(eng._h)
        _cache(eng, cat, L)
        assert np.array_equal(_cached(eng, node, 0, n, old_level, level, False, 0, True), good["ref"])
    finally:
        _uncache(eng, L)
