"""Per-level existence bounds of the one-wave-per-SIMD beam kernel (DM_LEVEL_BOUNDS, csrc/dm_hip.hip: dm_level_bounds_bits).

Where the existing codes of a tree level are a contiguous prefix of the level's code range, the kernel's expand and its initial
frontier answer "does this child exist" with a compare against the level's largest code instead of a load from the existence
bitmap, and where every child of the beam exists they skip the ordered compaction.  Both are the same function of the tree, so a
search must return the same bits either way: every case runs once with DM_LEVEL_BOUNDS=1 and once with =0 on the same engine (the
knob is read per call) and ids, scores, counts and every level of the trace are compared with array_equal.

Shapes: depth-10 trees and 1 500 users, so that each of the 1 024 waves of a launch takes more than one user and state left by the
previous user would show.  E = 128 with L = 10 (the hand-placed folded tile) and L = 12 (unfolded), E = 32 with L = 4 (the generic
tile).  Beams: 200 (25 tiles), 24 (48 children: two head tiles and an odd one), 8 (one tile), 3 (fewer children than a tile).

The bounds function itself needs no device: it is checked against a numpy restatement on the same trees plus one with an empty level.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import random_din_weights, random_histories

DEPTH, U = 10, 1500
FIRST = (1 << DEPTH) - 1
NI = (1 << (DEPTH + 1)) - 1
CASES = [(128, 10), (128, 12), (32, 4)]          # (E, L): FOLD, unfolded, generic tile
BEAMS = [200, 24, 8, 3]
N_BOUNDS, USE_BITS = 32, -2                      # DM_N_LEVEL_BOUNDS, DM_LEVEL_USE_BITS (csrc/beam_kernel.hip.inc)


def _tree_from_leaves(rng, leaf_codes, max_level=DEPTH):
    """The tree whose leaves are `leaf_codes` (any level) and whose inner nodes are their ancestors; ids as helpers.synthetic_tree."""
    leaf_codes = np.array(sorted(set(int(c) for c in leaf_codes)), dtype=np.int64)
    present = set(leaf_codes.tolist())
    c = leaf_codes
    while c.size and c.max() > 0:
        c = np.unique((c[c > 0] - 1) >> 1)
        present.update(c.tolist())
    inner = present - set(leaf_codes.tolist())
    assert not any(((l - 1) >> 1) in set(leaf_codes.tolist()) for l in leaf_codes if l > 0), "a leaf below a leaf"
    codes = np.array(sorted(present), dtype=np.int32)
    leaf_ids = (rng.permutation(leaf_codes.size) + 1).astype(np.int32)
    off = int(leaf_ids.max()) + 1
    lut = {int(cc): int(i) for cc, i in zip(leaf_codes, leaf_ids)}
    ids = np.array([lut.get(int(cc), int(cc) + off) for cc in codes], dtype=np.int32)
    is_leaf = np.array([int(cc) not in inner for cc in codes], dtype=np.uint8)
    return dict(codes=codes, ids=ids, is_leaf=is_leaf, leaf_ids=leaf_ids, leaf_codes=leaf_codes.astype(np.int32), max_level=np.int32(max_level))


def _leaves(name):
    rng = np.random.default_rng(77)
    if name == "prefix700":          # children missing on the deepest levels: the scan under the range test, a head tile with a missing child
        return np.arange(FIRST, FIRST + 700)
    if name == "complete":           # the identity path on every level including the last
        return np.arange(FIRST, FIRST + 1024)
    if name == "single":             # almost everything absent; every level is the one-node prefix
        return np.array([FIRST])
    if name == "single_mid":         # ... and the same with a leaf whose ancestors are not the first of their levels: bits below level 1
        return np.array([FIRST + 300])
    if name == "scattered":          # a whole level-7 subtree and scattered leaves missing: levels 7 .. 10 have gaps, 0 .. 6 are complete
        keep = rng.random(1024) >= 0.1
        keep[8 * 37:8 * 38] = False
        keep[:8] = True
        return FIRST + np.flatnonzero(keep)
    if name == "leaf_above":         # a leaf on level 8 (the last node of its level): leaves_at_max_only is false, every level keeps a bound
        lv8 = (1 << 8) - 1 + 174
        return np.concatenate([np.arange(FIRST, FIRST + 696), [lv8]])
    raise KeyError(name)


TREES = ["prefix700", "complete", "single", "single_mid", "scattered", "leaf_above"]


@functools.lru_cache(maxsize=None)
def _tree(name):
    t = _tree_from_leaves(np.random.default_rng(5 + len(name)), _leaves(name))
    for a in t.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def _bounds_ref(codes):
    """numpy restatement: per level the largest existing code if the level's codes are the run first .. last, first - 1 for an
    empty level, USE_BITS for a level with a gap; level 31 holds no int32 code."""
    codes = np.unique(np.asarray(codes, dtype=np.int64))
    out = np.empty(N_BOUNDS, np.int32)
    for l in range(N_BOUNDS):
        first = (1 << l) - 1
        lv = codes[(codes >= first) & (codes <= 2 * first)]
        if l > 30:
            out[l] = USE_BITS
        elif lv.size == 0:
            out[l] = first - 1
        else:
            out[l] = lv.max() if lv.size == lv.max() - first + 1 else USE_BITS
    return out


def _bounds_lib(codes):
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_level_bounds
    fn.restype, fn.argtypes = C.c_int, [N.i32p, C.c_int64, N.i32p]
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    out = np.full(N_BOUNDS, 12345, np.int32)
    assert fn(codes.ctypes.data_as(N.i32p), codes.size, out.ctypes.data_as(N.i32p)) == 0
    return out


@pytest.mark.parametrize("name", TREES)
def test_bounds_function_matches_numpy(name):
    codes = _tree(name)["codes"]
    got, want = _bounds_lib(codes), _bounds_ref(codes)
    assert np.array_equal(got, want), (got, want)
    # what the kernel relies on: with a bound, "exists" is the compare
    present = set(codes.tolist())
    for l in range(DEPTH + 2):
        if got[l] != USE_BITS:
            first = (1 << l) - 1
            assert all((c in present) == (c <= got[l]) for c in range(first, 2 * first + 1))


def test_bounds_function_empty_level_gap_and_order():
    # level 2 is empty although level 3 has nodes (codes need not form a heap); duplicates and any order are fine
    codes = np.array([7, 0, 2, 1, 9, 7, 8], dtype=np.int32)
    got = _bounds_lib(codes)
    assert np.array_equal(got, _bounds_ref(codes))
    assert got[0] == 0 and got[1] == 2 and got[2] == 2 and got[3] == 9 and got[4] == 14 and got[31] == USE_BITS
    codes = np.array([7, 9, 0], dtype=np.int32)
    got = _bounds_lib(codes)
    assert np.array_equal(got, _bounds_ref(codes)) and got[3] == USE_BITS and got[1] == 0
    # a level filled to its last code, and the deepest level an int32 code can sit on
    codes = np.array([3, 4, 5, 6, 2 ** 31 - 2, 2 ** 30 - 1], dtype=np.int32)
    got = _bounds_lib(codes)
    assert np.array_equal(got, _bounds_ref(codes)) and got[2] == 6 and got[30] == USE_BITS and got[29] == 2 ** 29 - 2


# ---------------------------------------------------------------- the kernel: DM_LEVEL_BOUNDS=1 against =0, bit for bit

@functools.lru_cache(maxsize=None)
def _weights(E, L):
    w = random_din_weights(np.random.default_rng(4200 + E + L), E, NI, bias_std=0.01)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _seqs(name, L):
    seqs = random_histories(np.random.default_rng(300 + L), _tree(name)["leaf_ids"], U, L, unknown_prob=0.03)
    seqs.setflags(write=False)
    return seqs


@pytest.fixture(scope="module")
def engines():
    from dismember_amd import Engine
    made = {}

    def get(E, L, name):
        if (E, L, name) not in made:
            t = _tree(name)
            eng = Engine(0)
            eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
            eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
            eng.load_weights_din(_weights(E, L), E, NI)
            eng.set_scorer_mode("split_f16")
            made[(E, L, name)] = eng
        return made[(E, L, name)]
    yield get
    for e in made.values():
        e.close()


NAMES = ("ids", "scores", "counts", "trace_codes", "trace_scores", "trace_counts")


def _assert_equal(got, want, what):
    bad = [n for n, a, b in zip(NAMES, got, want) if not (a.dtype == b.dtype and np.array_equal(a, b))]
    assert not bad, "%s: differs in %s" % (what, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TREES)
@pytest.mark.parametrize("beam", BEAMS)
@pytest.mark.parametrize("E,L", CASES)
def test_bounds_against_bits(engines, monkeypatch, E, L, beam, name):
    eng = engines(E, L, name)
    seqs = _seqs(name, L)
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("DM_LEVEL_BOUNDS", knob)
        out[knob] = eng.tdm_beam_search_trace(seqs, beam, 10, max_levels=DEPTH + 2)
        assert eng.last_beam_kernel().startswith("dm_beam_w_kernel<%d" % E), eng.last_beam_kernel()
    assert out["1"][2].sum() > 0 and out["1"][5].sum() > 0, "the search returned nothing: the comparison would be empty"
    _assert_equal(out["1"], out["0"], "DM_LEVEL_BOUNDS=1 against =0 (E %d, L %d, beam %d, tree %s)" % (E, L, beam, name))
    monkeypatch.delenv("DM_LEVEL_BOUNDS")
    _assert_equal(eng.tdm_beam_search_trace(seqs, beam, 10, max_levels=DEPTH + 2), out["0"], "DM_LEVEL_BOUNDS unset against =0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prefix700", "scattered", "leaf_above"])
@pytest.mark.parametrize("E,L", CASES)
def test_widened_beams_start_on_their_own_level(engines, monkeypatch, E, L, name):
    """widen_consumed: a user's beam is max(beam, (consumed + topk) / 2), so the users of one launch start on levels 3 .. 5."""
    eng = engines(E, L, name)
    seqs = _seqs(name, L)
    rng = np.random.default_rng(11)
    leaf_ids = _tree(name)["leaf_ids"]
    consumed = [rng.choice(leaf_ids, size=int(n)) for n in rng.choice([0, 3, 14, 30, 61, 100], size=U)]
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("DM_LEVEL_BOUNDS", knob)
        out[knob] = eng.tdm_beam_search(seqs, 8, 10, consumed=consumed, widen_consumed=True)
        assert eng.last_beam_kernel().startswith("dm_beam_w_kernel<%d" % E), eng.last_beam_kernel()
    assert out["1"][2].sum() > 0
    _assert_equal(out["1"], out["0"], "widened beams, DM_LEVEL_BOUNDS=1 against =0 (E %d, L %d, tree %s)" % (E, L, name))
