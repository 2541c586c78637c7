"""Edges of the JTM / OTM greedy re-balance (csrc/jtm_rebalance_dev.hip.inc, jtm_host.hip.inc) that the parity cases of
tests/test_gpu_edges.py reach incidentally or never: the same three-way comparison — device == host (DM_JTM_REBALANCE=host) item
for item, both == the oracle's reBalance parent by parent — on inputs made by tests/sort_ref.py, whose properties
tests/test_dev_sort_host.py proves on the CPU.  float weights go through dm_jtm_rebalance_all, double ones through
dm_otm_rebalance_all."""
import ctypes as C
import os

import numpy as np
import pytest

import sort_ref as S
from dismember_amd import Engine
from dismember_amd import _native as N

pytestmark = pytest.mark.gpu

f64p = C.POINTER(C.c_double)


def live():
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def call_all(eng, mode, w, old_node, item_node, n, old_level, level, max_assign, out):
    """dm_jtm_rebalance_all (float32 weights) / dm_otm_rebalance_all (float64) on the device route or with DM_JTM_REBALANCE=host"""
    f64 = w.dtype == np.float64
    fn = N.lib().dm_otm_rebalance_all if f64 else N.lib().dm_jtm_rebalance_all
    os.environ["DM_JTM_REBALANCE"] = mode
    try:
        return fn(eng._h, w.ctypes.data_as(f64p if f64 else N.f32p), old_node.ctypes.data_as(N.i32p), item_node.ctypes.data_as(N.i32p),
                  n, old_level, level, max_assign, out.ctypes.data_as(N.i32p))
    finally:
        del os.environ["DM_JTM_REBALANCE"]


def both_routes(eng, c):
    outs = {}
    for mode in ("device", "host"):
        out = np.full(c["n"], -99, np.int32)
        eng._chk(call_all(eng, mode, c["w"], c["old_node"], c["item_node"], c["n"], c["old_level"], c["level"], c["max_assign"], out))
        outs[mode] = out
    assert np.array_equal(outs["device"], outs["host"]), (c["name"], c["f64"], int((outs["device"] != outs["host"]).sum()))
    return outs["device"]


def oracle_parent(oracle, c, idx, p):
    """the oracle's reBalance for the items idx (in item order) of parent p -> new codes, p where the item is dropped"""
    w, old_node = c["w"][idx], c["old_node"][idx]
    if not c["f64"]:
        r = np.asarray(oracle.jtm_rebalance(np.arange(idx.size, dtype=np.int32), w, old_node, int(p), c["old_level"], c["level"], c["max_assign"]))
    else:
        from oracle import otm_tree_oracle as oto
        children = oto.get_children_at_level(int(p), c["old_level"], c["level"])
        cand = {i: oto.sort_node_weights(w[i].tolist(), children) for i in range(idx.size)}
        node_items = {}
        for i in range(idx.size):
            node_items.setdefault(cand[i][0][0], []).append((i, cand[i][0][1], 1))
        res = oto.re_balance(node_items, {i: int(old_node[i]) for i in range(idx.size)}, children, c["max_assign"], cand)
        r = np.full(idx.size, -1, np.int64)
        for child, lst in res.items():
            for it, _, _ in lst:
                r[it] = child
    return np.where(r >= 0, r, p)


def check_against_oracle(oracle, c, out, max_parents=None):
    """every occupied parent of the level, lowest code first, or the first max_parents of them"""
    inl = S.in_level(c)
    parents = np.unique(c["item_node"][inl])
    for p in parents[:max_parents]:
        idx = np.flatnonzero(c["item_node"] == p)
        ref = oracle_parent(oracle, c, idx, p)
        assert np.array_equal(out[idx], ref), (c["name"], c["f64"], int(p), int((out[idx] != ref).sum()))
    return parents.size


def child_counts(c, out):
    """items per child code of the new level, over the items that were placed"""
    first = (1 << c["level"]) - 1
    placed = out[S.in_level(c) & (out != c["item_node"])].astype(np.int64)
    assert ((placed >= first) & (placed < first + (1 << c["level"]))).all()
    return np.bincount(placed - first)


@pytest.mark.parametrize("f64", [False, True])
def test_wide_keys(eng, oracle, f64):
    """continuous weights over the whole exponent range with ±Inf, ±denormals, ±0.0 and NaNs of both signs and many payloads: every
    byte of the weight key varies among the sorted items, so a wrong rank in any digit pass moves somebody.  The oracle checks all
    eight parents."""
    c = S.rebalance_case("wide_keys", f64)
    out = both_routes(eng, c)
    check_against_oracle(oracle, c, out)
    assert child_counts(c, out).max() <= c["max_assign"]


@pytest.mark.parametrize("f64", [False, True])
def test_cap_zero(eng, oracle, f64):
    """max_assign = 0: every list is over-full in every round, everybody is handed on until no child is left and keeps the old node"""
    c = S.rebalance_case("cap_zero", f64)
    out = both_routes(eng, c)
    assert np.array_equal(out, c["item_node"])
    check_against_oracle(oracle, c, out)


def test_cap_huge(eng, oracle):
    """max_assign = n: no list is over-full, no round runs, every item takes its first choice (the first of equally heavy children)"""
    c = S.rebalance_case("cap_huge")
    out = both_routes(eng, c)
    want = (c["item_node"].astype(np.int64) << c["gap"]) + c["C"] - 1 + S.first_choice(c["w"])
    assert np.array_equal(out, want)
    check_against_oracle(oracle, c, out)


@pytest.mark.parametrize("n", [4096, 4097])
def test_threshold(eng, oracle, n):
    """the first two sizes on the device route: one full tile, and one tile plus one element"""
    c = S.rebalance_case("threshold_%d" % n)
    assert c["n"] == n
    out = both_routes(eng, c)
    check_against_oracle(oracle, c, out)
    assert child_counts(c, out).max() <= c["max_assign"]


@pytest.mark.parametrize("f64", [False, True])
def test_outside_level(eng, oracle, f64):
    """a tenth of the items sit in nodes of levels 2, 3 and 5 or at negative codes: they take no part and keep their entry on both
    routes; the items of the level equal the oracle run on them alone, for all sixteen parents"""
    c = S.rebalance_case("outside_level", f64)
    out = both_routes(eng, c)
    outside = ~S.in_level(c)
    assert np.array_equal(out[outside], c["item_node"][outside])
    check_against_oracle(oracle, c, out)
    assert child_counts(c, out).max() <= c["max_assign"]


def test_deep_sparse(eng, oracle):
    """old_level 21: the parent index fills key bits 33 .. 53 (end bit 54), 200 of the 2^21 parents are occupied and the choose
    kernel's grid-stride loop makes a second trip.  The oracle checks the 40 lowest occupied parents, host == device the rest."""
    c = S.rebalance_case("deep_sparse")
    out = both_routes(eng, c)
    assert check_against_oracle(oracle, c, out, 40) == S.DEEP_SPARSE_PARENTS
    assert child_counts(c, out).max() <= c["max_assign"]
    assert (out == c["item_node"]).any()                    # slack 1.0 over unevenly filled parents: somebody was dropped


def test_many_tiles(eng, oracle):
    """4.2 M items over 1 024 parents: the compaction scans more than 1 024 tiles and round 1 sorts about 3.5 M items, more than 256
    tiles, inside the real caller.  The oracle checks the first 40 parents, host == device the rest."""
    c = S.rebalance_case("many_tiles")
    out = both_routes(eng, c)
    assert check_against_oracle(oracle, c, out, 40) == c["P"]
    assert child_counts(c, out).max() <= c["max_assign"]


@pytest.mark.parametrize("old_level,level", [(24, 31), (23, 31)])
def test_levels_above_30_are_refused(eng, old_level, level):
    """level-31 codes do not fit the int32 of the outputs: every route refuses by name, before it allocates"""
    n, Cn = 4096, 1 << (level - old_level)
    rng = np.random.default_rng(level - old_level)
    item_node = np.full(n, (1 << old_level) - 1, np.int32)
    old_node = np.zeros(n, np.int32)
    before = live()
    for dtype in (np.float32, np.float64):
        w = rng.standard_normal((n, Cn)).astype(dtype)
        for mode in ("device", "host"):
            out = np.full(n, -99, np.int32)
            assert call_all(eng, mode, w, old_node, item_node, n, old_level, level, 16, out) == -1
            msg = N.lib().dm_last_error(eng._h).decode()
            assert "level %d" % level in msg and ("otm" if dtype == np.float64 else "jtm") in msg, msg
            assert (out == -99).all() and live() == before
    out = np.full(n, -99, np.int32)
    w32 = rng.standard_normal((n, Cn)).astype(np.float32)
    w64 = w32.astype(np.float64)
    assert N.lib().dm_jtm_rebalance(eng._h, w32.ctypes.data_as(N.f32p), old_node.ctypes.data_as(N.i32p), n, int(item_node[0]), old_level, level,
                                    16, out.ctypes.data_as(N.i32p)) == -1
    assert N.lib().dm_otm_rebalance(eng._h, w64.ctypes.data_as(f64p), old_node.ctypes.data_as(N.i32p), n, int(item_node[0]), old_level, level,
                                    16, out.ctypes.data_as(N.i32p)) == -1
    assert (out == -99).all() and live() == before


@pytest.mark.parametrize("last_parent", [True, False])
def test_level_30_is_accepted(eng, oracle, last_parent):
    """the last level whose codes fit: eight items under the last (or first) parent of level 29, host route (the device route starts
    at 4 096 items; a level this sparse is grouped by a sort of the eight items, not by a table over its 2^29 nodes), so nothing
    large is allocated.  Under the last parent the new codes reach 2^31 - 2."""
    old_level, level, n, Cn = 29, 30, 8, 2
    rng = np.random.default_rng(int(last_parent))
    p = (1 << (old_level + 1)) - 2 if last_parent else (1 << old_level) - 1
    c = dict(name="level_30", f64=False, w=S.recipe_weights(rng, n, Cn), item_node=np.full(n, p, np.int32), n=n, old_level=old_level, level=level,
             gap=1, C=Cn, P=1 << old_level, lo=(1 << old_level) - 1, max_assign=n // Cn)
    c["old_node"] = ((np.int64(p) << 1) + Cn - 1 + rng.integers(0, Cn, n)).astype(np.int32)
    for f64 in (False, True):
        c["f64"], c["w"] = f64, c["w"].astype(np.float64 if f64 else np.float32)
        out = np.full(n, -99, np.int32)
        assert call_all(eng, "host", c["w"], c["old_node"], c["item_node"], n, old_level, level, c["max_assign"], out) == 0
        assert np.array_equal(out, oracle_parent(oracle, c, np.arange(n), p))
        # capacity 4 + 4 for eight items: both children are full, so the last code of the level is in use
        assert np.bincount(out.astype(np.int64) - 2 * p - 1).tolist() == [4, 4] and (not last_parent or out.max() == (1 << 31) - 2)
