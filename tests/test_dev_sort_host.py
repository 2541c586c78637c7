"""The conditions tests/test_gpu_dev_sort.py and tests/test_gpu_rebalance_edges.py put on their inputs, proved on the CPU (no GPU):
which sizes reach a second and third chunk of the two scan loops of csrc/dev_sort.hip.inc, what the key distributions hold, and what
the re-balance cases make the device sort.  Conditions, not measurements: the seeds in tests/sort_ref.py are chosen so they hold."""
import numpy as np
import pytest

import sort_ref as S


def test_references_on_hand_checked_inputs():
    keys = np.array([0x0300, 0x0101, 0x0200, 0x8000_0000_0000_0001, 0x0100], np.uint64)
    vals = np.arange(5, dtype=np.int32)
    k, v = S.sort_ref(keys, vals, 8, 16)                       # digits 3, 1, 2, 0, 1: stable, whole keys travel
    assert v.tolist() == [3, 1, 4, 2, 0] and k.tolist() == keys[[3, 1, 4, 2, 0]].tolist()
    k, v = S.sort_ref(keys, vals, 0, 64)                       # unsigned: the key with the top bit set is the greatest
    assert v.tolist() == [4, 1, 2, 0, 3]
    assert S.sort_ref(keys, vals, 7, 7)[1].tolist() == [0, 1, 2, 3, 4]
    assert [S.passes(5, b, e) & 1 for b, e in S.SORT_RANGES] == [1, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    assert S.passes(1, 0, 8) == 0 and S.passes(0, 0, 64) == 0
    flag = np.array([0, 2, 0, 255, 1], np.uint8)
    a, b, c = S.select_ref(flag, np.array([10, 11, 12, 13, 14], np.int32), np.array([5, 6, 7, 8, 9], np.uint64))
    assert a.tolist() == [11, 13, 14] and b.tolist() == [6, 8, 9] and c == 3
    assert S.select_ref(flag)[0].tolist() == [1, 3, 4] and S.select_ref(flag)[0].dtype == np.int32


def test_sizes_reach_the_chunks_they_claim():
    assert [S.tiles(m) for m in S.SMALL_SIZES] == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 4]
    assert [S.tiles(m) for m in S.SORT_BIG_SIZES] == [258, 514]          # the odd elements open one more tile
    assert [S.chunks(m, S.SORT_SCAN_CHUNK) for m in S.SORT_BIG_SIZES] == [2, 3]
    assert max(S.chunks(m, S.SORT_SCAN_CHUNK) for m in S.SMALL_SIZES) == 1
    assert [S.tiles(n) for n in S.SELECT_BIG_SIZES] == [1026, 2050]
    assert [S.chunks(n, S.SELECT_SCAN_CHUNK) for n in S.SELECT_BIG_SIZES] == [2, 3]
    assert all(m % S.TILE not in (0,) for m in S.SORT_BIG_SIZES + S.SELECT_BIG_SIZES)       # a partial last tile as well
    assert max(S.SORT_BIG_SIZES + S.SELECT_BIG_SIZES) < 1 << 31


@pytest.mark.parametrize("m", [3 * 4096 + 1] + S.SORT_BIG_SIZES)
def test_key_distributions_hold_what_they_claim(m):
    uni = S.sort_keys("uniform", m)
    assert (uni >> np.uint64(63)).any() and not (uni >> np.uint64(63)).all()        # top-bit-set keys: the order is unsigned
    for byte in range(8):
        assert np.unique((uni >> np.uint64(8 * byte)) & np.uint64(255)).size == 256
    assert np.unique(S.sort_keys("equal", m)).size == 1
    two = S.sort_keys("two_runs", m)
    a, b = np.unique(two)
    change = np.flatnonzero(two[1:] != two[:-1]) + 1
    assert np.array_equal(np.diff(change), np.full(change.size - 1, S.RUN)) and (change % S.TILE != 0).all()      # long runs, cut inside tiles
    assert np.unique(change // S.TILE).size == change.size >= 2                    # ... every run straddles a tile boundary
    xa, xb = int(a), int(b)
    sides = [((xa >> s) & 255) < ((xb >> s) & 255) for s in range(0, 64, 8)]
    assert True in sides and False in sides                                        # the two values swap sides between passes
    td = S.sort_keys("tile_digit", m)
    t = np.arange(m) // S.TILE
    for byte in (0, 2, 4, 6):                                                      # the passes at shift 0, 16, 32 and 48
        d = ((td >> np.uint64(8 * byte)) & np.uint64(255)).astype(np.int64)
        assert np.array_equal(d, S.tile_digit(t, byte))                            # one digit holds each whole tile: a count of 4 096
        assert np.unique(d[::S.TILE]).size >= min(S.tiles(m), 256) - 1             # while the tiles differ
        assert np.bincount(d[: S.TILE], minlength=256).max() == S.TILE
    for byte in (1, 3, 5, 7):
        assert np.unique((td >> np.uint64(8 * byte)) & np.uint64(255)).size == 256
    srt = S.sort_keys("sorted", m)
    rev = S.sort_keys("reversed", m)
    assert (srt[1:] >= srt[:-1]).all() and (rev[1:] <= rev[:-1]).all() and srt[0] < srt[-1] and rev[0] > rev[-1]
    e8 = S.sort_keys("eight", m)
    assert np.unique(e8).size == 8 and np.bincount(np.unique(e8, return_inverse=True)[1]).min() > m // 16


@pytest.mark.parametrize("n", [4097] + S.SELECT_BIG_SIZES)
def test_flag_patterns_hold_what_they_claim(n):
    count = {k: int(np.count_nonzero(S.select_flags(k, n))) for k in S.SELECT_FLAGS}
    assert count["none"] == 0 and count["all"] == n and count["first"] == 1 and count["last"] == 1
    assert S.select_flags("first", n)[0] and S.select_flags("last", n)[-1]
    assert abs(count["half"] - n / 2) < 4 * np.sqrt(n) and 0 < count["sparse"] < n / 300
    tr = S.select_flags("truthy", n)
    assert set(np.unique(tr).tolist()) == {0, 1, 2, 255} and abs(count["truthy"] - n / 2) < 4 * np.sqrt(n)
    if n > S.TILE * S.SELECT_SCAN_CHUNK:           # set flags in every chunk of the scan: the carry is never zero
        for k in ("half", "sparse", "truthy", "all"):
            per_tile = np.add.reduceat(S.select_flags(k, n) != 0, np.arange(0, n, S.TILE))
            assert all(per_tile[c: c + S.SELECT_SCAN_CHUNK].sum() > 0 for c in range(0, per_tile.size, S.SELECT_SCAN_CHUNK)), k


def test_asc_key_is_the_java_compare_order():
    for ft, ut in ((np.float32, np.uint32), (np.float64, np.uint64)):
        nan2 = np.array([1, 1 << 20], ut) | np.array([0x7F800000, 0xFF800000] if ft == np.float32 else [0x7FF0000000000000, 0xFFF0000000000000], ut)
        tiny = np.array([1], ut).view(ft)[0]
        w = np.array([-np.inf, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, np.inf], ft)
        k = S.asc_key(np.concatenate([w, nan2.view(ft)]))
        assert (k[1:8] > k[:7]).all() and k[8] == k[9] > k[7]                       # -0.0 < 0.0; one NaN, above +Inf
    assert S.first_choice(np.array([[1.0, 2.0, 2.0], [0.0, -0.0, -1.0], [np.nan, np.inf, 0.0]], np.float32)).tolist() == [1, 0, 0]


@pytest.mark.parametrize("f64", [False, True])
def test_wide_keys_vary_every_byte_of_the_weight_key(f64):
    c = S.rebalance_case("wide_keys", f64)
    sizes, best, sorted_items = S.round_one(c)
    assert (best >= 0).sum() >= 4 and c["n"] >= 4096                                # most parents take part in round 1, on the device
    # the keys the device sorts in round 1 alone: the processed child's weight of every item in a processed list
    p = c["item_node"].astype(np.int64) - c["lo"]
    k = S.asc_key(c["w"][sorted_items, best[p[sorted_items]]])
    nbytes = 8 if f64 else 4
    distinct = [np.unique((k >> k.dtype.type(8 * b)) & k.dtype.type(255)).size for b in range(nbytes)]
    assert min(distinct) >= 200, distinct
    w = c["w"]
    bits = w.view(np.uint64 if f64 else np.uint32)
    nan = np.isnan(w)
    assert np.isposinf(w).any() and np.isneginf(w).any() and ((w == 0) & np.signbit(w)).any() and ((w == 0) & ~np.signbit(w)).any()
    tiny = np.finfo(w.dtype).tiny
    assert ((w > 0) & (w < tiny)).any() and ((w < 0) & (w > -tiny)).any()           # denormals of both signs
    assert (nan & np.signbit(w)).any() and (nan & ~np.signbit(w)).any() and np.unique(bits[nan]).size > 100      # NaN payloads
    if f64:                                                                         # pairs that differ only below bit 32 of the key
        ka = S.asc_key(w)
        same_hi = (ka[1:] >> np.uint64(32) == ka[:-1] >> np.uint64(32)) & (ka[1:] != ka[:-1])
        assert same_hi.sum() > 1000
        both = sorted_items[1:] & sorted_items[:-1] & (p[1:] == p[:-1])             # ... and such pairs meet in one sorted segment
        assert (same_hi[np.arange(c["n"] - 1), best[p[1:]]] & both).sum() >= 100


@pytest.mark.parametrize("f64", [False, True])
def test_cap_cases_sit_on_their_side_of_every_list(f64):
    z = S.rebalance_case("cap_zero", f64)
    sizes, best, _ = S.round_one(z)
    assert z["max_assign"] == 0 and (sizes > 0).all() and (best >= 0).all()         # every list of every parent is over capacity
    h = S.rebalance_case("cap_huge", f64)
    sizes, best, items = S.round_one(h)
    assert h["max_assign"] >= h["n"] >= sizes.max() and (best == -1).all() and not items.any()       # no list is: no round at all
    assert (sizes > 0).all()


def test_threshold_cases_are_the_first_device_sizes():
    for n in (4096, 4097):
        c = S.rebalance_case("threshold_%d" % n)
        assert c["n"] == n and S.tiles(n) == (1 if n == 4096 else 2)
        assert (S.round_one(c)[1] >= 0).all()


@pytest.mark.parametrize("f64", [False, True])
def test_outside_level_has_items_on_both_sides(f64):
    c = S.rebalance_case("outside_level", f64)
    nd, lo, P = c["item_node"].astype(np.int64), c["lo"], c["P"]
    inl = S.in_level(c)
    assert 0.07 * c["n"] < (~inl).sum() < 0.13 * c["n"]
    assert ((nd >= 3) & (nd < lo)).sum() > 100 and (nd >= lo + P).sum() > 100 and 0 < (nd < 0).sum() < 10 and nd.min() == -(1 << 31)
    assert set(np.unique(nd[~inl & (nd >= 0)]).tolist()) <= set(range(3, 15)) | set(range(31, 63))
    assert np.unique(nd[inl]).size == P and (S.round_one(c)[1] >= 0).all()


def test_deep_sparse_fills_the_high_key_bits():
    c = S.rebalance_case("deep_sparse")
    p = np.unique(c["item_node"].astype(np.int64) - c["lo"])
    assert c["old_level"] == 21 and p.size == S.DEEP_SPARSE_PARENTS
    assert p.max() >= 1 << 20                                   # past the 4 096 x 256 threads of the choose kernel's first trip
    assert 33 + c["old_level"] == 54 and (p.max() << 33) >> 53 == 1        # the parent index reaches the sort's last key bit
    sizes, best, items = S.round_one(c)
    per_parent = sizes.sum(axis=1)
    assert (per_parent > c["C"] * c["max_assign"]).any()        # a parent over capacity: somebody is dropped
    assert (best >= 0).sum() > 100 and (per_parent == 0).sum() == c["P"] - S.DEEP_SPARSE_PARENTS


def test_many_tiles_runs_both_scan_loops_a_second_time():
    c = S.rebalance_case("many_tiles")
    assert c["n"] > 4_194_304 and S.chunks(c["n"], S.SELECT_SCAN_CHUNK) == 2        # the compaction runs over all n items
    sizes, best, items = S.round_one(c)
    m = int(items.sum())
    assert m > 1_048_576 and S.chunks(m, S.SORT_SCAN_CHUNK) >= 2, m                 # round 1 sorts m items
    assert (best >= 0).all() and (sizes[np.arange(c["P"]), best] == sizes.max(axis=1)).all()
    assert 0.8 < (S.first_choice(c["w"]) == 0).mean() < 0.87                        # about 5 / 6 choose child 0 first
