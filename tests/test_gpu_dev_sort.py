"""The device primitives of csrc/dev_sort.hip.inc on their own, through the debug entries dm_debug_sort_pairs and
dm_debug_select_flagged, against the numpy restatements of tests/sort_ref.py.  Every comparison is exact.  The sizes reach what no
caller reaches under pytest: a second and third chunk of the sort's digit scan (> 256 and > 512 tiles) and of the compaction's scan
(> 1 024 and > 2 048 tiles); tests/test_dev_sort_host.py proves these properties of the inputs on the CPU."""
import ctypes as C

import numpy as np
import pytest

import sort_ref as S
from dismember_amd import Engine
from dismember_amd import _native as N

pytestmark = pytest.mark.gpu

u64p = C.POINTER(C.c_uint64)
SENTINEL32, SENTINEL64 = np.int32(-123456789), np.uint64(0xDEAD_BEEF_F00D_CAFE)


def _fns():
    L = N.lib()
    s, f = L.dm_debug_sort_pairs, L.dm_debug_select_flagged
    s.restype = f.restype = C.c_int
    s.argtypes = [C.c_void_p, u64p, N.i32p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int)]
    f.argtypes = [C.c_void_p, N.i32p, u64p, N.u8p, C.c_int64, N.i32p, u64p, u64p]
    return s, f


def live():
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def sort_pairs(eng, keys, vals, begin, end):
    k, v, where = keys.copy(), vals.copy(), C.c_int(-5)
    assert _fns()[0](eng._h, _ptr(k, u64p), _ptr(v, N.i32p), k.size, begin, end, C.byref(where)) == 0
    return k, v, where.value


def check_sort(eng, keys, begin, end, tag):
    vals = np.arange(keys.size, dtype=np.int32)
    k, v, where = sort_pairs(eng, keys, vals, begin, end)
    rk, rv = S.sort_ref(keys, vals, begin, end)
    assert np.array_equal(k, rk), (tag, "keys", int((k != rk).sum()))
    assert np.array_equal(v, rv), (tag, "vals", int((v != rv).sum()))
    # the pair that holds the result: the parity of the passes run, ceil(bits / 8) & 1 — and pair 0, the input, where no pass runs
    # (an empty bit range; fewer than two elements, which dev_radix_sort_pairs returns as they are)
    assert where == S.passes(keys.size, begin, end) & 1, (tag, where)
    return k, v


@pytest.mark.parametrize("m", S.SMALL_SIZES)
def test_sort_small_sizes_every_range_and_distribution(eng, m):
    """0 .. 3 tiles + 1: the wave, round and tile edges, at every bit range (one partial pass, odd and even pass counts, non-zero
    begin, the re-balance's own ranges, no pass at all) and every key distribution; vals = arange, so the sorted vals ARE the
    permutation and "equal" / "eight" check stability across lanes, waves, rounds and tiles"""
    for dist in S.SORT_DISTS:
        keys = S.sort_keys(dist, m)
        for begin, end in S.SORT_RANGES:
            k, v = check_sort(eng, keys, begin, end, (dist, m, begin, end))
            if dist == "equal" or end == begin:
                assert np.array_equal(v, np.arange(m)) and np.array_equal(k, keys), (dist, m, begin, end)


@pytest.mark.parametrize("dist", S.SORT_DISTS)
@pytest.mark.parametrize("begin,end", S.SORT_BIG_RANGES)
@pytest.mark.parametrize("m", S.SORT_BIG_SIZES)
def test_sort_more_than_one_chunk_of_the_digit_scan(eng, m, begin, end, dist):
    """257 and 513 tiles: dsort_digit_scan_kernel walks a digit's row in two and three chunks of 256 tiles, the carry between them
    is part of every later tile's offset"""
    keys = S.sort_keys(dist, m)
    k, v = check_sort(eng, keys, begin, end, (dist, m, begin, end))
    if dist == "equal":
        assert np.array_equal(v, np.arange(m))


@pytest.mark.parametrize("m", [4097, 257 * 4096 + 5])
def test_sort_is_deterministic(eng, m):
    keys = S.sort_keys("eight", m, seed=3)
    vals = np.random.default_rng(m).integers(-(1 << 31), 1 << 31, m).astype(np.int32)      # any payload, negative ones included
    a, b = sort_pairs(eng, keys, vals, 0, 64), sort_pairs(eng, keys, vals, 0, 64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    rk, rv = S.sort_ref(keys, vals, 0, 64)
    assert np.array_equal(a[0], rk) and np.array_equal(a[1], rv)


def select(eng, flag, inp, in2):
    n = flag.size
    out = np.full(n, SENTINEL32, np.int32)
    out2 = None if in2 is None else np.full(n, SENTINEL64, np.uint64)
    count = C.c_uint64(1 << 40)
    assert _fns()[1](eng._h, _ptr(inp, N.i32p), _ptr(in2, u64p), _ptr(flag, N.u8p), n, _ptr(out, N.i32p), _ptr(out2, u64p), C.byref(count)) == 0
    return out, out2, int(count.value)


def check_select(eng, flag, inp, in2, tag):
    r1, r2, rc = S.select_ref(flag, inp, in2)
    for a, b in ((inp, in2), (None, in2), (inp, None), (None, None)):        # `in` given / the indices, with and without `in2`
        out, out2, count = select(eng, flag, a, b)
        form = tag + ("in" if a is not None else "indices", "in2" if b is not None else "-")
        assert count == rc, (form, count, rc)
        want = r1 if a is not None else np.flatnonzero(flag).astype(np.int32)
        assert np.array_equal(out[:count], want), (form, int((out[:count] != want).sum()))
        assert (out[count:] == SENTINEL32).all(), form                        # nothing is written past the count
        if b is not None:
            assert np.array_equal(out2[:count], r2), (form, int((out2[:count] != r2).sum()))
            assert (out2[count:] == SENTINEL64).all(), form


@pytest.mark.parametrize("n", S.SMALL_SIZES)
def test_select_small_sizes_every_flag_pattern_and_form(eng, n):
    inp, in2 = S.select_inputs(n)
    for kind in S.SELECT_FLAGS:
        check_select(eng, S.select_flags(kind, n), inp, in2, (kind, n))


@pytest.fixture(scope="module")
def big_inputs():
    return {n: S.select_inputs(n) for n in S.SELECT_BIG_SIZES}


@pytest.mark.parametrize("kind", S.SELECT_FLAGS)
@pytest.mark.parametrize("n", S.SELECT_BIG_SIZES)
def test_select_more_than_one_chunk_of_the_tile_scan(eng, big_inputs, n, kind):
    """1 025 and 2 049 tiles: dsort_scan_kernel scans the per-tile counts in two and three chunks of 1 024 with a running carry"""
    inp, in2 = big_inputs[n]
    check_select(eng, S.select_flags(kind, n), inp, in2, (kind, n))


def test_argument_errors_leave_the_outputs_untouched(eng):
    sort, sel = _fns()
    keys = S.sort_keys("uniform", 100)
    vals = np.arange(100, dtype=np.int32)
    k, v, where = keys.copy(), vals.copy(), C.c_int(-5)
    kp, vp, wp = _ptr(k, u64p), _ptr(v, N.i32p), C.byref(where)
    for args in ((None, kp, vp, 100, 0, 64, wp), (eng._h, None, vp, 100, 0, 64, wp), (eng._h, kp, None, 100, 0, 64, wp),
                 (eng._h, kp, vp, 100, 0, 64, None), (eng._h, kp, vp, -1, 0, 64, wp), (eng._h, kp, vp, 1 << 31, 0, 64, wp),
                 (eng._h, kp, vp, 100, -1, 8, wp), (eng._h, kp, vp, 100, 9, 8, wp), (eng._h, kp, vp, 100, 0, 65, wp),
                 (eng._h, kp, vp, 100, 64, 65, wp)):
        assert sort(*args) == -1, args[3:6]
        assert np.array_equal(k, keys) and np.array_equal(v, vals) and where.value == -5
    flag = S.select_flags("half", 100)
    inp, in2 = S.select_inputs(100)
    out, out2, count = np.full(100, SENTINEL32, np.int32), np.full(100, SENTINEL64, np.uint64), C.c_uint64(77)
    ip, i2p, fp, op, o2p, cp = _ptr(inp, N.i32p), _ptr(in2, u64p), _ptr(flag, N.u8p), _ptr(out, N.i32p), _ptr(out2, u64p), C.byref(count)
    for args in ((None, ip, i2p, fp, 100, op, o2p, cp), (eng._h, ip, i2p, None, 100, op, o2p, cp), (eng._h, ip, i2p, fp, 100, None, o2p, cp),
                 (eng._h, ip, i2p, fp, 100, op, None, cp), (eng._h, ip, i2p, fp, 100, op, o2p, None), (eng._h, ip, i2p, fp, -1, op, o2p, cp),
                 (eng._h, ip, i2p, fp, 1 << 31, op, o2p, cp)):
        assert sel(*args) == -1, args[4]
        assert (out == SENTINEL32).all() and (out2 == SENTINEL64).all() and count.value == 77
    # the bounds themselves are inside: an empty range at 64, the empty input
    assert sort(eng._h, kp, vp, 100, 64, 64, wp) == 0 and where.value == 0 and np.array_equal(k, keys) and np.array_equal(v, vals)
    assert sort(eng._h, kp, vp, 0, 0, 64, wp) == 0 and where.value == 0
    assert sel(eng._h, ip, i2p, fp, 0, op, o2p, cp) == 0 and count.value == 0 and (out == SENTINEL32).all()


def test_debug_entries_leave_no_device_memory(eng):
    sort, sel = _fns()
    before = live()
    where = C.c_int(0)
    for m in (0, 1, 4097, 257 * 4096 + 5):
        sort_pairs(eng, S.sort_keys("uniform", m), np.arange(m, dtype=np.int32), 0, 64)
        inp, in2 = S.select_inputs(m)
        flag = S.select_flags("half", m)
        select(eng, flag, inp, in2)
        select(eng, flag, None, None)
    k = S.sort_keys("uniform", 10)
    assert sort(eng._h, _ptr(k, u64p), None, 10, 0, 64, C.byref(where)) == -1           # a refusal too
    assert live() == before
