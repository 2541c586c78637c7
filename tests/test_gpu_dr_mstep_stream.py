"""Streaming M-step on the device (dm_dr_mstep_streaming_path_scores).  The call hands out the beams it folded (its trace);
the tests replay the fold on exactly those with oracle/dr_mstep_oracle.streaming_path_score and ask for equality with no tolerance:
codes, their order, offsets, occurrences, scores.  Unchunked calls of at most 65 536 samples are also held against the host mirror
dr_mstep.streaming_path_scores, which tests/test_dr_mstep_stream_host.py pins to the same oracle: both routes then search the same batch
(a chunked call may take the search's small-batch pipeline, and there the replay of the call's own trace is the yardstick).  The cases are
built in tests/dr_mstep_stream_cases.py and tests/dr_mstep_cases.py; the CPU file checks that each has the structure it names."""
import ctypes as C

import numpy as np
import pytest

import dr_mstep_cases as cs
import dr_mstep_stream_cases as sc
from dismember_amd import _native as N
from dismember_amd import dr_mstep
from dismember_amd.dr_train import DRTrainer

pytestmark = pytest.mark.gpu
f64p = C.POINTER(C.c_double)
NEW_KINDS = (89, 90, 91, 92)      # EV_DMS_CODES, _ORDER, _FOLD, _EMIT of csrc/host_request.hip.inc


def _engine(case, dtype=np.float64):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.dr_load_model(case["w"], case["E"], case["L"], case["K"], case["D"], case["items"], dtype=dtype)
    return eng


def _run(eng, case, decay=0.999, **kw):
    return eng.dr_mstep_streaming_path_scores(case["seqs"], case["targets"], case["C"], decay, trace=True, **kw)


def _check(eng, case, decay=0.999):
    r = _run(eng, case, decay)
    want = sc.assert_result_is_replay(r, case, decay, *r[4:])
    return r, want


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _live(eng):
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert N.lib().dm_debug_live_device_allocs(C.byref(c), C.byref(b)) == 0
    return c.value, b.value


def _raw(eng, seqs, targets, n, c, decay, cap, off, codes, scores, occ, total, trace=(None, None, None)):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return N.lib().dm_dr_mstep_streaming_path_scores(eng._h, p(seqs, N.i32p), p(targets, N.i32p), n, c, decay, cap, p(off, N.i64p), p(codes, N.i64p),
                                                     p(scores, f64p), p(occ, N.i64p), p(total, N.i64p), p(trace[0], N.i32p), p(trace[1], f64p), p(trace[2], N.i32p))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(cs.REPLAY_SHAPES))
def test_replay_is_exact(shape, dtype):
    case = cs.model_case(*cs.REPLAY_SHAPES[shape])
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    assert r[6].min() == min(case["C"], case["K"] ** case["D"]) and len(want) > 10
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", sc.BOUNDARY_C)
def test_wave_workgroup_boundary(c, dtype):
    case = sc.boundary_case(c)
    eng = _engine(case, dtype)
    r, _ = _check(eng, case)
    assert (r[6] == c).all()
    st = sc.merge_stats(case["targets"], c, 0.999, *r[4:], case["K"])
    assert st["max_union"] > c and st["beam_only"] > 0 and st["both"] > 0
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_short_beams(dtype):
    case = cs.short_beam_case()
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    assert (r[6] == 4).all() and len(r[1]) == r[0][-1] == 4 * len(want)      # the lists never fill, and no slot past a count got in
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_first_and_last_item(dtype):
    case = cs.edge_case("4095")
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    off = r[0]
    assert off[1] == 0 and off[-1] > off[-2] and case["items"] - 1 in want and 0 not in want
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_long_chain_of_one_history(dtype):
    case = sc.long_chain_case()
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    idx = np.flatnonzero(case["targets"] == case["long_item"])
    st = sc.merge_stats(case["targets"][idx], case["C"], 0.999, *[a[idx] for a in r[4:]], case["K"])
    assert len(idx) == 3000 and st["both"] == 2999 * case["C"] and st["beam_only"] == 0 and st["list_only"] == 0
    assert len(want[case["long_item"]]) == case["C"]
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_alternating_disjoint_beams(dtype):
    case = sc.alternating_case()
    eng = _engine(case, dtype)
    r, _ = _check(eng, case)
    idx = np.flatnonzero(case["targets"] == case["alt_item"])
    paths, _, counts = (a[idx] for a in r[4:])
    a, b = (set(map(tuple, paths[k, :counts[k]].tolist())) for k in (0, 1))
    assert len(a) == len(b) == case["C"] and not (a & b)      # the device's own beams are disjoint too
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("decay", [1.0, 0.0])
def test_exact_ties(decay, dtype):
    case = cs.tie_case()
    eng = _engine(case, dtype)
    r, want = _check(eng, case, decay)
    st = sc.merge_stats(case["targets"], case["C"], decay, *r[4:], case["K"])
    print("merges whose cut falls inside a tie group:", st["cut_in_tie"], "tied neighbours in the lists:", sc.tied_neighbours(want))
    # decay 1: cuts fall inside tie groups.  decay 0: the +0 scores of what only the list held fall behind the full beam, the list is the
    # last beam by (score descending, path ascending) and its twins are the ties
    assert (st["cut_in_tie"] > 0) == (decay == 1.0) and sc.tied_neighbours(want) > 0 and not np.signbit(r[2]).any()
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("decay", [0.999, 0.5])
def test_decay_factors(decay, dtype):
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng = _engine(case, dtype)
    r, _ = _check(eng, case, decay)
    other = _run(eng, case, 0.25)
    assert other[2].tobytes() != r[2].tobytes()
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_queue_across_many_workgroups(dtype):
    case = sc.queue_case()
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    assert len(want) == case["items"] and r[3][0] == 2000 and r[3][1:].max() == 3
    eng.close()


@pytest.mark.parametrize("chunk", [64, 100])
def test_chunks(chunk, monkeypatch):
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng = _engine(case)
    whole = _run(eng, case)
    _same(whole[4:], eng.dr_beam_search(case["seqs"], case["C"]))      # N <= 32 768: one search of the whole request
    monkeypatch.setenv("DM_DR_MSTEP_CHUNK", str(chunk))
    r, _ = _check(eng, case)                                           # items span chunks; equal to this call's own replay
    assert (np.bincount(case["targets"][:chunk], minlength=case["items"]) * np.bincount(case["targets"][chunk:], minlength=case["items"])).any()
    for o in range(0, len(case["seqs"]), chunk):
        _same([a[o:o + chunk].copy() for a in r[4:]], eng.dr_beam_search(case["seqs"][o:o + chunk], case["C"]))
    eng.close()


def test_entry_points_agree_and_repeat():
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng = _engine(case, np.float32)
    first = _run(eng, case)
    _same(first, _run(eng, case))
    seqs, tg, Cn, D, items = case["seqs"], case["targets"], case["C"], case["D"], case["items"]
    n, cap = len(seqs), len(seqs) * Cn
    host = [seqs, tg, np.empty(items + 1, np.int64), np.empty(cap, np.int64), np.empty(cap, np.float64), np.empty(items, np.int64),
            np.empty((n, Cn, D), np.int32), np.empty((n, Cn), np.float64), np.empty(n, np.int32)]
    dev = [eng.dev_alloc(a.nbytes) for a in host]
    eng.h2d(dev[0], seqs)
    eng.h2d(dev[1], tg)
    total = eng.dr_mstep_streaming_path_scores_dev(dev[0], dev[1], n, Cn, cap, dev[2], dev[3], dev[4], dev[5], d_trace=tuple(dev[6:9]), decay_factor=0.999)
    for a, d in zip(host[2:], dev[2:]):
        eng.d2h(a, d)
    for d in dev:
        eng.dev_free(d)
    assert total == len(first[1])
    _same(first, (host[2], host[3][:total].copy(), host[4][:total].copy(), host[5], host[6], host[7], host[8]))
    eng.close()


def test_after_training_equals_a_fresh_load():
    from dismember_amd import Engine
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    K, D, L, E, items = (case[k] for k in ("K", "D", "L", "E", "items"))
    for dtype in (np.float64, np.float32):
        eng = _engine(case, dtype)
        before = _run(eng, case)
        rng = np.random.default_rng(3)
        tr = DRTrainer(eng, rng.integers(0, K, size=(items, 2, D)), lr=1e-2)
        for _ in range(2):
            tr.step(case["seqs"][:64], case["targets"][:64])
        trained, _ = _check(eng, case)
        assert trained[2].tobytes() != before[2].tobytes()
        fresh = Engine(0)
        fresh.dr_load_model(tr.weights(), E, L, K, D, items, dtype=dtype)
        _same(trained, _run(fresh, case))
        fresh.close()
        tr.close()
        eng.close()


@pytest.mark.parametrize("name", ["base", "C33", "tie", "few"])
def test_device_route_equals_the_host_mirror(name):
    """unchunked, N <= 65 536: both routes search the same batch"""
    case = {"base": lambda: cs.model_case(*cs.REPLAY_SHAPES["base"]), "C33": lambda: sc.boundary_case(33), "tie": cs.tie_case, "few": cs.few_samples_case}[name]()
    assert len(case["seqs"]) <= 65536
    eng = _engine(case)
    seqs, tg, Cn, items = case["seqs"], case["targets"], case["C"], case["items"]
    for decay in (0.999, 0.0):
        host = dr_mstep.streaming_path_scores(eng, seqs, tg, Cn, decay)
        dev, occ = dr_mstep.streaming_path_scores_dev(eng, seqs, tg, Cn, decay, with_occurrence=True)
        assert set(host) == set(dev) and occ == {int(v): int(n) for v, n in enumerate(np.bincount(tg)) if n}
        for v in host:
            assert host[v][0].tolist() == dev[v][0].tolist() and host[v][1].tobytes() == dev[v][1].tobytes()
    if name == "base":
        kw = dict(num_iteration=2, penalty_factor=1e-4, seed=5, train_mode="streaming", decay_factor=0.999)
        m_host = dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, **kw)
        m_dev = dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, path_scores="device_streaming", **kw)
        assert m_host == m_dev and len(m_dev) == items
        with pytest.raises(ValueError):
            dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, train_mode="batch", path_scores="device_streaming")
    eng.close()


def test_cap_too_small_and_live_allocations():
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng = _engine(case)
    good = _run(eng, case)
    live = _live(eng)
    again = _run(eng, case)
    assert _live(eng) == live                          # a warm call allocates nothing it keeps, and releases its temporaries
    _same(good, again)
    need, items = len(good[1]), case["items"]
    off, occ = np.full(items + 1, -7, np.int64), np.full(items, -7, np.int64)
    codes, scores, total = np.full(need, -7, np.int64), np.full(need, -7.0), np.zeros(1, np.int64)
    rc = _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], 0.999, need - 1, off, codes, scores, occ, total)
    assert rc == -1 and total[0] == need and "too small" in N.lib().dm_last_error(eng._h).decode()
    assert "streaming" in N.lib().dm_last_error(eng._h).decode()
    assert (off == -7).all() and (occ == -7).all() and (codes == -7).all() and (scores == -7.0).all()
    assert _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], 0.999, need, off, codes, scores, occ, total) == 0
    _same(good[:4], (off, codes, scores, occ))
    live = _live(eng)                                  # (without a trace the call holds one chunk's node ids itself: its block has grown once)
    assert _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], 0.999, need, off, codes, scores, occ, total) == 0
    assert _live(eng) == live
    eng.close()


def test_refusals_leave_the_handle_usable():
    from dismember_amd import Engine
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    seqs, tg, Cn, items = case["seqs"], case["targets"], case["C"], case["items"]
    n, cap = len(seqs), len(seqs) * Cn
    off, occ, codes, scores, total = np.empty(items + 1, np.int64), np.empty(items, np.int64), np.empty(cap, np.int64), np.empty(cap), np.zeros(1, np.int64)
    msg = lambda e: N.lib().dm_last_error(e._h).decode()
    eng = Engine(0)
    assert _raw(eng, seqs, tg, n, Cn, 0.999, cap, off, codes, scores, occ, total) == -3          # no model
    eng.dr_load_model(case["w"], case["E"], case["L"], case["K"], case["D"], items)
    good = _run(eng, case)

    def ok():
        _same(good, _run(eng, case))
    ok()
    for decay in (float("nan"), -0.1, 1.5, float("inf")):
        assert _raw(eng, seqs, tg, n, Cn, decay, cap, off, codes, scores, occ, total) == -1 and "decay_factor" in msg(eng)
        ok()
    for c in (0, 2049):
        assert _raw(eng, seqs, tg, n, c, 0.999, cap, off, codes, scores, occ, total) == -1 and "dm_dr_mstep_streaming_path_scores" in msg(eng)
        ok()
    assert _raw(eng, seqs, tg, n, Cn, 0.999, len(good[1]) - 1, off, codes, scores, occ, total) == -1 and total[0] == len(good[1])      # a short cap
    ok()
    bad = tg.copy()
    bad[7] = items
    assert _raw(eng, seqs, bad, n, Cn, 0.999, cap, off, codes, scores, occ, total) == -4
    ok()
    bad[7] = -1
    assert _raw(eng, seqs, bad, n, Cn, 0.999, cap, off, codes, scores, occ, total) == -4
    ok()
    off[:] = -1
    occ[:] = -1
    assert _raw(eng, seqs, tg, 0, Cn, 0.999, 0, off, None, None, occ, total) == 0 and total[0] == 0 and not off.any() and not occ.any()      # N = 0
    ok()
    r0 = eng.dr_mstep_streaming_path_scores(seqs[:0], tg[:0], Cn)
    assert not r0[0].any() and len(r0[1]) == 0 and not r0[3].any()
    ok()
    eng.close()


def test_new_launch_kinds_follow_the_switch(monkeypatch):
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng = _engine(case)
    monkeypatch.delenv("DM_DR_TIME_LAUNCHES", raising=False)
    _run(eng, case)
    eng.timing_reset()
    _run(eng, case)
    assert eng.timing_get()[0] > 0 and all(eng.timing_get_kind(k)[0] == 0 for k in NEW_KINDS)
    monkeypatch.setenv("DM_DR_TIME_LAUNCHES", "1")
    eng.timing_reset()
    _run(eng, case)
    assert [eng.timing_get_kind(k)[0] for k in NEW_KINDS] == [1, 1, 1, 1]      # one chunk: one pair each
    assert all(eng.timing_get_kind(k)[0] == 0 for k in range(80, 89))          # the batch route's kinds stay silent
    eng.close()
