"""Deep-Retrieval M-step path scores on the device (dm_dr_mstep_path_scores).  The call hands out the beams it aggregated
(its trace); the tests replay the aggregation on exactly those with oracle/dr_mstep_oracle.py, whose Python loop is the left-to-right sum,
and ask for equality with no tolerance: codes, their order, offsets, occurrences, scores.  The cases are built in tests/dr_mstep_cases.py;
tests/test_dr_mstep_dev_host.py checks without a GPU that each has the structure it names."""
import ctypes as C

import numpy as np
import pytest

import dr_mstep_cases as cs
from dismember_amd import _native as N
from dismember_amd import dr_mstep
from dismember_amd.dr_train import DRTrainer

pytestmark = pytest.mark.gpu
f64p = C.POINTER(C.c_double)


def _engine(case, dtype=np.float64):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.dr_load_model(case["w"], case["E"], case["L"], case["K"], case["D"], case["items"], dtype=dtype)
    return eng


def _run(eng, case, **kw):
    return eng.dr_mstep_path_scores(case["seqs"], case["targets"], case["C"], trace=True, **kw)


def _check(eng, case):
    r = _run(eng, case)
    want = cs.assert_result_is_replay(r, case, *r[4:])
    return r, want


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _live(eng):
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert N.lib().dm_debug_live_device_allocs(C.byref(c), C.byref(b)) == 0
    return c.value, b.value


def _raw(eng, seqs, targets, n, c, cap, off, codes, scores, occ, total, trace=(None, None, None)):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return N.lib().dm_dr_mstep_path_scores(eng._h, p(seqs, N.i32p), p(targets, N.i32p), n, c, cap, p(off, N.i64p), p(codes, N.i64p), p(scores, f64p),
                                           p(occ, N.i64p), p(total, N.i64p), p(trace[0], N.i32p), p(trace[1], f64p), p(trace[2], N.i32p))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(cs.REPLAY_SHAPES))
def test_replay_is_exact(shape, dtype):
    case = cs.model_case(*cs.REPLAY_SHAPES[shape])
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    assert r[6].min() == min(case["C"], case["K"] ** case["D"]) and len(want) > 10
    eng.close()


def test_one_layer_model_is_not_loadable():
    """D = 1: the reference requires at least two layers (LayerModel.scala:12) and dm_dr_load_model refuses such a model with that message,
    so no M-step can run on one; what can be checked is that refusal.  D = 2 and D = 4 are the ends of what loads."""
    from dismember_amd import Engine
    from dismember_amd.engine import DismemberError
    case = cs.model_case(8, 2, 5, 16, 120, 300, 6)
    w = dict(case["w"], layer_w=case["w"]["layer_w"][:1], layer_b=case["w"]["layer_b"][:1], layer_emb=case["w"]["layer_emb"][:120])
    eng = Engine(0)
    with pytest.raises(DismemberError) as e:
        eng.dr_load_model(w, 16, 5, 8, 1, 120)
    assert e.value.code == -1 and "at least 2" in str(e.value)
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_short_beams(dtype):
    case = cs.short_beam_case()
    eng = _engine(case, dtype)
    r, want = _check(eng, case)
    assert (r[6] == 4).all() and (r[4][:, 4:] == -1).all()
    assert len(r[1]) == r[0][-1] == sum(len(v) for v in want.values()) == 4 * len(want)      # no slot past a count reached a sum
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_long_segments(dtype):
    case = cs.long_segment_case()
    eng = _engine(case, dtype)
    r, _ = _check(eng, case)
    seg = cs.segments(case["targets"], case["K"], *r[4:])
    lens = {len(v) for v in seg.values()}
    assert {3000, cs.LANE_MAX - 1, cs.LANE_MAX, cs.LANE_MAX + 1, 63, 64, 65, 127, 129} <= lens
    # fp64: a pairwise sum would have been caught.  An f32 model's probabilities are 24-bit values of one magnitude: 3 000 of them add
    # without rounding in fp64 whatever the order, so there the case checks the long-segment path alone
    assert dtype == np.float32 or cs.sequential_vs_reduceat(seg) > 0
    eng.close()


@pytest.mark.parametrize("name", list(cs.EDGE_SHAPES))
def test_sort_tile_edges(name):
    case = cs.edge_case(name)
    eng = _engine(case)
    r, want = _check(eng, case)
    off = r[0]
    assert off[1] == 0 and off[-1] > off[-2] and case["items"] - 1 in want and 0 not in want
    eng.close()


def test_all_samples_on_one_item():
    case = cs.one_item_case()
    eng = _engine(case, np.float32)
    r, want = _check(eng, case)
    assert len(cs.segments(case["targets"], case["K"], *r[4:])) > cs.TILE      # more segments than a sort tile, all of one item
    assert list(want) == [case["items"] - 1] and len(r[1]) == case["C"]
    eng.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_exact_ties(dtype):
    case = cs.tie_case()
    eng = _engine(case, dtype)
    r, _ = _check(eng, case)
    off, codes, scores = r[:3]
    ties = 0
    for v in range(case["items"]):
        c, s = codes[off[v]:off[v + 1]], scores[off[v]:off[v + 1]]
        assert (np.diff(s) <= 0).all()
        eq = np.flatnonzero(np.diff(s) == 0)
        assert (c[eq] < c[eq + 1]).all()               # equal scores: ascending path code
        ties += len(eq)
    print("tied neighbours in the results:", ties)
    eng.close()


@pytest.mark.parametrize("chunk", [64, 100])
def test_chunks(chunk, monkeypatch):
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng = _engine(case)
    whole = _run(eng, case)
    _same(whole[4:], eng.dr_beam_search(case["seqs"], case["C"]))      # N <= 32 768: one search of the whole request
    monkeypatch.setenv("DM_DR_MSTEP_CHUNK", str(chunk))
    r, _ = _check(eng, case)
    for o in range(0, len(case["seqs"]), chunk):
        _same([a[o:o + chunk].copy() for a in r[4:]], eng.dr_beam_search(case["seqs"][o:o + chunk], case["C"]))
    eng.close()


def test_entry_points_agree():
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
    total = eng.dr_mstep_path_scores_dev(dev[0], dev[1], n, Cn, cap, dev[2], dev[3], dev[4], dev[5], d_trace=tuple(dev[6:9]))
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
    rc = _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], need - 1, off, codes, scores, occ, total)
    assert rc == -1 and total[0] == need and "too small" in N.lib().dm_last_error(eng._h).decode()
    assert (off == -7).all() and (occ == -7).all() and (codes == -7).all() and (scores == -7.0).all()
    assert _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], need, off, codes, scores, occ, total) == 0
    _same(good[:4], (off, codes, scores, occ))
    live = _live(eng)                                  # (without a trace the call holds one chunk's node ids itself: its block has grown once)
    assert _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], need - 1, off, codes, scores, occ, total) == -1
    assert _raw(eng, case["seqs"], case["targets"], len(case["seqs"]), case["C"], need, off, codes, scores, occ, total) == 0
    assert _live(eng) == live
    eng.close()


def test_refusals_leave_the_handle_usable():
    from dismember_amd import Engine
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    seqs, tg, Cn, items = case["seqs"], case["targets"], case["C"], case["items"]
    n, cap = len(seqs), len(seqs) * Cn
    off, occ, codes, scores, total = np.empty(items + 1, np.int64), np.empty(items, np.int64), np.empty(cap, np.int64), np.empty(cap), np.zeros(1, np.int64)
    tr = (np.empty((n, Cn, case["D"]), np.int32), np.empty((n, Cn)), np.empty(n, np.int32))
    msg = lambda e: N.lib().dm_last_error(e._h).decode()
    eng = Engine(0)
    assert _raw(eng, seqs, tg, n, Cn, cap, off, codes, scores, occ, total) == -3          # no model
    eng.dr_load_model(case["w"], case["E"], case["L"], case["K"], case["D"], items)
    good = _run(eng, case)

    def ok():
        _same(good, _run(eng, case))
    ok()
    for c in (0, 2049, -1):
        assert _raw(eng, seqs, tg, n, c, cap, off, codes, scores, occ, total) == -1
        ok()
    for args in ((None, tg, n, Cn, cap, off, codes, scores, occ, total), (seqs, None, n, Cn, cap, off, codes, scores, occ, total),
                 (seqs, tg, n, Cn, cap, None, codes, scores, occ, total), (seqs, tg, n, Cn, cap, off, None, scores, occ, total),
                 (seqs, tg, n, Cn, cap, off, codes, None, occ, total), (seqs, tg, n, Cn, cap, off, codes, scores, occ, None)):
        assert _raw(eng, *args) == -1 and "null" in msg(eng)
        ok()
    assert _raw(eng, seqs, tg, -1, Cn, cap, off, codes, scores, occ, total) == -1
    ok()
    for part in ((tr[0], None, None), (None, tr[1], tr[2]), (tr[0], tr[1], None)):
        assert _raw(eng, seqs, tg, n, Cn, cap, off, codes, scores, occ, total, trace=part) == -1 and "trace" in msg(eng)
        ok()
    assert _raw(eng, seqs, tg, 2 ** 31 // 2048, 2048, cap, off, codes, scores, occ, total) == -5 and "2^31" in msg(eng)      # nothing is read
    ok()
    bad = tg.copy()
    bad[7] = items
    assert _raw(eng, seqs, bad, n, Cn, cap, off, codes, scores, occ, total) == -4
    bad = seqs.copy()
    bad[3, 2] = items
    assert _raw(eng, bad, tg, n, Cn, cap, off, codes, scores, occ, total) == -4
    ok()
    assert _raw(eng, seqs, tg, n, Cn, cap, off, codes, scores, None, total) == 0           # the occurrences are optional
    _same(good[:3], (off, codes[:total[0]].copy(), scores[:total[0]].copy()))
    off[:] = -1
    occ[:] = -1
    assert _raw(eng, seqs, tg, 0, Cn, 0, off, None, None, occ, total) == 0 and total[0] == 0 and not off.any() and not occ.any()      # N = 0
    ok()
    eng.close()


def test_key_too_wide_is_refused():
    """ceil(log2 num_item) + ceil(log2 K^D) = 20 + 44 = 64 > 63: refused by name of the limit; the handle then serves another model"""
    from dismember_amd import Engine
    K, D, L, E, items = 2048, 4, 2, 16, 2 ** 19 + 1
    rng = np.random.default_rng(0)
    row = lambda *s: (rng.standard_normal(s[-1]).astype(np.float32) * 0.05) * np.ones(s, np.float32)      # (cheap: one random row, repeated)
    w = dict(layer_emb=row(items + K * (D - 1), E), layer_w=[row(K, (L + d) * E) for d in range(D)], layer_b=[np.zeros(K, np.float32) for _ in range(D)])
    eng = Engine(0)
    eng.dr_load_model(w, E, L, K, D, items, dtype=np.float32)
    seqs, tg = np.zeros((4, L), np.int32), np.arange(4, dtype=np.int32)
    off, occ, codes, scores, total = np.empty(items + 1, np.int64), np.empty(items, np.int64), np.empty(8, np.int64), np.empty(8), np.zeros(1, np.int64)
    assert _raw(eng, seqs, tg, 4, 2, 8, off, codes, scores, occ, total) == -5
    assert "63" in N.lib().dm_last_error(eng._h).decode()
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    eng.dr_load_model(case["w"], case["E"], case["L"], case["K"], case["D"], case["items"])
    _check(eng, case)
    eng.close()


def test_end_to_end_device_route():
    case = cs.few_samples_case()
    n_max = np.bincount(case["targets"]).max()
    assert n_max <= 7 and n_max <= 2       # no pairwise sum on the host route, and no third term either (see dr_mstep_cases.few_samples_case)
    eng = _engine(case)
    seqs, tg, Cn, K, D, items = case["seqs"], case["targets"], case["C"], case["K"], case["D"], case["items"]
    host, dev = dr_mstep.batch_path_scores(eng, seqs, tg, Cn), dr_mstep.batch_path_scores_dev(eng, seqs, tg, Cn)
    assert set(host) == set(dev)
    for v in host:
        assert host[v][0].tolist() == dev[v][0].tolist() and host[v][1].tobytes() == dev[v][1].tobytes()
    kw = dict(num_iteration=2, penalty_factor=1e-4, seed=5)
    m_host = dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, **kw)
    m_dev = dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, path_scores="device", **kw)
    assert m_host == m_dev and len(m_dev) == items
    with pytest.raises(ValueError):
        dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, train_mode="streaming", path_scores="device")
    # one E/M round through the device route
    tr = DRTrainer(eng, np.array([m_dev[i] for i in range(items)]), lr=1e-2)
    for o in range(0, len(tg), 32):
        loss = tr.step(seqs[o:o + 32], tg[o:o + 32])
    assert np.isfinite(loss).all()
    new = dr_mstep.optimize(eng, seqs, tg, range(items), Cn, 2, path_scores="device", **kw)
    assert set(new) == set(range(items)) and all(len(p) == 2 and all(len(q) == D and all(0 <= x < K for x in q) for q in p) for p in new.values())
    tr.set_item_paths(np.array([new[i] for i in range(items)]))
    tr.close()
    eng.close()
