"""Path assignment of the Deep-Retrieval M-step on the device (dm_dr_mstep_assign_paths, dm_dr_mstep_optimize) on the
synthetic CSRs of tests/dr_assign_cases.py.  On the "exact" cases (tests/test_dr_assign_host.py: every decision won by more than 8
tolerances) the codes of the hit items, the final sizes and every chosen position equal the restatement tests/dr_assign_ref.py; on every
case the replay of the call's own trace passes, no decision left out.  The tolerance is derived in dr_assign_ref.py."""
import ctypes as C

import numpy as np
import pytest

import dr_assign_cases as ac
import dr_assign_ref as ref
import dr_mstep_cases as cs
from dismember_amd import _native as N
from dismember_amd import dr_mstep
from dismember_amd.dr_train import DRTrainer

pytestmark = pytest.mark.gpu
f64p = C.POINTER(C.c_double)
NEW_KINDS = (94, 95, 96, 97)      # EV_DRA_INDEX, _CHECK, _CHAIN, _RANDOM of csrc/host_request.hip.inc
SEED = 5


@pytest.fixture(scope="module")
def eng():
    from dismember_amd import Engine
    e = Engine(0)                 # no model: the assignment needs a handle only
    yield e
    e.close()


def _run(eng, case, **kw):
    """-> (out, path_codes, path_sizes, trace_sel, trace_gain)"""
    a = dict(num_iteration=case["T"], penalty_factor=case["pf"], penalty_poly_order=case["p"], seed=SEED, with_paths=True, trace=True)
    a.update(kw)
    return eng.dr_mstep_assign_paths(case["off"], case["codes"], case["scores"], case["occ"], case["K"], case["D"], case["J"], **a)


def _raw(eng, case, **kw):
    a = dict(case, num_item=len(case["occ"]), total=len(case["codes"]), seed=SEED, out=np.full((len(case["occ"]), max(case["J"], 1)), -7, np.int64),
             pc=None, ps=None, npaths=None, ts=None, tg=None)
    a.update(kw)
    p = lambda x, t: None if x is None else x.ctypes.data_as(t)
    rc = N.lib().dm_dr_mstep_assign_paths(eng._h, p(a["off"], N.i64p), p(a["codes"], N.i64p), p(a["scores"], f64p), p(a["occ"], N.i64p), a["num_item"], a["total"],
                                          a["K"], a["D"], a["J"], a["T"], a["pf"], a["p"], a["seed"], p(a["out"], N.i64p), p(a["pc"], N.i64p), p(a["ps"], N.i32p),
                                          p(a["npaths"], N.i64p), p(a["ts"], N.i32p), p(a["tg"], f64p))
    return rc, a["out"]


def _msg(eng):
    return N.lib().dm_last_error(eng._h).decode()


def _live():
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert N.lib().dm_debug_live_device_allocs(C.byref(c), C.byref(b)) == 0
    return c.value, b.value


def _check(case, want, r, exact):
    out, pc, ps, ts, tg = r
    hit = ref.hit_items(case)
    sizes, out_replay, n = ref.replay(case, ts, tg)
    assert n == case["T"] * len(hit) * case["J"]
    assert np.array_equal(out[hit], out_replay[hit])
    # the sizes: those the trace implies, the histogram of the final assignment, never negative
    assert pc.tolist() == sorted(set(case["codes"].tolist())) and (ps >= 0).all()
    assert dict(zip(pc.tolist(), ps.tolist())) == sizes
    u, cnt = np.unique(out[hit], return_counts=True)
    hist = dict(zip(u.tolist(), cnt.tolist()))
    assert all(hist.get(c, 0) == s for c, s in zip(pc.tolist(), ps.tolist()))
    if exact:
        assert np.array_equal(ts, want["sel"]) and np.array_equal(out[hit], want["out"][hit])
        assert dict(zip(pc.tolist(), ps.tolist())) == want["sizes"]
    # the other items: the integer restatement of the draw
    rest = np.flatnonzero(case["occ"] <= 0)
    for v in rest[:50].tolist() + rest[-50:].tolist():
        assert out[v].tolist() == [ref.random_code(SEED, v, j, case["K"], case["D"]) for j in range(case["J"])]


@pytest.mark.parametrize("name", list(ac.CASES))
def test_assignment_equals_the_restatement(eng, name):
    case, want = ac.get(name)
    r = _run(eng, case)
    _check(case, want, r, name not in ac.NOT_EXACT)
    if name == "tie":
        assert np.array_equal(r[3], want["sel"])          # equal inputs give equal gains on one machine: the first maximum on both
    again = _run(eng, case)                               # repeats are byte-identical
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r, again))


def test_random_paths_do_not_depend_on_the_iterations(eng):
    case, _ = ac.get("sparse")
    outs = [_run(eng, case, num_iteration=t)[0] for t in (1, 2, 3)]
    rest = np.flatnonzero(case["occ"] <= 0)
    assert all(np.array_equal(o[rest], outs[0][rest]) for o in outs)
    assert not np.array_equal(_run(eng, case, seed=SEED + 1)[0][rest], outs[0][rest])
    assert (outs[0][rest] >= 0).all() and (outs[0][rest] < case["K"] ** case["D"]).all()


def test_host_and_device_entries_are_byte_equal(eng):
    case, _ = ac.get("hit257")
    out, pc, ps, ts, tg = _run(eng, case)
    ni, total, J, T, nh = len(case["occ"]), len(case["codes"]), case["J"], case["T"], len(ref.hit_items(case))
    host_in = [case["off"], case["codes"], case["scores"], case["occ"]]
    d_in = [eng.dev_alloc(a.nbytes) for a in host_in]
    for d, a in zip(d_in, host_in):
        eng.h2d(d, a)
    res = [np.empty((ni, J), np.int64), np.empty(total, np.int64), np.empty(total, np.int32), np.empty((T, nh, J), np.int32), np.empty((T, nh, J))]
    d_out = [eng.dev_alloc(a.nbytes) for a in res]
    P = eng.dr_mstep_assign_paths_dev(*d_in, ni, total, case["K"], case["D"], J, d_out[0], num_iteration=T, penalty_factor=case["pf"],
                                      penalty_poly_order=case["p"], seed=SEED, d_paths=(d_out[1], d_out[2]), d_trace=(d_out[3], d_out[4]))
    for d, a in zip(d_out, res):
        eng.d2h(a, d)
    assert P == len(pc)
    assert res[0].tobytes() == out.tobytes() and res[1][:P].tobytes() == pc.tobytes() and res[2][:P].tobytes() == ps.tobytes()
    assert res[3].tobytes() == ts.tobytes() and res[4].tobytes() == tg.tobytes()
    for d in d_in + d_out:
        eng.dev_free(d)


def test_refusals_and_the_stop_leave_the_handle_usable(eng):
    case, _ = ac.get("hit2")
    good = _run(eng, case)

    def ok():
        assert all(a.tobytes() == b.tobytes() for a, b in zip(good, _run(eng, case)))

    def refused(code, word, **kw):
        rc, out = _raw(eng, case, **kw)
        assert rc == code and word in _msg(eng) and (out is None or (out == -7).all()), (rc, _msg(eng))
        ok()
    refused(-1, "num_path_per_item", J=0)
    refused(-1, "num_iteration", T=0)
    for p in (0, 9):
        refused(-1, "penalty_poly_order", p=p)
    for pf in (-1.0, float("nan"), float("inf")):
        refused(-1, "penalty_factor", pf=pf)
    refused(-1, "2^62", K=1 << 16, D=4)
    refused(-1, "null", off=None)
    refused(-1, "null", out=None)
    refused(-1, "together", npaths=np.zeros(1, np.int64))
    refused(-1, "both", ts=np.zeros((3, 2, 3), np.int32))
    refused(-5, "2^31", total=1 << 31)
    # the device-side validation: the first offending item is named, nothing is written
    off = case["off"].copy()
    off[1] = off[2] + 1
    refused(-1, "item 0", off=off)
    codes = case["codes"].copy()
    codes[case["off"][1]] = -1
    refused(-1, "item 1", codes=codes)
    codes[case["off"][1]] = case["K"] ** case["D"]
    refused(-1, "item 1", codes=codes)
    codes[case["off"][1]] = codes[case["off"][1] + 1]
    refused(-1, "twice", codes=codes)
    for bad in (float("nan"), -0.5, float("inf")):
        scores = case["scores"].copy()
        scores[3] = bad
        refused(-1, "item 0", scores=scores)
    refused(-1, "item 0", J=21)                             # fewer candidates than paths per item
    big = ac.generic(20, 2, 2049, 3, 3000)
    rc, out = _raw(eng, big)
    assert rc == -1 and "2048" in _msg(eng) and (out == -7).all()
    ok()
    # the stop: the item the host route fails at
    stop = ac.stop_case()
    rc, out = _raw(eng, stop)
    assert rc == -1 and "item 3" in _msg(eng) and "log1p" in _msg(eng) and (out == -7).all()
    ok()
    # nothing to do is no error
    assert _raw(eng, case, num_item=0, total=0)[0] == 0
    rc, out = _raw(eng, dict(case, occ=np.zeros_like(case["occ"])))
    assert rc == 0 and out.tolist() == [[ref.random_code(SEED, v, j, case["K"], case["D"]) for j in range(case["J"])] for v in range(2)]
    ok()


def test_warm_call_allocates_nothing(eng):
    case, _ = ac.get("C130")
    first = _run(eng, case)
    live = _live()
    again = _run(eng, case)
    assert _live() == live
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_new_launch_kinds_follow_the_switch(eng, monkeypatch):
    case, _ = ac.get("T1")
    monkeypatch.delenv("DM_DR_TIME_LAUNCHES", raising=False)
    eng.timing_reset()
    _run(eng, case)
    assert all(eng.timing_get_kind(k)[0] == 0 for k in NEW_KINDS)
    monkeypatch.setenv("DM_DR_TIME_LAUNCHES", "1")
    eng.timing_reset()
    _run(eng, case, num_iteration=3)
    assert [eng.timing_get_kind(k)[0] for k in NEW_KINDS] == [1, 1, 3, 1]      # the chain: one launch per iteration
    assert all(eng.timing_get_kind(k)[0] == 0 for k in range(80, 94))          # the path-score kinds stay silent


# ---- with a small loaded model: the shape of tests/test_gpu_dr_mstep.py's smallest case
def _model_engine(case):
    from dismember_amd import Engine
    e = Engine(0)
    e.dr_load_model(case["w"], case["E"], case["L"], case["K"], case["D"], case["items"])
    return e


def test_fused_optimize_equals_path_scores_plus_assignment():
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    e = _model_engine(case)
    seqs, tg, Cn, K, D = case["seqs"], case["targets"], case["C"], case["K"], case["D"]
    kw = dict(num_iteration=2, penalty_factor=1e-4, penalty_poly_order=4, seed=SEED)
    for mode, scores in (("batch", e.dr_mstep_path_scores), ("streaming", e.dr_mstep_streaming_path_scores)):
        fused = e.dr_mstep_optimize(seqs, tg, Cn, 2, train_mode=mode, **kw)
        two = e.dr_mstep_assign_paths(*scores(seqs, tg, Cn), K, D, 2, **kw)
        assert fused.shape == (case["items"], 2) and fused.tobytes() == two.tobytes()
    with pytest.raises(Exception):
        e.dr_mstep_optimize(seqs, tg, 0, 2)
    e.close()


def test_optimize_device_assignment_equals_the_host_assignment():
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    e = _model_engine(case)
    seqs, tg, Cn, items = case["seqs"], case["targets"], case["C"], case["items"]
    kw = dict(num_iteration=2, penalty_factor=1e-4, seed=SEED)
    off, codes, scores, occ = e.dr_mstep_path_scores(seqs, tg, Cn)
    csr = dict(off=off, codes=codes, scores=scores, occ=occ, K=case["K"], D=case["D"], J=2, T=2, pf=1e-4, p=4)
    assert ref.min_margin(csr, ref.assign_ref(csr)) > 8.0      # the case shows the margin: both routes must decide alike
    hit = ref.hit_items(csr).tolist()
    m_host = dr_mstep.optimize(e, seqs, tg, range(items), Cn, 2, path_scores="device", **kw)
    for ps in ("device", "host"):
        m_dev = dr_mstep.optimize(e, seqs, tg, range(items), Cn, 2, path_scores=ps, assign="device", **kw)
        assert len(m_dev) == items
        assert all(m_dev[v] == m_host[v] for v in hit)
    arr = dr_mstep.optimize(e, seqs, tg, range(items), Cn, 2, path_scores="device", assign="device", as_array=True, **kw)
    assert arr.shape == (items, 2) and [tuple(x) for x in dr_mstep.decode_codes(arr[hit[0]], case["K"], case["D"]).tolist()] == m_dev[hit[0]]
    sub = dr_mstep.optimize(e, seqs, tg, hit[:5], Cn, 2, path_scores="device", assign="device", **kw)
    assert sorted(sub) == hit[:5]
    e.close()


def test_trainer_round_with_the_device_assignment():
    case = cs.model_case(*cs.REPLAY_SHAPES["base"])
    e = _model_engine(case)
    rng = np.random.default_rng(3)
    tr = DRTrainer(e, rng.integers(0, case["K"], size=(case["items"], 2, case["D"])), lr=1e-2)
    tr.step(case["seqs"][:64], case["targets"][:64])
    before = tr.item_paths.copy()
    paths = tr.mstep(case["seqs"], case["targets"], case["C"], num_iteration=2, assign="device", path_scores="device", seed=SEED)
    assert paths.shape == before.shape and (paths >= 0).all() and (paths < case["K"]).all() and not np.array_equal(paths, before)
    tr.step(case["seqs"][:64], case["targets"][:64])
    tr.close()
    e.close()
