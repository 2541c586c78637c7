"""JTM tree learning with a DeepFM model on the device (dismember_amd/csrc/dfm_jtm.hip.inc and the dm_deepfm_jtm_* entry points).

Scores are compared as |gpu - ref64| <= 1e-5 + 1e-4 |ref64| against the float64 restatement of the reference's graph (tests/deepfm_ref.py);
tests/test_deepfm_jtm_host.py shows on the same inputs that the reference's own float32 arithmetic needs that much, and that the
per-history form equals the graph.  Everything downstream of the scorer is bit-exact: a pair's logit depends on its (code, history) only
(test 2), so every pipeline path must EQUAL jtm_ref.sum_weights_f32 over dm_deepfm_pairs_forward of jtm_ref.expand_pairs (test 3).

Set-up (tests/dfm_jtm_ref.py): the depth-10 tree and the 943-row catalogue of tests/test_gpu_jtm_scoring.py, DeepFM weights of
deepfm_ref.random_deepfm_weights(default_rng(5), E, L, 2047)."""
import ctypes as C
import os

import numpy as np
import pytest

import deepfm_ref
import dfm_jtm_ref as D
import jtm_ref

pytestmark = pytest.mark.gpu
INVALID, STATE, INDEX = -1, -3, -4
_ENGINES = {}


def _lib():
    from dismember_amd import _native as N
    return N, N.lib()


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _new_engine(E, L, w=None):
    from dismember_amd import Engine
    t, cat = D.tree(), D.catalogue(L)
    eng = Engine(0)
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], D.DEPTH)
    eng.load_id_maps(cat["map_ids"], cat["map_codes"])
    eng.load_weights_deepfm(D.weights(E, L) if w is None else w, E, L, D.NI)
    return eng


def _engine(E, L):
    if (E, L) not in _ENGINES:
        _ENGINES[(E, L)] = _new_engine(E, L)
    return _ENGINES[(E, L)]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


# ---- the entry points on the catalogue (the calls of tests/test_gpu_jtm_scoring.py, through the twins)
def _uncached(eng, cat, L, node, old_level, level, hier, min_level, use_mask=0, check=True):
    N, lib = _lib()
    n = cat["items"].size
    w = np.full((n, 1 << (level - old_level)), np.nan, np.float32)
    rc = lib.dm_deepfm_jtm_child_weights(eng._h, _ptr(cat["row_off"], N.i64p), _ptr(cat["row_ids"], N.i32p), _ptr(node, N.i32p), n, L, old_level, level,
                                         int(hier), min_level, use_mask, _ptr(w, N.f32p))
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


def _cached(eng, node, lo, hi, old_level, level, hier, min_level, use_mask=0, check=True):
    N, lib = _lib()
    sub = np.ascontiguousarray(node[lo:hi])
    w = np.full((hi - lo, 1 << (level - old_level)), np.nan, np.float32)
    rc = lib.dm_deepfm_jtm_child_weights_cached(eng._h, _ptr(sub, N.i32p), lo, hi - lo, old_level, level, int(hier), min_level, use_mask, _ptr(w, N.f32p))
    if check:
        eng._chk(rc)
        return w
    return rc


def _cuts(n):
    return [(0, n // 3), (n // 3, n // 3 + 1), (n // 3 + 1, n)]


def _all_device_paths(eng, cat, L, node, old_level, level, hier, min_level):
    """uncached call, cached call over the full range, three cached ranges on a handle that holds only that range"""
    n = cat["items"].size
    out = {"uncached": _uncached(eng, cat, L, node, old_level, level, hier, min_level)}
    try:
        _cache(eng, cat, L)
        out["cached"] = _cached(eng, node, 0, n, old_level, level, hier, min_level)
        parts = []
        for lo, hi in _cuts(n):
            _cache(eng, cat, L, lo, hi)
            parts.append(_cached(eng, node, lo, hi, old_level, level, hier, min_level))
        out["ranges"] = np.concatenate(parts, axis=0)
    finally:
        _uncache(eng, L)
    return out


# --------------------------------------------------------------------------- 1. the scorer against the restatement
@pytest.mark.parametrize("seq_div", D.SEQ_DIVS)
@pytest.mark.parametrize("E,L", D.SCORER_EL)
def test_scorer_against_the_restatement(E, L, seq_div):
    """dm_deepfm_pairs_forward within 1e-5 + 1e-4 |ref| of float64 deepfm_ref.forward, for P = 1, 17 and all pairs.  The inputs hold a -1
    node code (pair 5), the all-pad history and the unmasked -1 key."""
    old = D.OLD_LEVEL[(E, L)]
    codes, seqs, ref = D.scorer_inputs(E, L, old, old + D.GAP_OF[seq_div])
    nchain = jtm_ref.nchain_of(D.GAP_OF[seq_div])
    hist = seqs if seq_div == 1 else seqs[::nchain]          # seq_div 1: the histories replicated per pair
    assert codes[5] == -1 and (seqs == -1).all(axis=1).any() and seq_div in (1, nchain)
    eng = _engine(E, L)
    for P in (1, 17, codes.size):
        got = eng.deepfm_pairs_forward(codes[:P], hist[:-(-P // seq_div)], seq_div)
        assert got.dtype == np.float32 and got.shape == (P,) and np.isfinite(got).all()
        ratio = np.abs(got.astype(np.float64) - ref[:P]) / D.tolerance(ref[:P])
        print("E=%d L=%d seq_div=%d P=%d error / tolerance: max %.3f" % (E, L, seq_div, P, ratio.max()))
        assert ratio.max() <= 1.0, (P, int(ratio.argmax()))


# --------------------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("E,L", D.PIPELINE_EL)
def test_a_logit_depends_on_its_pair_only(E, L):
    """The same pairs in catalogue order with seq_div = nchain, in a random permutation with seq_div = 1 and replicated histories, and
    as single-pair calls: identical bytes per pair; two runs: identical bytes."""
    old, gap = 4, 2
    nchain = jtm_ref.nchain_of(gap)
    px = D.pairs(L, old, old + gap)
    codes, seqs = px["codes"], px["seqs"]
    eng = _engine(E, L)
    a = eng.deepfm_pairs_forward(codes, seqs[::nchain], nchain)
    assert a.tobytes() == eng.deepfm_pairs_forward(codes, seqs[::nchain], nchain).tobytes()
    assert len(np.unique(a)) > a.size // 2
    perm = np.random.default_rng(3).permutation(codes.size)
    b = eng.deepfm_pairs_forward(codes[perm], seqs[perm], 1)
    assert np.array_equal(b, a[perm]), int((b != a[perm]).sum())
    for q in np.random.default_rng(4).choice(codes.size, 20, replace=False):
        one = eng.deepfm_pairs_forward(codes[q:q + 1], seqs[q:q + 1], 1)
        assert one.tobytes() == a[q:q + 1].tobytes(), int(q)
        assert eng.deepfm_pairs_forward(codes[q:q + 1], seqs[q:q + 1], nchain).tobytes() == one.tobytes()      # seq_div does not enter


@pytest.mark.parametrize("slice_", [1, 100, 943])
def test_set_up_slices_do_not_move_a_logit(monkeypatch, slice_):
    """The per-history results live for one slice of histories (2^18 by default; DM_DFM_JTM_SLICE brings the slice edges to a size a test
    can afford): 1, 100 and 943 histories per slice — every pair its own slice at seq_div 1, slices of 6 and 600 pairs that end inside a
    tile, and exactly one slice — give the unsliced bytes."""
    E, L, old, gap = 128, 15, 4, 2
    nchain = jtm_ref.nchain_of(gap)
    px = D.pairs(L, old, old + gap)
    eng = _engine(E, L)
    whole = eng.deepfm_pairs_forward(px["codes"], px["seqs"][::nchain], nchain)
    monkeypatch.setenv("DM_DFM_JTM_SLICE", str(slice_))
    assert eng.deepfm_pairs_forward(px["codes"], px["seqs"][::nchain], nchain).tobytes() == whole.tobytes()
    assert eng.deepfm_pairs_forward(px["codes"][:700], px["seqs"][:700], 1).tobytes() == whole[:700].tobytes()
    cat = D.catalogue(L)
    assert np.array_equal(_uncached(eng, cat, L, px["node"], old, old + gap, False, 0), _case(E, L, gap, False)["ref"])


# --------------------------------------------------------------------------- 3. / 4. the pipeline
_CASES = {}


def _case(E, L, gap, hier):
    """every device path of one case and the restatement over dm_deepfm_pairs_forward of the same pairs (one history per pair, a
    different tiling from the cached path's); computed once, shared by tests 3 and 4"""
    key = (E, L, gap, hier)
    if key not in _CASES:
        old, level, min_level = 4, 4 + gap, 6 if hier else 0
        eng, cat = _engine(E, L), D.catalogue(L)
        px = D.pairs(L, old, level, hier, min_level)
        assert not px["bad"]
        out = _all_device_paths(eng, cat, L, px["node"], old, level, hier, min_level)
        logits = eng.deepfm_pairs_forward(px["codes"], px["seqs"], 1)
        out.update(pairs=px, logits=logits, ref=jtm_ref.sum_weights_f32(logits, cat["row_off"], gap), min_level=min_level)
        _CASES[key] = out
    return _CASES[key]


PIPELINE = [(E, L, gap, hier) for E, L in D.PIPELINE_EL for gap in (1, 2, 3) for hier in (False, True)]
_pid = lambda c: "E%d-L%d-gap%d-hier%d" % c


@pytest.mark.parametrize("case", PIPELINE, ids=_pid)
def test_every_path_equals_the_restatement_bit_for_bit(case):
    E, L, gap, hier = case
    r, cat = _case(*case), D.catalogue(L)
    seen = np.diff(cat["row_off"]) > 0
    assert (r["ref"][~seen] == np.float32(-1e6)).all() and np.isfinite(r["ref"]).all()
    assert len(np.unique(r["ref"][seen])) > seen.sum()                       # the weights are not degenerate
    for name in ("cached", "ranges", "uncached"):
        got = r[name]
        differ = np.flatnonzero((got != r["ref"]).any(axis=1))
        assert np.array_equal(got, r["ref"]), "%s: %d items differ, first %s (rows %s)" % (
            name, differ.size, differ[:5].tolist(), np.diff(cat["row_off"])[differ[:5]].tolist())


@pytest.mark.parametrize("cap", [96, 1000])
@pytest.mark.parametrize("case", [(16, 10, 2, False), (16, 10, 2, True), (128, 15, 3, False), (128, 15, 1, True)], ids=_pid)
def test_chunked_scoring_equals_unchunked(monkeypatch, case, cap):
    """DM_JTM_MAX_PAIRS = 96 (chunk edges between the items of 2 .. 5 rows; the 40-row item alone exceeds it) and 1000 (chunks of many
    items): every path, bit for bit"""
    E, L, gap, hier = case
    whole = _case(*case)
    monkeypatch.setenv("DM_JTM_MAX_PAIRS", str(cap))
    got = _all_device_paths(_engine(E, L), D.catalogue(L), L, whole["pairs"]["node"], 4, 4 + gap, hier, whole["min_level"])
    for name in ("uncached", "cached", "ranges"):
        assert np.array_equal(got[name], whole["ref"]), (name, cap)


@pytest.mark.parametrize("case", PIPELINE, ids=_pid)
def test_weights_against_float64(case):
    """|w - w64| <= sum over the weight's rows * gap logits of (1e-5 + 1e-4 |logit64|) + the bound of the sequential fp32 sums: the
    budget of tests/test_gpu_jtm_scoring.py's oracle test"""
    E, L, gap, hier = case
    r, cat = _case(*case), D.catalogue(L)
    ref = D.ref64(E, L, 4, 4 + gap, hier, r["min_level"])
    w64 = jtm_ref.chain_sum(ref, cat["row_off"], gap)
    bound = jtm_ref.chain_sum(D.tolerance(ref), cat["row_off"], gap) + jtm_ref.sum_bound_f32(ref, cat["row_off"], gap)
    seen = np.diff(cat["row_off"]) > 0
    for name in ("cached", "uncached"):
        err = np.abs(r[name].astype(np.float64) - w64)
        print("%s %s: max |w - w64| = %.3g, max err / bound = %.3g, max |w| = %.3g" % (_pid(case), name, err[seen].max(), (err[seen] / bound[seen]).max(),
                                                                                     np.abs(w64[seen]).max()))
        assert (r[name][~seen] == np.float32(-1e6)).all() and (err[seen] <= bound[seen]).all()


# --------------------------------------------------------------------------- 5. optimize
@pytest.mark.parametrize("hier", [False, True])
def test_optimize_three_ways(monkeypatch, hier):
    """dm_deepfm_jtm_optimize_cached, the step-wise dm_deepfm_jtm_step_cached loop and JTM._optimize with the host dm_jtm_rebalance_all on
    the device's own weights: one projection, a bijection onto level-10 codes; one rank."""
    from dismember_amd.jtm import JTM
    E, L = 16, 10
    eng, cat = _engine(E, L), D.catalogue(L)
    jt = JTM.from_arrays(eng, cat["items"], cat["item_code"], D.DEPTH, cat["row_off"], cat["row_ids"], gap=2, seq_len=L, hierarchical=hier, min_level=6,
                         use_mask=True)
    assert jt.deepfm and jt.use_mask is False                     # the graph has no mask input
    monkeypatch.delenv("DM_JTM_FUSED", raising=False)
    fused = jt.optimize(as_array=True)
    st = jt.optimize_stats()
    assert st["nranks"] == 1 and st["transport"] == "none" and st["items_scored"] == 5 * cat["items"].size
    monkeypatch.setenv("DM_JTM_FUSED", "step")
    tm = {}
    step = jt.optimize(as_array=True, timing=tm)
    assert tm["fused_step_s"] > 0                                 # the step-wise loop ran dm_deepfm_jtm_step_cached
    monkeypatch.setenv("DM_JTM_FUSED", "0")
    tm = {}
    host = jt.optimize(as_array=True, timing=tm)
    assert tm["fused_step_s"] == 0 and tm["scoring_s"] > 0
    assert np.array_equal(fused, step) and np.array_equal(fused, host)
    assert np.unique(fused).size == fused.size and (fused >= (1 << D.DEPTH) - 1).all() and (fused < (2 << D.DEPTH) - 1).all()
    assert not np.array_equal(fused, cat["item_code"])
    as_map = jt.optimize()
    assert sorted(as_map) == cat["items"].tolist() and list(as_map.values()) == host.tolist()


# --------------------------------------------------------------------------- 6. no stale copy
def test_no_stale_copy_after_training_clone_and_checkpoint(tmp_path):
    """One training step moves l1.W: the W1s fragments the set-up kernel reads are rebuilt with the serving copies.  Child weights then
    equal, byte for byte, those of a fresh engine loaded with the downloaded vector; the same through a clone made BEFORE the step and
    after a checkpoint round trip."""
    from dismember_amd import Engine
    E, L, old, level = 16, 10, 4, 6
    cat = D.catalogue(L)
    px = D.pairs(L, old, level)
    eng = _new_engine(E, L)
    clone = eng.clone()
    fresh = loaded = None
    try:
        before = _uncached(eng, cat, L, px["node"], old, level, False, 0)
        assert np.array_equal(before, _case(E, L, 2, False)["ref"])
        eng.deepfm_train_init(lr=0.05)
        rng = np.random.default_rng(8)
        rows = rng.choice(px["codes"].size, 512, replace=False)
        loss = eng.deepfm_train_forward_backward(px["codes"][rows], px["seqs"][rows], rng.integers(0, 2, 512).astype(np.float32))
        assert np.isfinite(loss)
        eng.deepfm_adam_step()
        wt = eng.deepfm_train_download("weights")
        o = deepfm_ref.deepfm_offsets(E, L, D.NI)
        assert not np.array_equal(wt[o["l1_w"]:o["l1_b"]], D.weights(E, L)[o["l1_w"]:o["l1_b"]])
        fresh = _new_engine(E, L, wt)
        want = _uncached(fresh, cat, L, px["node"], old, level, False, 0)
        assert not np.array_equal(want, before)
        after = _all_device_paths(eng, cat, L, px["node"], old, level, False, 0)
        for name in ("uncached", "cached", "ranges"):
            assert after[name].tobytes() == want.tobytes(), name
        assert _uncached(clone, cat, L, px["node"], old, level, False, 0).tobytes() == want.tobytes()
        path = str(tmp_path / "trained.bin")
        eng.save_model(path)
        loaded = Engine(0)
        loaded.load_model(path)
        assert loaded.scorer_kind() == ("deepfm", L)
        assert _uncached(loaded, cat, L, px["node"], old, level, False, 0).tobytes() == want.tobytes()
    finally:
        for e in (clone, eng, fresh, loaded):
            if e is not None:
                e.close()


# --------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_usable():
    from dismember_amd import DismemberError
    N, lib = _lib()
    E, L, old, level = 16, 10, 4, 6
    cat, px = D.catalogue(L), D.pairs(L, old, level)
    n, node = cat["items"].size, px["node"]
    good = _case(E, L, 2, False)["ref"]
    eng = _new_engine(E, L)
    h = eng._h
    out_f, out_i = np.zeros(4 * n, np.float32), np.zeros(n, np.int32)
    old_node = jtm_ref.ancestor_at_level(cat["item_code"], level).astype(np.int32)
    i32p, f32p = lambda a: _ptr(a, N.i32p), lambda a: _ptr(a, N.f32p)

    def twins(hh, use_mask=0, L_=L):
        return {
            "dm_deepfm_jtm_child_weights": lambda: lib.dm_deepfm_jtm_child_weights(hh, _ptr(cat["row_off"], N.i64p), i32p(cat["row_ids"]), i32p(node), n, L_, old,
                                                                                   level, 0, 0, use_mask, f32p(out_f)),
            "dm_deepfm_jtm_child_weights_cached": lambda: lib.dm_deepfm_jtm_child_weights_cached(hh, i32p(node), 0, n, old, level, 0, 0, use_mask, f32p(out_f)),
            "dm_deepfm_jtm_step_cached": lambda: lib.dm_deepfm_jtm_step_cached(hh, i32p(node), i32p(old_node), n, old, level, 0, 0, use_mask, 16, i32p(out_i)),
            "dm_deepfm_jtm_optimize_cached": lambda: lib.dm_deepfm_jtm_optimize_cached(hh, i32p(cat["item_code"]), n, D.DEPTH, 2, 0, 0, use_mask, i32p(out_i), None),
        }

    def still_good():
        assert np.array_equal(_uncached(eng, cat, L, node, old, level, False, 0), good)

    def msg():
        return (lib.dm_last_error(h) or b"").decode()
    try:
        # a NULL handle
        for name, call in twins(None).items():
            assert call() == INVALID, name
        assert lib.dm_deepfm_pairs_forward(None, i32p(px["codes"]), i32p(px["seqs"]), 1, L, 1, f32p(out_f)) == INVALID
        _cache(eng, cat, L)
        # use_mask != 0: the graph has no mask input
        for name, call in twins(h, use_mask=1).items():
            assert call() == INVALID and "no mask input" in msg(), (name, msg())
            still_good()
        # a history length that is not the model's: the call's, or the cached catalogue's
        assert twins(h, L_=9)["dm_deepfm_jtm_child_weights"]() == INVALID and "seq_len" in msg()
        still_good()
        with pytest.raises(DismemberError) as e:
            eng.deepfm_pairs_forward(px["codes"][:3], px["seqs"][:3, :9], 1)
        assert e.value.code == INVALID
        cat9 = D.catalogue(9)
        _cache(eng, cat9, 9)
        for name, call in twins(h).items():
            if name != "dm_deepfm_jtm_child_weights":
                assert call() == INVALID and "seq_len" in msg(), (name, msg())
        _cache(eng, cat, L)
        assert np.array_equal(_cached(eng, node, 0, n, old, level, False, 0), good)
        # codes outside the table: the index errors of dm_deepfm_forward
        bad_seqs = px["seqs"][:3].copy()
        bad_seqs[1, 2] = D.NI
        for codes_, seqs_ in ((np.array([1, D.NI, 2], np.int32), px["seqs"][:3]), (np.array([1, -2, 2], np.int32), px["seqs"][:3]), (px["codes"][:3], bad_seqs)):
            with pytest.raises(DismemberError) as e:
                eng.deepfm_pairs_forward(codes_, seqs_, 1)
            assert e.value.code == INDEX and "valid index range" in str(e.value)
        assert eng.deepfm_pairs_forward(px["codes"][:3], px["seqs"][:3], 1).tobytes() == _case(E, L, 2, False)["logits"][:3].tobytes()
        # a hole of the id map in a history: DM_ERR_INDEX, and again on a retry (the per-row codes built with it are dropped)
        bad_cat = dict(cat, row_ids=cat["row_ids"].copy())
        bad_cat["row_ids"][int(cat["row_off"][n // 2]) + 9, 3] = cat["hole_ids"][0]
        text = "history code outside the embedding table"
        assert _uncached(eng, bad_cat, L, node, old, level, False, 0, check=False) == INDEX and text in msg()
        _cache(eng, bad_cat, L)
        for _ in range(2):
            assert _cached(eng, node, 0, n, old, level, False, 0, check=False) == INDEX and text in msg()
        _cache(eng, cat, L)
        assert np.array_equal(_cached(eng, node, 0, n, old, level, False, 0), good)
        # DIN weights on the same handle: the twins answer DM_ERR_STATE, the DIN entry points score as on a handle that never held DeepFM
        eng.load_weights_din_synthetic(32, D.NI, 9, tree_depth=D.DEPTH, rho=0.9)
        for name, call in twins(h).items():
            assert call() == STATE and "the loaded scorer is DIN" in msg(), (name, msg())
        with pytest.raises(DismemberError) as e:
            eng.deepfm_pairs_forward(px["codes"][:3], px["seqs"][:3], 1)
        assert e.value.code == STATE and "the loaded scorer is DIN" in str(e.value)

        def din_weights(en):
            w = np.full((n, 4), np.nan, np.float32)
            en._chk(lib.dm_jtm_child_weights(en._h, _ptr(cat["row_off"], N.i64p), i32p(cat["row_ids"]), i32p(node), n, L, old, level, 0, 0, 1, f32p(w)))
            return w
        from dismember_amd import Engine
        t = D.tree()
        other = Engine(0)
        try:
            other.load_tree(t["codes"], t["ids"], t["is_leaf"], D.DEPTH)
            other.load_id_maps(cat["map_ids"], cat["map_codes"])
            other.load_weights_din_synthetic(32, D.NI, 9, tree_depth=D.DEPTH, rho=0.9)
            want = din_weights(other)
        finally:
            other.close()
        assert np.isfinite(want).all() and din_weights(eng).tobytes() == want.tobytes()
        # ... and back
        eng.load_weights_deepfm(D.weights(E, L), E, L, D.NI)
        still_good()
    finally:
        _uncache(eng, L)
        eng.close()


# --------------------------------------------------------------------------- 8. the task
def test_jtm_tree_learning_task_with_a_deepfm_checkpoint(tmp_path):
    """TDMInitializeTree -> TDMTrainDeepModel (DeepFM, 120 iterations) -> JTMTreeLearning from one conf file: the learned projection is a
    bijection onto level-12 leaf codes, the written tree reloads and TDM serves on it."""
    from dismember_amd import TDM, tasks, tree_io
    from test_tasks import _conf
    conf = _conf(tmp_path, **{"model.iteration_number": 120, "model.show_progress_interval": 60, "model.deep_model": "DeepFM",
                              "tree.deep_model": "DeepFM", "tree.data_path": str(tmp_path / "train_data.csv"),
                              "tree.tree_protobuf_path": str(tmp_path / "tdm_tree.bin"), "tree.model_path": str(tmp_path / "tdm_model.bin"),
                              "tree.gap": 2, "tree.seq_len": 10, "tree.hierarchical_preference": "false", "tree.min_level": 0,
                              "tree.thread_number": 0})
    tasks.tdm_initialize_tree(conf)
    r = tasks.tdm_train_deep_model(conf, time_recommend=False)
    assert len(r["losses"]) == 120 and r["engine"].scorer == "deepfm"
    r["engine"].close()
    old = tree_io.read_tree_file(str(tmp_path / "tdm_tree.bin"))
    j = tasks.jtm_tree_learning(conf)
    eng = j["engine"]
    try:
        assert eng.scorer == "deepfm"
        proj = j["projection"]
        new = tree_io.read_tree_file(str(tmp_path / "tdm_tree.bin"))
        assert sorted(proj) == sorted(old["leaf_ids"].tolist())
        codes = np.array(list(proj.values()))
        assert len(set(codes.tolist())) == len(codes) and (codes >= (1 << 12) - 1).all() and (codes < (1 << 13) - 1).all()
        assert dict(zip(new["leaf_ids"].tolist(), new["leaf_codes"].tolist())) == {int(k): int(v) for k, v in proj.items()}
        assert new["max_level"] == 12
        assert codes.tolist() != [dict(zip(old["leaf_ids"].tolist(), old["leaf_codes"].tolist()))[k] for k in proj]      # the tree was learned, not copied
        eng.load_tree_file(str(tmp_path / "tdm_tree.bin"))                  # the written file is a valid index
        q = np.array([0, 0, 2126, 204, 3257, 3439, 996, 1681, 3438, 1882], np.int32)
        recs = TDM(eng, "DeepFM").recommend(q, 10, 20)
        assert len(recs) == 10 and all(int(i) in proj for i, _ in recs)
    finally:
        eng.close()
