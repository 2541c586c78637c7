"""DeepFM on the device (csrc/deepfm.hip.inc): row forward, TDM beam search through the level pipeline, checkpoint, refusals, facade.

Scores are always compared as |gpu - ref64| <= 1e-5 + 1e-4 |ref64| against the float64 restatement of the reference's graph
(tests/deepfm_ref.py) — the project's fp32 contract (tests/test_gpu_parity.py); tests/test_deepfm_host.py shows on the same inputs that
the reference's own float32 arithmetic needs that much.  Tree indices and item ids are bit-exact: the oracle's integer logic is replayed
on the scores the device produced."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import deepfm_ref as R

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
NI_S = (1 << (R.SEARCH_DEPTH + 1)) - 1


def close(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b) <= ATOL + RTOL * np.abs(b)


@functools.lru_cache(maxsize=None)
def row_ref(E, L):
    w, codes, seqs = R.row_case(E, L)
    ref = R.forward(w, E, L, R.ROW_NUM_INDEX, codes, seqs, np.float64)
    ref.setflags(write=False)
    return w, codes, seqs, ref


def deepfm_engine(E, L, tree=None, w=None):
    from dismember_amd import Engine
    eng = Engine(0)
    if tree is not None:
        eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
        eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    if w is not None:
        eng.load_weights_deepfm(w, E, L, NI_S if tree is not None else R.ROW_NUM_INDEX)
    return eng


@pytest.fixture(scope="module")
def otree(oracle):
    tree, _, _ = R.search_case(16, 10)
    return oracle.TdmTree(tree["codes"], tree["ids"], tree["is_leaf"], tree["leaf_ids"], tree["leaf_codes"], tree["max_level"])


@pytest.fixture(scope="module")
def search_engines():
    """One engine per (E, L) of the search tests, loaded once."""
    engines = {}

    def get(E, L):
        if (E, L) not in engines:
            tree, w, _ = R.search_case(E, L)
            engines[(E, L)] = deepfm_engine(E, L, tree, w)
        return engines[(E, L)]
    yield get
    for e in engines.values():
        e.close()


# --------------------------------------------------------------------------- row forward
@pytest.mark.parametrize("E", R.ROW_E)
@pytest.mark.parametrize("L", R.ROW_L)
def test_row_forward(E, L):
    w, codes, seqs, ref = row_ref(E, L)
    assert (seqs[5] == -1).all() and codes[9] == -1
    eng = deepfm_engine(E, L, None, w)
    try:
        assert eng.scorer_kind() == ("deepfm", L)
        for B in R.ROW_B:
            got = eng.deepfm_forward(codes[:B], seqs[:B])
            assert got.dtype == np.float32 and got.shape == (B,)
            err = np.abs(got.astype(np.float64) - ref[:B]) / (ATOL + RTOL * np.abs(ref[:B]))
            print("E=%d L=%d B=%d error / tolerance: max %.3f" % (E, L, B, err.max()))
            assert close(got, ref[:B]).all(), (B, err.max())
    finally:
        eng.close()


def test_row_forward_errors():
    from dismember_amd import DismemberError
    w, codes, seqs, _ = row_ref(16, 10)
    eng = deepfm_engine(16, 10, None, w)
    try:
        with pytest.raises(DismemberError) as e:
            eng.deepfm_forward([R.ROW_NUM_INDEX], [[1] * 10])
        assert e.value.code == -4 and "valid index range" in str(e.value)
        with pytest.raises(DismemberError) as e:
            eng.deepfm_forward([1], [[1] * 9 + [-5]])
        assert e.value.code == -4
        with pytest.raises(DismemberError) as e:
            eng.deepfm_forward(codes[:3], seqs[:3, :9])                 # L differs from the model's
        assert e.value.code == -1
        assert close(eng.deepfm_forward(codes[:3], seqs[:3]), row_ref(16, 10)[3][:3]).all()      # the handle stays usable
    finally:
        eng.close()


# --------------------------------------------------------------------------- search
def replay(otree, eng, w, E, L, seqs, beam, topk, cut_beam=None, consumed=None, expect=None):
    """Trace the device search, replay the oracle's integer logic (level_step / finalize) on the device's own scores: every level's codes
    and the final ids and scores bit-exact, every traced score within tolerance of the restatement.  cut_beam / consumed / expect: the
    widened search of ONE user — the trace runs at the user's widened beam and its final list, with the consumed ids dropped, must be
    `expect` = (ids, scores) of the widened search."""
    trace_beam = cut_beam or beam
    ids, sc, cnt, tc, ts, tn = eng.tdm_beam_search_trace(seqs, trace_beam, topk, use_mask=False)
    level = trace_beam.bit_length() - 1
    start = (1 << level) - 1
    present = set(otree.codes.tolist())
    n_iter = otree.max_level - level + 1
    hist = R.history_codes(dict(leaf_ids=otree_leaf_ids(otree), leaf_codes=otree_leaf_codes(otree)), seqs)
    worst = 0.0
    for u in range(seqs.shape[0]):
        seq_codes, _ = otree.id_to_code(seqs[u])
        assert np.array_equal(seq_codes, hist[u]), u
        cand = np.array([c for c in range(start, 2 * start + 1) if c in present], np.int32)
        preds = np.zeros(cand.size, np.float32)
        leaves, all_codes, all_scores = [], [], []
        for it in range(n_iter):
            lc, lp, children = otree.level_step(trace_beam, cand, preds)
            leaves.insert(0, (lc, lp))
            n = int(tn[u, it])
            assert n == children.size, (u, it, n, children.size)
            if n:
                assert np.array_equal(tc[u, it, :n], children), (u, it)            # tree indices: bit-exact
                all_codes.append(children); all_scores.append(ts[u, it, :n].copy())
            cand, preds = children, ts[u, it, :n].copy()
        for it in range(n_iter, tn.shape[1]):
            assert tn[u, it] == 0
        if all_codes:
            codes_u = np.concatenate(all_codes); got = np.concatenate(all_scores)
            ref = R.forward(w, E, L, NI_S, codes_u, np.tile(seq_codes, (codes_u.size, 1)), np.float64)
            worst = max(worst, float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max()))
            assert close(got, ref).all(), u
        fl_c = np.concatenate([a for a, _ in leaves]) if leaves else np.zeros(0, np.int32)
        fl_p = np.concatenate([b for _, b in leaves]) if leaves else np.zeros(0, np.float32)
        if expect is None:
            fi, fs = otree.finalize(fl_c, fl_p, topk)
            assert cnt[u] == fi.size, (u, cnt[u], fi.size)
            assert np.array_equal(ids[u, :cnt[u]], fi), u                             # item ids: bit-exact
            assert np.array_equal(sc[u, :cnt[u]], fs), u
        else:
            fi, fs = otree.finalize(fl_c, fl_p, topk, consumed=consumed)
            assert np.array_equal(expect[0], fi) and np.array_equal(expect[1], fs)
    print("E=%d L=%d beam=%d traced score error / tolerance: max %.3f" % (E, L, trace_beam, worst))
    return ids, sc, cnt


def otree_leaf_ids(otree):
    return R.search_case(16, 10)[0]["leaf_ids"]


def otree_leaf_codes(otree):
    return R.search_case(16, 10)[0]["leaf_codes"]


@pytest.mark.parametrize("E", R.SEARCH_E)
@pytest.mark.parametrize("L", R.SEARCH_L)
@pytest.mark.parametrize("beam", [3, 20, 24, 50])
def test_search_trace_replay(otree, search_engines, E, L, beam):
    _, w, seqs = R.search_case(E, L)
    eng = search_engines(E, L)
    ids, sc, cnt = replay(otree, eng, w, E, L, seqs, beam, 10)
    name = eng.last_beam_kernel()
    assert "level pipeline" in name and "dfm_level_kernel" in name, name
    assert eng.last_scored_rows() > 0
    # the plain entry point returns the traced search's bytes
    i2, s2, c2 = eng.tdm_beam_search(seqs, beam, 10, use_mask=False)
    assert np.array_equal(c2, cnt)
    for u in range(seqs.shape[0]):
        assert np.array_equal(i2[u, :c2[u]], ids[u, :cnt[u]]) and np.array_equal(s2[u, :c2[u]], sc[u, :cnt[u]])


def test_search_consumed_widened(otree, search_engines):
    E, L, beam, topk = 16, 10, 20, 10
    _, w, seqs = R.search_case(E, L)
    eng = search_engines(E, L)
    rng = np.random.default_rng(3)
    leaf_ids = otree_leaf_ids(otree)
    base, _, bcnt = eng.tdm_beam_search(seqs, beam, topk, use_mask=False)
    # consumed lists: the user's own top results first (so that the filter bites), then random items; (n + topk) // 2 gives the widened
    # beams 20 (not widened), 25 and 30 — all on start level 4, like beam 20
    n_cons = [4, 40, 50]
    consumed = []
    for u in range(seqs.shape[0]):
        own = base[u, :min(3, bcnt[u])].tolist()
        rest = [int(i) for i in rng.permutation(leaf_ids) if int(i) not in own][:n_cons[u % 3] - len(own)]
        consumed.append(np.array(own + rest, np.int32))
    ids, sc, cnt = eng.tdm_beam_search(seqs, beam, topk, use_mask=False, consumed=consumed, widen_consumed=True)
    for u in range(seqs.shape[0]):
        assert not set(ids[u, :cnt[u]].tolist()) & set(consumed[u].tolist())
        wide = max((len(consumed[u]) + topk) // 2, beam)
        replay(otree, eng, w, E, L, seqs[u:u + 1], beam, topk, cut_beam=wide, consumed=consumed[u].tolist(),
               expect=(ids[u, :cnt[u]], sc[u, :cnt[u]]))


def test_search_host_dev_clone_and_rerun_identical(search_engines):
    E, L, beam, topk = 128, 15, 24, 10
    _, w, seqs = R.search_case(E, L)
    eng = search_engines(E, L)
    U = seqs.shape[0]
    a = eng.tdm_beam_search(seqs, beam, topk, use_mask=False)
    b = eng.tdm_beam_search(seqs, beam, topk, use_mask=False)                 # two runs: the same bits
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # device-resident request
    d_seq, d_ids, d_sc, d_cnt = eng.dev_alloc(seqs.nbytes), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * 4)
    try:
        eng.h2d(d_seq, seqs)
        eng.tdm_beam_search_dev(d_seq, U, L, beam, topk, d_ids, d_sc, d_cnt, use_mask=False)
        eng.synchronize()
        ids = np.empty((U, topk), np.int32); sc = np.empty((U, topk), np.float32); cnt = np.empty(U, np.int32)
        eng.d2h(ids, d_ids); eng.d2h(sc, d_sc); eng.d2h(cnt, d_cnt)
    finally:
        for p in (d_seq, d_ids, d_sc, d_cnt):
            eng.dev_free(p)
    assert np.array_equal(cnt, a[2])
    for u in range(U):
        assert ids[u, :cnt[u]].tobytes() == a[0][u, :cnt[u]].tobytes() and sc[u, :cnt[u]].tobytes() == a[1][u, :cnt[u]].tobytes()
    # a dm_clone clone serves the same model through the shared storage
    c = eng.clone()
    try:
        assert c.scorer_kind() == ("deepfm", L)
        cc = c.tdm_beam_search(seqs, beam, topk, use_mask=False)
        for x, y in zip(a, cc):
            assert x.tobytes() == y.tobytes()
        # a single-user request (the serving loop's shape) gives the batch's row
        one = c.tdm_beam_search(seqs[3], beam, topk, use_mask=False)
        assert one[0][0, :one[2][0]].tobytes() == a[0][3, :a[2][3]].tobytes() and one[1][0, :one[2][0]].tobytes() == a[1][3, :a[2][3]].tobytes()
    finally:
        c.close()


# --------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("E", [16, 24])
def test_checkpoint_roundtrip(tmp_path, E):
    from dismember_amd import Engine
    L = 10
    tree, _, seqs = R.search_case(16, L)
    w = R.random_deepfm_weights(np.random.default_rng(40 + E), E, L, NI_S)
    eng = deepfm_engine(E, L, tree, w)
    fresh = Engine(0)
    try:
        a = eng.tdm_beam_search(seqs, 20, 10, use_mask=False)
        path = str(tmp_path / "deepfm.ckpt")
        eng.save_model(path)
        hd = open(path, "rb").read(72)
        _, dtype, embed, _, _, _, kind, seq_len = struct.unpack("<8i", hd[8:40])
        _, n_elems = struct.unpack("<2q", hd[40:56])
        assert (dtype, embed, kind, seq_len) == (0, E, 1, L) and n_elems == R.deepfm_param_count(E, L, NI_S)      # the model's own layout
        fresh.load_model(path)
        assert fresh.scorer == "deepfm" and fresh.scorer_kind() == ("deepfm", L)
        b = fresh.tdm_beam_search(seqs, 20, 10, use_mask=False)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    finally:
        eng.close(); fresh.close()


def test_din_checkpoint_reserved_words_zero(tmp_path, engine_fixture):
    from dismember_amd import Engine
    path = str(tmp_path / "din.ckpt")
    engine_fixture.save_model(path)
    hd = open(path, "rb").read(72)
    assert struct.unpack("<2i", hd[32:40]) == (0, 0)
    fresh = Engine(0)
    try:
        fresh.load_model(path)
        assert fresh.scorer == "din"
    finally:
        fresh.close()


# --------------------------------------------------------------------------- refusals and switching
def test_refusals_and_switch_back_to_din(otree, fixture_tree, fixture_w32, oracle_tree, oracle_din32):
    from dismember_amd import DismemberError, _native as N
    from test_gpu_parity import replay_and_check
    E, L = 16, 10
    tree, w, seqs = R.search_case(E, L)
    eng = deepfm_engine(E, L, tree, None)
    lib, h = N.lib(), eng._h
    try:
        # loading: a wrong n_elems, E, L -> INVALID; DM_F64 -> UNSUPPORTED
        def load(dt, E_, L_, n):
            return lib.dm_load_weights_deepfm(h, dt, E_, L_, NI_S, w.ctypes.data_as(C.c_void_p), n)
        assert load(0, E, L, w.size - 1) == -1
        assert load(0, E, L + 1, w.size) == -1
        assert load(0, 0, L, w.size) == -1 and load(0, 129, L, w.size) == -1 and load(0, E, 33, w.size) == -1 and load(0, E, 0, w.size) == -1
        assert load(1, E, L, w.size) == -5
        with pytest.raises(DismemberError) as e:      # no model yet
            eng.deepfm_forward([1], [[1] * L])
        assert e.value.code == -3
        eng.load_weights_deepfm(w, E, L, NI_S)
        base = eng.tdm_beam_search(seqs, 20, 10, use_mask=False)

        i32 = lambda *v: np.array(v, np.int32)
        p32 = lambda a: a.ctypes.data_as(N.i32p)
        one_seq, codes1 = np.full((1, L), 1, np.int32), i32(1)
        out_i, out_f, out_c = np.zeros(256, np.int32), np.zeros(256, np.float32), np.zeros(16, np.int32)
        out_d = np.zeros(256, np.float64)
        f32p, f64p = lambda a: a.ctypes.data_as(N.f32p), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        off2 = np.array([0, 1], np.int64)
        i64p = lambda a: a.ctypes.data_as(N.i64p)
        d_buf = eng.dev_alloc(4096)
        adam = N.AdamOpts(1e-3, 0.0, 0.9, 0.999, 1e-8)
        sopt = N.SampleOpts(1, 0, 20, 0, 0)
        oopt = N.OtmTrainOpts(4, 5, 0, 0)
        neg = np.full(R.SEARCH_DEPTH + 1, 2, np.int32)
        n64, nlev, loss = C.c_int64(0), C.c_int(0), C.c_float(0)
        dptr = C.c_void_p()
        refused = {
            "dm_din_forward": lambda: lib.dm_din_forward(h, p32(codes1), p32(one_seq), None, 0, 1, L, out_f.ctypes.data_as(C.c_void_p)),
            "dm_otm_beam_search": lambda: lib.dm_otm_beam_search(h, p32(one_seq), 1, L, 4, 5, p32(out_i), f32p(out_f), p32(out_c)),
            "dm_otm_beam_search_trace": lambda: lib.dm_otm_beam_search_trace(h, p32(one_seq), 1, L, 4, 5, p32(out_i), f32p(out_f), p32(out_c), 2,
                                                                             p32(np.zeros(64, np.int32)), f32p(np.zeros(64, np.float32)), p32(np.zeros(2, np.int32))),
            "dm_otm_beam_search_f64": lambda: lib.dm_otm_beam_search_f64(h, p32(one_seq), 1, L, 4, 5, p32(out_i), f64p(out_d), p32(out_c)),
            "dm_otm_beam_search_dev": lambda: lib.dm_otm_beam_search_dev(h, d_buf, 1, L, 4, 5, d_buf, d_buf, d_buf),
            "dm_otm_child_weights": lambda: lib.dm_otm_child_weights(h, i64p(off2), p32(one_seq), p32(i32(1)), 1, L, 1, 2, 0, f64p(out_d)),
            "dm_otm_pseudo_targets": lambda: lib.dm_otm_pseudo_targets(h, p32(one_seq), 1, L, i64p(off2), p32(i32(40)), C.byref(oopt), p32(out_i), f64p(out_d), p32(out_c)),
            "dm_otm_train_batch": lambda: lib.dm_otm_train_batch(h, p32(one_seq), 1, L, i64p(off2), p32(i32(40)), C.byref(oopt), f64p(out_d), C.byref(nlev)),
            "dm_tdm_bruteforce_topk": lambda: lib.dm_tdm_bruteforce_topk(h, p32(seqs[:1].copy()), 1, L, 5, 0, p32(out_i), f32p(out_f), p32(out_c)),
            "dm_jtm_child_weights": lambda: lib.dm_jtm_child_weights(h, i64p(off2), p32(seqs[:1].copy()), p32(i32(1)), 1, L, 1, 2, 0, 0, 0, f32p(out_f)),
            "dm_jtm_child_weights_cached": lambda: lib.dm_jtm_child_weights_cached(h, p32(i32(1)), 0, 1, 1, 2, 0, 0, 0, f32p(out_f)),
            "dm_jtm_step_cached": lambda: lib.dm_jtm_step_cached(h, p32(i32(1)), p32(i32(1)), 1, 1, 2, 0, 0, 0, 0, p32(out_i)),
            "dm_jtm_optimize_cached": lambda: lib.dm_jtm_optimize_cached(h, p32(i32(600)), 1, R.SEARCH_DEPTH, 2, 0, 0, 0, p32(out_i), None),
            "dm_train_init": lambda: lib.dm_train_init(h, C.byref(adam)),
            "dm_train_forward_backward": lambda: lib.dm_train_forward_backward(h, p32(codes1), p32(one_seq), None, 0, f32p(np.ones(1, np.float32)), 1, L, C.byref(loss)),
            "dm_train_forward_backward_dev": lambda: lib.dm_train_forward_backward_dev(h, d_buf, d_buf, None, d_buf, 1, L, None),
            "dm_train_forward_backward_grouped_dev": lambda: lib.dm_train_forward_backward_grouped_dev(h, d_buf, None, d_buf, d_buf, 1, 1, L, None),
            "dm_adam_step": lambda: lib.dm_adam_step(h, 1.0),
            "dm_train_download": lambda: lib.dm_train_download(h, 0, out_f.ctypes.data_as(C.c_void_p), 256),
            "dm_train_dense_block": lambda: lib.dm_train_dense_block(h, C.byref(dptr), C.byref(n64)),
            "dm_train_export_rows": lambda: lib.dm_train_export_rows(h, None, None, 0, C.byref(n64)),
            "dm_train_add_rows": lambda: lib.dm_train_add_rows(h, d_buf, d_buf, 0),
            "dm_train_sync_gradients": lambda: lib.dm_train_sync_gradients(h),
            "dm_tdm_make_train_batch": lambda: lib.dm_tdm_make_train_batch(h, p32(seqs[:1].copy()), p32(i32(int(tree["leaf_ids"][0]))), 1, L, p32(neg), neg.size,
                                                                           C.byref(sopt), None, None, None, None, 0, C.byref(n64)),
            "dm_tdm_sample_train_batch_dev": lambda: lib.dm_tdm_sample_train_batch_dev(h, None, None, 1, L, p32(neg), neg.size, C.byref(sopt), None, None, None, None,
                                                                                       0, C.byref(n64)),
            "dm_set_scorer_mode": lambda: lib.dm_set_scorer_mode(h, 0),
        }
        for name, call in refused.items():
            rc = call()
            msg = (lib.dm_last_error(h) or b"").decode()
            assert rc == -5, (name, rc, msg)
            assert "DeepFM" in msg, (name, msg)
        eng.dev_free(d_buf)
        # the same handle still searches, bit for bit
        again = eng.tdm_beam_search(seqs, 20, 10, use_mask=False)
        for x, y in zip(base, again):
            assert x.tobytes() == y.tobytes()
        # use_mask = 1 and a foreign L are INVALID
        with pytest.raises(DismemberError) as e:
            eng.tdm_beam_search(seqs, 20, 10, use_mask=True)
        assert e.value.code == -1 and "no mask" in str(e.value)
        with pytest.raises(DismemberError) as e:
            eng.tdm_beam_search(seqs[:, :9], 20, 10, use_mask=False)
        assert e.value.code == -1
        # DIN weights on the same handle switch it back: forward and search match the oracle again
        t = fixture_tree
        eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
        eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
        eng.load_weights_din(fixture_w32, 16, 8191)
        assert eng.scorer_kind() == ("din", 0)
        with pytest.raises(DismemberError) as e:
            eng.deepfm_forward([1], [[1] * L])
        assert e.value.code == -3
        rng = np.random.default_rng(11)
        codes = rng.integers(0, 8191, 100).astype(np.int32)
        hs = rng.integers(0, 8191, (100, 10)).astype(np.int32)
        hs[rng.random((100, 10)) < 0.2] = -1
        pad = np.flatnonzero(hs.reshape(-1) == -1).astype(np.int32)
        assert close(eng.din_forward(codes, hs, pad), oracle_din32.forward(codes, hs, pad)).all()
        from helpers import random_histories
        dseqs = random_histories(np.random.default_rng(120), t["leaf_ids"], 9, 10, unknown_prob=0.05)
        replay_and_check(oracle_tree, oracle_din32, eng, dseqs, 20, 10)
    finally:
        eng.close()


# --------------------------------------------------------------------------- facade
def test_facade_predict_and_recommend(search_engines):
    from dismember_amd import TDM
    from dismember_amd.facade import sigmoid
    E, L = 16, 10
    tree, w, seqs = R.search_case(E, L)
    eng = search_engines(E, L)
    tdm = TDM(eng, "DeepFM")
    target = int(tree["leaf_ids"][7])
    for u in (0, 1, 2, 5):
        codes, _ = eng.id_to_code(np.concatenate([seqs[u], [target]]).astype(np.int32))
        logit = eng.deepfm_forward(codes[-1:], codes[None, :-1])
        assert tdm.predict(seqs[u].tolist(), target) == float(sigmoid(np.float32(logit[0])))
        ref = R.forward(w, E, L, NI_S, codes[-1:], codes[None, :-1], np.float64)
        assert close(logit, ref).all()
    ids, sc, cnt, _, _, _ = eng.tdm_beam_search_trace(seqs, 20, 10, use_mask=False)
    recs = tdm.recommend(seqs, 10, 20)
    for u in range(seqs.shape[0]):
        assert [r[0] for r in recs[u]] == ids[u, :cnt[u]].tolist()
        assert np.array_equal(np.array([r[1] for r in recs[u]]), sigmoid(sc[u, :cnt[u]]))
    single = tdm.recommend(seqs[0].tolist(), 10, 20)
    assert [r[0] for r in single] == ids[0, :cnt[0]].tolist()
    items = TDM(eng, "din").recommend_items(seqs[0].tolist(), 10, 20)          # the engine's scorer decides, not the name
    assert items.tolist() == ids[0, :cnt[0]].tolist()
