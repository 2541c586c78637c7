"""OTM with the DeepFM scorer on the device (csrc/dfm_otm.hip.inc, csrc/otm_train.hip.inc): the fused beam kernel, the targets, one
training iteration, refusals, facade and the conf task.

The method is the one of tests/test_gpu_deepfm.py: the reference's integer logic is replayed on the DEVICE's own scores (codes
bit-exact), every traced score is compared with the float64 restatement under |gpu - ref64| <= 1e-5 + 1e-4 |ref64|.  The cases, the
restatement and the replay are tests/dfm_otm_ref.py; tests/test_dfm_otm_host.py shows on the same cases that the reference's own float32
arithmetic meets the tolerance and that the tolerance sees a missing term or a 5 % error in W1a."""
import ctypes as C
import threading

import numpy as np
import pytest

import dfm_otm_ref as D

pytestmark = pytest.mark.gpu


def live_allocs():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


@pytest.fixture(scope="module")
def engines():
    """one engine per model (E, L, leaf level of the tree, kind), loaded once"""
    from dismember_amd import Engine
    cache = {}

    def get(c):
        E, L, _, leaf_level, _, kind = c
        key = (E, L, 9 if leaf_level <= 9 else 10, kind)
        if key not in cache:
            w, ni = D.model(*key)
            eng = Engine(0)
            eng.load_weights_deepfm(w, E, L, ni)
            cache[key] = eng
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def traced(eng, c, seqs=None):
    E, L, beam, leaf_level, U, kind = c
    seqs = D.case_inputs(c)[2] if seqs is None else seqs
    levels = max(1, len(D.level_counts(beam, leaf_level)))
    r = eng.otm_beam_search_trace(seqs, beam, leaf_level, levels)
    return r[:3], r[3:]


def check_case(eng, c):
    E, L, beam, leaf_level, U, kind = c
    w, ni, seqs = D.case_inputs(c)
    eng.timing_reset()
    outs, trace = traced(eng, c)
    assert eng.timing_get_kind(42)[0] == 1                                    # EV_DFM_OTM: one launch per call
    assert eng.last_beam_kernel() == "dfm_otm_beam_kernel<%d, %d>" % ({24: 32}.get(E, E), (L + 2 + 15) // 16)
    rows = C.c_int64(0)
    from dismember_amd import _native as N
    assert N.lib().dm_last_scored_rows(eng._h, C.byref(rows)) == 0 and rows.value == U * sum(D.level_counts(beam, leaf_level))
    worst, ties = D.replay(seqs, beam, leaf_level, outs, trace, lambda u, codes: D.ref_scores(w, E, L, ni, codes, seqs[u]))
    print("%s: traced score error / tolerance: max %.3f, ties at a cut: %d" % (D.case_id(c), worst, ties))
    plain = eng.otm_beam_search(seqs, beam, leaf_level)                       # trace on = trace off for the outputs
    for x, y in zip(outs, plain):
        assert x.tobytes() == y.tobytes()
    return outs, trace, ties


@pytest.mark.parametrize("c", [c for c in D.CASES if c[5] == "plain"], ids=D.case_id)
def test_search_trace_replay(engines, c):
    E, L, beam, leaf_level, U, kind = c
    outs, trace, _ = check_case(engines(c), c)
    if not D.level_counts(beam, leaf_level):                                  # leaf_level = s: the frontier itself, scores 0
        start, _ = D.level_start(beam)
        ids, sc, cnt = outs
        assert (cnt == start + 1).all() and (ids[:, :start + 1] == np.arange(start, 2 * start + 1)).all() and (sc == 0).all()
        assert (trace[2] == 0).all()


def test_twin_rows_cut_on_the_position_tiebreak(engines):
    c = (16, 10, 21, 9, 33, "twins")
    outs, trace, ties = check_case(engines(c), c)
    tc, ts, tn = trace
    assert ties > 0                                                           # equal scores at a cut: the case is about the tiebreak
    pairs = ts[:, 1:, 0:42:2] == ts[:, 1:, 1:42:2]                            # the twins' scores are bit-equal, wherever their tile puts them
    assert pairs.all()


def test_nan_row_orders_first(engines):
    c = (16, 10, 20, 9, 33, "nan")
    outs, trace, _ = check_case(engines(c), c)
    tc, ts, tn = trace
    for u in (0, 2):
        i = int(np.flatnonzero(tc[u, 0, :tn[u, 0]] == D.NAN_CODE)[0])
        assert np.isnan(ts[u, 0, i]) and np.isnan(ts[u, 0, :32]).sum() == 1
        assert tc[u, 1, :2].tolist() == [2 * D.NAN_CODE + 1, 2 * D.NAN_CODE + 2]
    u = D.NAN_USER                                                            # every score NaN: one canonical NaN, the order is the position order
    assert all(np.isnan(ts[u, it, :tn[u, it]]).all() for it in range(tn.shape[1]))
    assert tc[u, 1, :40].tolist() == [x for k in range(31, 51) for x in (2 * k + 1, 2 * k + 2)]      # the first 20 of level 5's 32 nodes


def test_byte_identity_across_batch_grid_entry_point_and_clone(engines, monkeypatch):
    c = (16, 10, 20, 9, 33, "plain")
    E, L, beam, leaf_level, U, _ = c
    eng = engines(c)
    seqs = D.case_inputs(c)[2]
    base_o, base_t = traced(eng, c)
    again_o, again_t = traced(eng, c)                                         # a second run
    for x, y in zip(base_o + base_t, again_o + again_t):
        assert x.tobytes() == y.tobytes()
    for u in (0, 1, 7, 32):                                                   # a user alone = the same user among 33
        o, t = traced(eng, c, seqs[u:u + 1])
        for x, y in zip(base_o + base_t, o + t):
            assert x[u:u + 1].tobytes() == y.tobytes(), u
    monkeypatch.setenv("DM_DFM_OTM_GRID", "2")                                # 33 users on 2 workgroups: a second, partial round of the user loop
    o, t = traced(eng, c)
    monkeypatch.delenv("DM_DFM_OTM_GRID")
    for x, y in zip(base_o + base_t, o + t):
        assert x.tobytes() == y.tobytes()
    # device-resident; one code outside the table counts as padding there (the host entry points reject it)
    ni = D.case_inputs(c)[1]
    dseqs = seqs.copy()
    pads = np.argwhere(dseqs == -1)
    pu, pj = [p for p in pads if p[0] not in (1,)][0]
    dseqs[pu, pj] = ni + 5
    d_seq, d_ids, d_sc, d_cnt = eng.dev_alloc(dseqs.nbytes), eng.dev_alloc(U * 2 * beam * 4), eng.dev_alloc(U * 2 * beam * 4), eng.dev_alloc(U * 4)
    try:
        eng.h2d(d_seq, dseqs)
        eng.otm_beam_search_dev(d_seq, U, L, beam, leaf_level, d_ids, d_sc, d_cnt)
        eng.synchronize()
        ids = np.empty((U, 2 * beam), np.int32); sc = np.empty((U, 2 * beam), np.float32); cnt = np.empty(U, np.int32)
        eng.d2h(ids, d_ids); eng.d2h(sc, d_sc); eng.d2h(cnt, d_cnt)
    finally:
        for p in (d_seq, d_ids, d_sc, d_cnt):
            eng.dev_free(p)
    for x, y in zip(base_o, (ids, sc, cnt)):
        assert x.tobytes() == y.tobytes()
    from dismember_amd import DismemberError
    with pytest.raises(DismemberError) as e:
        eng.otm_beam_search(dseqs, beam, leaf_level)
    assert e.value.code == -4
    cl = eng.clone()                                                          # a dm_clone handle
    try:
        o, t = traced(cl, c)
        for x, y in zip(base_o + base_t, o + t):
            assert x.tobytes() == y.tobytes()
    finally:
        cl.close()


def test_facade_recommend(engines):
    from dismember_amd import OTM
    c = (16, 10, 20, 9, 33, "plain")
    eng = engines(c)
    ni, seqs = D.case_inputs(c)[1:]
    rng = np.random.default_rng(4)
    leaves = rng.permutation(np.arange(511, 1023))[:400]                      # 400 items on 400 of the 512 leaves
    mapping = {int(i + 1): int(n) for i, n in enumerate(leaves)}
    otm = OTM(eng, mapping, "DeepFM")
    assert otm.leaf_level == 9 and not otm.use_mask
    inv = {v: k for k, v in mapping.items()}
    items = np.array([[inv.get(int(n), 0) for n in row] for row in seqs])     # histories of item ids; unmapped nodes and pads -> 0 -> -1
    codes = np.array([[mapping.get(int(i), -1) for i in row] for row in items], np.int32)
    ids, sc, cnt = eng.otm_beam_search(codes, 20, 9)
    n2i = np.full(ni, -1, np.int32)
    for item, node in mapping.items():
        n2i[node] = item
    recs = otm.recommend(items, 7, 20)
    for u in range(items.shape[0]):
        want = D.otm_finalize(ids[u, :cnt[u]], sc[u, :cnt[u]], n2i, 7)
        assert [r[0] for r in recs[u]] == [x[0] for x in want]
        assert np.allclose([r[1] for r in recs[u]], [x[1] for x in want], rtol=1e-6, atol=0)
    assert otm.recommend(items[0].tolist(), 7, 20) == recs[0]


# --------------------------------------------------------------------------- targets
def _device_targets(tr, targets, seqs, mode):
    """dm_deepfm_otm_pseudo_targets -> per level, per user [(node, label)] in list order"""
    from dismember_amd import _native as N
    seqs, off, flat = tr._flatten(seqs, targets)
    U, levels, NT = seqs.shape[0], tr.leaf_level - tr.start_level, max(int(off[-1]), 1)
    nodes = np.empty((levels, NT), np.int32); labels = np.empty((levels, NT), np.float64); counts = np.empty((levels, U), np.int32)
    opts = tr._opts(mode)
    p = lambda a, t: a.ctypes.data_as(t)
    tr.e._chk(N.lib().dm_deepfm_otm_pseudo_targets(tr.e._h, p(seqs, N.i32p), U, tr.L, p(off, N.i64p), p(flat, N.i32p), C.byref(opts),
                                                   p(nodes, N.i32p), p(labels, C.POINTER(C.c_double)), p(counts, N.i32p)))
    return [[list(zip(nodes[lv, int(off[u]):int(off[u]) + int(counts[lv, u])].tolist(),
                      labels[lv, int(off[u]):int(off[u]) + int(counts[lv, u])].tolist())) for u in range(U)] for lv in range(levels)]


def test_pseudo_targets_ragged_batch():
    from dismember_amd import Engine
    from dismember_amd.otm_train import OTMTrainer
    targets = D.ragged_targets()
    U, leaf, beam, E, L = len(targets), D.RAGGED_TARGETS_LEAF, 20, 16, 10
    w, ni = D.model(E, L, 9)
    seqs = np.random.default_rng(8).integers(0, ni, (U, L)).astype(np.int32)
    seqs[3] = -1
    eng = Engine(0)
    try:
        eng.load_weights_deepfm(w, E, L, ni)
        tr = OTMTrainer(eng, leaf_level=leaf, beam=beam, seq_len=L)
        for mode in ("pseudo", "normal"):
            got = _device_targets(tr, targets, seqs, mode)
            want = D.pseudo_targets(targets, beam, leaf, mode)
            assert got == want, mode                                          # nodes, order and labels, exactly
            assert all(lab == 1.0 for lv in got for user in lv for _, lab in user)
        d = tr.optimal_pseudo_targets(targets, seqs)                          # the trainer's dict view
        assert d[0][2] == dict(D.pseudo_targets(targets, beam, leaf)[0][2])
    finally:
        eng.close()


# --------------------------------------------------------------------------- one training iteration
@pytest.mark.parametrize("mode", ["pseudo", "normal"])
def test_train_batch_equals_the_row_steps(mode):
    """dm_deepfm_otm_train_batch == traced search with fixed weights, then per level the batch of the restatement through
    dm_deepfm_train_forward_backward and dm_deepfm_adam_step: weights, moments and losses, bit for bit"""
    from dismember_amd import Engine
    from dismember_amd.otm_train import OTMTrainer
    E, L, beam, leaf, U = 16, 10, 20, 9, 8
    w, ni = D.model(E, L, 9)
    seqs = D.histories(L, ni, 33)[:U]
    targets = D.ragged_targets(20)[1:1 + U]
    a, b, fresh = Engine(0), Engine(0), Engine(0)
    try:
        a.load_weights_deepfm(w, E, L, ni); b.load_weights_deepfm(w, E, L, ni)
        tr = OTMTrainer(a, leaf_level=leaf, beam=beam, seq_len=L, lr=1e-3)
        losses = tr.train_batch(seqs, targets, mode)
        st = tr.last_stats()
        counts = D.level_counts(beam, leaf)
        assert len(losses) == len(counts) and st["pseudo_target_forward_rows"] == 0 and st["rows_trained"] == U * sum(counts)
        b.deepfm_train_init(lr=1e-3)
        levels = len(counts)
        _, _, _, tc, ts, tn = b.otm_beam_search_trace(seqs, beam, leaf, levels)
        tgt = D.pseudo_targets(targets, beam, leaf, mode)
        want = []
        for it in range(levels):
            codes, rows, labels = D.level_batch(tc, tn, it, tgt[it], seqs)
            if it == 0:
                assert labels.sum() > 0                                       # level 5 holds all 32 nodes: every target's ancestor is a candidate
            want.append(b.deepfm_train_forward_backward(codes, rows, labels))
            b.deepfm_adam_step()
        assert losses == want and all(np.isfinite(losses))
        for what in ("weights", "s", "r"):
            assert a.deepfm_train_download(what).tobytes() == b.deepfm_train_download(what).tobytes(), what
        assert a.deepfm_train_download("weights").tobytes() != w.tobytes()
        # serving after the iteration == a fresh handle loaded from the downloaded weights
        fresh.load_weights_deepfm(a.deepfm_train_download("weights"), E, L, ni)
        x = a.otm_beam_search_trace(D.histories(L, ni, 33), beam, leaf, levels)
        y = fresh.otm_beam_search_trace(D.histories(L, ni, 33), beam, leaf, levels)
        for p, q in zip(x, y):
            assert p.tobytes() == q.tobytes()
    finally:
        a.close(); b.close(); fresh.close()


# --------------------------------------------------------------------------- refusals
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_refusals(fixture_w32):
    from dismember_amd import Engine, _native as N
    from dismember_amd.comm import Comm
    E, L, beam, leaf = 16, 10, 20, 9
    w, ni = D.model(E, L, 9)
    eng, din = Engine(0), Engine(0)
    lib = N.lib()
    p32 = lambda a: a.ctypes.data_as(N.i32p)
    f32p = lambda a: a.ctypes.data_as(N.f32p)
    f64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    i64p = lambda a: a.ctypes.data_as(N.i64p)
    seq, seq9 = np.full((1, L), 5, np.int32), np.full((1, L - 1), 5, np.int32)
    ids, sc, cnt = np.zeros(2 * 1024, np.int32), np.zeros(2 * 1024, np.float32), np.zeros(4, np.int32)
    tcb, tsb, tnb = np.zeros(8 * 1056, np.int32), np.zeros(8 * 1056, np.float32), np.zeros(8, np.int32)
    off, tgt = np.array([0, 1], np.int64), np.array([600], np.int32)
    on, ol, oc = np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.int32)
    loss, nlev = np.zeros(16, np.float64), C.c_int(0)

    def calls(h, s, L_, beam_, opts, d_buf):
        return {
            "dm_deepfm_otm_beam_search": lambda: lib.dm_deepfm_otm_beam_search(h, p32(s), 1, L_, beam_, leaf, p32(ids), f32p(sc), p32(cnt)),
            "dm_deepfm_otm_beam_search_trace": lambda: lib.dm_deepfm_otm_beam_search_trace(h, p32(s), 1, L_, beam_, leaf, p32(ids), f32p(sc), p32(cnt), 5,
                                                                                           p32(tcb), f32p(tsb), p32(tnb)),
            "dm_deepfm_otm_beam_search_dev": lambda: lib.dm_deepfm_otm_beam_search_dev(h, d_buf, 1, L_, beam_, leaf, d_buf, d_buf, d_buf),
            "dm_deepfm_otm_pseudo_targets": lambda: lib.dm_deepfm_otm_pseudo_targets(h, p32(s), 1, L_, i64p(off), p32(tgt), C.byref(opts), p32(on), f64p(ol), p32(oc)),
            "dm_deepfm_otm_train_batch": lambda: lib.dm_deepfm_otm_train_batch(h, p32(s), 1, L_, i64p(off), p32(tgt), C.byref(opts), f64p(loss), C.byref(nlev)),
        }

    def refused(h, table, names, code, word):
        for name in names:
            rc = table[name]()
            msg = (lib.dm_last_error(h) or b"").decode()
            assert rc == code, (name, rc, msg)
            assert word in msg, (name, msg)
    comms = [None, None]
    try:
        eng.load_weights_deepfm(w, E, L, ni)
        din.load_weights_din(fixture_w32, 16, 8191)
        d_e, d_d = eng.dev_alloc(1 << 16), din.dev_alloc(1 << 16)
        before = live_allocs()
        searches = ["dm_deepfm_otm_beam_search", "dm_deepfm_otm_beam_search_trace", "dm_deepfm_otm_beam_search_dev"]
        train = ["dm_deepfm_otm_pseudo_targets", "dm_deepfm_otm_train_batch"]
        ok = N.OtmTrainOpts(beam, leaf, 0, 0)
        refused(din._h, calls(din._h, seq, L, beam, ok, d_d), searches + train, -3, "the loaded scorer is DIN")
        refused(eng._h, calls(eng._h, seq9, L - 1, beam, ok, d_e), searches + train, -1, "seq_len")
        refused(eng._h, calls(eng._h, seq, L, beam, N.OtmTrainOpts(beam, leaf, 1, 0), d_e), train, -1, "no mask")
        refused(eng._h, calls(eng._h, seq, L, 513, N.OtmTrainOpts(513, leaf, 0, 0), d_e), searches + train, -5, "beam too large")
        refused(eng._h, calls(eng._h, seq, L, beam, ok, d_e), ["dm_deepfm_otm_train_batch"], -3, "dm_deepfm_train_init")
        eng.deepfm_train_init()
        after_init = live_allocs()
        # a communicator with more than one rank (host transport: two ranks of one process)
        port = _free_port()

        def make(r):
            comms[r] = Comm(2, r, "127.0.0.1", port, transport="host")
        th = [threading.Thread(target=make, args=(r,)) for r in range(2)]
        [t.start() for t in th]; [t.join(60) for t in th]
        assert comms[0] is not None and comms[1] is not None
        eng.attach_comm(comms[0])
        refused(eng._h, calls(eng._h, seq, L, beam, ok, d_e), ["dm_deepfm_otm_train_batch"], -5, "communicator")
        eng.attach_comm(None)
        # the row step's limit: U * 2 beam rows, checked before anything runs (the arrays are never read)
        big = N.OtmTrainOpts(512, leaf, 0, 0)
        rc = lib.dm_deepfm_otm_train_batch(eng._h, p32(seq), 5000, L, i64p(off), p32(tgt), C.byref(big), f64p(loss), C.byref(nlev))
        assert rc == -5 and "4 194 240" in (lib.dm_last_error(eng._h) or b"").decode()      # 5000 * 1024 rows
        assert live_allocs() == after_init
        eng.deepfm_train_free()
        assert live_allocs() == before
        # the DIN entry points still refuse the DeepFM handle, and the handle still serves
        for name, call in {"dm_otm_beam_search": lambda: lib.dm_otm_beam_search(eng._h, p32(seq), 1, L, beam, leaf, p32(ids), f32p(sc), p32(cnt)),
                           "dm_otm_train_batch": lambda: lib.dm_otm_train_batch(eng._h, p32(seq), 1, L, i64p(off), p32(tgt), C.byref(ok), f64p(loss), C.byref(nlev)),
                           "dm_otm_pseudo_targets": lambda: lib.dm_otm_pseudo_targets(eng._h, p32(seq), 1, L, i64p(off), p32(tgt), C.byref(ok), p32(on), f64p(ol),
                                                                                      p32(oc))}.items():
            assert call() == -5 and "DeepFM" in (lib.dm_last_error(eng._h) or b"").decode(), name
        from dismember_amd import DismemberError
        with pytest.raises(DismemberError) as e:
            eng.otm_beam_search_f64(seq, beam, leaf)                          # the fp64 search keeps the library's refusal
        assert e.value.code == -5
        eng.dev_free(d_e); din.dev_free(d_d)
        c = (16, 10, 20, 9, 33, "plain")
        check_case(eng, c)
    finally:
        for cm in comms:
            if cm is not None:
                cm.close()
        eng.close(); din.close()


# --------------------------------------------------------------------------- the conf task
def test_conf_task_trains_saves_and_serves(tmp_path):
    from test_tasks import _otm_conf
    from dismember_amd import Engine, OTM, tasks
    from dismember_amd import otm_data as od
    conf = _otm_conf(tmp_path, **{"model.deep_model": "DeepFM"})
    r = tasks.otm_train_deep_model(conf, time_recommend=False, max_iterations=4)
    eng = r["engine"]
    e2 = Engine(0)
    try:
        levels = r["epoch_losses"]["epoch 1"]
        assert len(levels) == 12 - 4 and len(levels[0]) == 4 and np.isfinite(levels).all()
        assert eng.scorer_kind() == ("deepfm", r["params"]["seq_len"])
        q = [0, 0, 2126, 204, 3257, 3439, 996, 1681, 3438, 1882]
        before = OTM(eng, r["mapping"], "DeepFM").recommend(q, 10, 20)
        e2.load_model(r["params"]["model_path"])
        assert e2.scorer_kind() == ("deepfm", r["params"]["seq_len"])
        after = OTM(e2, od.load_mapping(r["params"]["mapping_path"]), "DeepFM").recommend(q, 10, 20)
        assert before == after and len(before) == 10
        with pytest.raises(ValueError, match="child-weight twin"):
            tasks.otm_construct_tree(conf, engine=e2)
    finally:
        eng.close(); e2.close()
