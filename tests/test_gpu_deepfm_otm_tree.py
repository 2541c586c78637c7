"""OTM tree construction with the DeepFM scorer on the device (csrc/dfm_otm_tree.hip.inc): the child weights of the one-shot call and of
the prepared form, TreeConstruction on a DeepFM engine and the conf task.

Cases and the numpy restatement are tests/dfm_otm_tree_ref.py; tests/test_dfm_otm_tree_host.py shows on the same cases that the reference's
own float32 arithmetic meets the bound and that the bound sees a dropped row, left-out depths and a wrong parent index.  Three kinds of
check: (1) against the float64 restatement within the bound (the fp32 contract per logit, summed over the pairs a weight adds up); (2) the
device oracle, byte for byte: the weights are the restatement's double sums over the logits Engine.deepfm_pairs_forward returns for the
same (code, history) pairs; (3) byte identity across everything that must not matter."""
import ctypes as C

import numpy as np
import pytest

import dfm_otm_tree_ref as D

pytestmark = pytest.mark.gpu
INVALID, STATE, INDEX = -1, -3, -4
J = D.J


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
    """one engine per model (E, L), loaded once"""
    from dismember_amd import Engine
    cache = {}

    def get(E, L):
        if (E, L) not in cache:
            eng = Engine(0)
            eng.load_weights_deepfm(J.weights(E, L), E, L, D.NI)
            cache[(E, L)] = eng
        return cache[(E, L)]
    yield get
    for e in cache.values():
        e.close()


def oracle(eng, row_off, h, node, gap, seg):
    """the restatement's sums over the DEVICE's pair logits"""
    nchain = (2 << gap) - 2
    lg = eng.deepfm_pairs_forward(D.pair_codes(row_off, node, gap), h, seq_div=nchain).reshape(-1, nchain)
    return D.weights_from_logits(lg, row_off, gap, seg)


def one_shot(eng, row_off, h, node, old_level, gap):
    return eng.deepfm_otm_child_weights(row_off, h, node, old_level, old_level + gap)


def prepared(eng, row_off, h, node, old_level, gap):
    eng.deepfm_otm_tree_prepare(row_off, h)
    try:
        return eng.deepfm_otm_tree_weights(node, old_level, old_level + gap)
    finally:
        eng.deepfm_otm_tree_release()


WORST = [0.0]


# --------------------------------------------------------------------------- 1, 2. the restatement and the device oracle
@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_weights_match_the_restatement_and_the_pair_kernel(engines, monkeypatch, c):
    E, L, old_level, gap, rows, n_items, seg = c
    row_off, h, node, lg64, w64, b = D.case_ref(c)
    eng = engines(E, L)
    if seg != D.SEG:
        monkeypatch.setenv("DM_DFM_OTM_TREE_SEG", str(seg))
    eng.timing_reset()
    w = one_shot(eng, row_off, h, node, old_level, gap)
    assert eng.timing_get_kind(44)[0] == 1 and eng.timing_get_kind(45)[0] == 1          # EV_DFM_OTM_TREE_SCORE, _SUM: one chunk
    has = np.diff(row_off) > 0
    assert w.shape == (n_items, 1 << gap) and (w[~has] == -1e6).all()
    ratio = float((np.abs(w - w64)[has] / b[has]).max())
    WORST[0] = max(WORST[0], ratio)
    print("%s: |gpu - ref64| / bound: max %.4f (worst so far %.4f)" % (D.case_id(c), ratio, WORST[0]))
    assert ratio <= 1.0
    assert w.tobytes() == oracle(eng, row_off, h, node, gap, seg).tobytes()
    assert prepared(eng, row_off, h, node, old_level, gap).tobytes() == w.tobytes()       # both forms, the same bytes
    assert one_shot(eng, row_off, h, node, old_level, gap).tobytes() == w.tobytes()       # rerun


# --------------------------------------------------------------------------- 3. what must not matter
IDENT = [c for c in D.CASES if (c[0], c[1], c[3]) in {(16, 10, 2), (128, 15, 3), (128, 10, 4), (16, 10, 8)} and c[6] == 4]


@pytest.mark.parametrize("c", IDENT, ids=D.case_id)
def test_bytes_do_not_depend_on_slice_grid_neighbours_or_form(engines, monkeypatch, c):
    E, L, old_level, gap, rows, n_items, seg = c
    row_off, h, node, _, _, _ = D.case_ref(c)
    eng = engines(E, L)
    monkeypatch.setenv("DM_DFM_OTM_TREE_SEG", "4")
    base = one_shot(eng, row_off, h, node, old_level, gap)
    # chunks of whole items with at most 7 histories: an item larger than the slice (11 rows), chunk edges between items
    monkeypatch.setenv("DM_DFM_JTM_SLICE", "7")
    eng.timing_reset()
    assert one_shot(eng, row_off, h, node, old_level, gap).tobytes() == base.tobytes()
    if rows == D.ROWS_SMALL:
        assert eng.timing_get_kind(45)[0] > 2
    assert prepared(eng, row_off, h, node, old_level, gap).tobytes() == base.tobytes()
    monkeypatch.delenv("DM_DFM_JTM_SLICE")
    # a forced grid of two workgroups: several rounds of the unit loop
    monkeypatch.setenv("DM_DFM_OTM_TREE_GRID", "2")
    assert one_shot(eng, row_off, h, node, old_level, gap).tobytes() == base.tobytes()
    assert prepared(eng, row_off, h, node, old_level, gap).tobytes() == base.tobytes()
    monkeypatch.delenv("DM_DFM_OTM_TREE_GRID")
    # a permutation of the items, and a subset call: an item's weights depend on its own rows and node only
    perm = np.random.default_rng(3).permutation(n_items)
    cnt = np.diff(row_off)
    p_off = np.concatenate([[0], np.cumsum(cnt[perm])]).astype(np.int64)
    p_h = np.concatenate([h[row_off[i]:row_off[i + 1]] for i in perm] + [np.zeros((0, L), np.int32)])
    assert one_shot(eng, p_off, p_h, node[perm], old_level, gap).tobytes() == base[perm].tobytes()
    lo, hi = 2, n_items - 1
    s_off = (row_off[lo:hi + 1] - row_off[lo]).astype(np.int64)
    assert one_shot(eng, s_off, h[row_off[lo]:row_off[hi]], node[lo:hi], old_level, gap).tobytes() == base[lo:hi].tobytes()
    # the segment length changes bytes only for items with more rows than the segment
    monkeypatch.setenv("DM_DFM_OTM_TREE_SEG", "5")
    other = one_shot(eng, row_off, h, node, old_level, gap)
    assert other[cnt <= 4].tobytes() == base[cnt <= 4].tobytes()
    assert other.tobytes() == oracle(eng, row_off, h, node, gap, 5).tobytes()
    monkeypatch.setenv("DM_DFM_OTM_TREE_SEG", "300")       # outside 1 .. 256: the native segment
    assert one_shot(eng, row_off, h, node, old_level, gap).tobytes() == oracle(eng, row_off, h, node, gap, D.SEG).tobytes()


# --------------------------------------------------------------------------- 4. the prepared form's life
def test_prepared_lifecycle(engines):
    from dismember_amd import DismemberError, Engine
    c = D.CASES[1]
    E, L, old_level, gap, rows, n_items, seg = c
    row_off, h, node, _, _, _ = D.case_ref(c)
    eng = Engine(0)
    try:
        eng.load_weights_deepfm(J.weights(E, L), E, L, D.NI)
        want = one_shot(eng, row_off, h, node, old_level, gap)
        base = live_allocs()

        def refused():
            with pytest.raises(DismemberError) as e:
                eng.deepfm_otm_tree_weights(node, old_level, old_level + gap)
            assert e.value.code == STATE, str(e.value)
            return str(e.value)
        assert "prepare first" in refused() and live_allocs() == base
        eng.deepfm_otm_tree_prepare(row_off, h)
        assert live_allocs()[0] > base[0]
        assert eng.deepfm_otm_tree_weights(node, old_level, old_level + gap).tobytes() == want.tobytes()
        assert eng.deepfm_otm_tree_weights(node, old_level, old_level + gap).tobytes() == want.tobytes()
        with pytest.raises(DismemberError) as e:                                              # another number of items
            eng.deepfm_otm_tree_weights(node[:-1], old_level, old_level + gap)
        assert e.value.code == STATE
        mid = live_allocs()
        eng.deepfm_otm_tree_prepare(row_off, h)                                              # a second prepare replaces the first
        assert live_allocs()[0] <= mid[0]
        assert eng.deepfm_otm_tree_weights(node, old_level, old_level + gap).tobytes() == want.tobytes()
        eng.deepfm_otm_tree_release()
        assert "prepare first" in refused()
        eng.deepfm_otm_tree_release()                                                        # nothing to release: fine
        assert live_allocs() == base
        # a weight load drops it too
        eng.deepfm_otm_tree_prepare(row_off, h)
        eng.load_weights_deepfm(J.weights(E, L), E, L, D.NI)
        assert "prepare first" in refused()
        assert one_shot(eng, row_off, h, node, old_level, gap).tobytes() == want.tobytes()
        assert live_allocs() == base
        # an Adam step moves the model: the prepared per-history part is stale
        eng.deepfm_train_init(lr=1e-2)
        eng.deepfm_otm_tree_prepare(row_off, h)
        codes = D.pair_codes(row_off, node, gap)[:8]
        eng.deepfm_train_forward_backward(codes, h[:8], np.arange(8) % 2)
        assert eng.deepfm_otm_tree_weights(node, old_level, old_level + gap).tobytes() == want.tobytes()      # (a gradient alone moves nothing)
        eng.deepfm_adam_step()
        assert "model changed" in refused()
        eng.deepfm_otm_tree_prepare(row_off, h)
        moved = eng.deepfm_otm_tree_weights(node, old_level, old_level + gap)
        assert moved.tobytes() != want.tobytes() and moved.tobytes() == one_shot(eng, row_off, h, node, old_level, gap).tobytes()
        assert moved.tobytes() == oracle(eng, row_off, h, node, gap, D.SEG).tobytes()
        training = live_allocs()
        eng.deepfm_otm_tree_release()
        assert live_allocs()[0] == training[0] - 5                                           # S, aux, the segments, their offsets, the partial sums
        eng.deepfm_train_free()
    finally:
        eng.close()


# --------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_handle_usable():
    from dismember_amd import Engine
    from dismember_amd import _native as N
    lib = N.lib()
    c = D.CASES[1]
    E, L, old_level, gap, rows, n_items, seg = c
    level = old_level + gap
    row_off, h, node, _, _, _ = D.case_ref(c)
    row_off, h, node = row_off.copy(), np.ascontiguousarray(h), node.copy()
    out = np.zeros((n_items, 1 << 8), np.float64)
    eng, din = Engine(0), Engine(0)
    i64p, i32p, f64p = (lambda a: a.ctypes.data_as(N.i64p)), (lambda a: a.ctypes.data_as(N.i32p)), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))

    def shot(hh, off=row_off, hist=h, nd=node, n=n_items, L_=L, old=old_level, lv=level, mask=0, w=out):
        return lib.dm_deepfm_otm_child_weights(hh, i64p(off) if off is not None else None, i32p(hist) if hist is not None else None,
                                               i32p(nd) if nd is not None else None, n, L_, old, lv, mask, f64p(w) if w is not None else None)

    def step(hh, nd=node, n=n_items, old=old_level, lv=level, w=out):
        return lib.dm_deepfm_otm_tree_weights(hh, i32p(nd) if nd is not None else None, n, old, lv, f64p(w) if w is not None else None)

    def prep(hh, off=row_off, hist=h, n=n_items, L_=L):
        return lib.dm_deepfm_otm_tree_prepare(hh, i64p(off) if off is not None else None, i32p(hist) if hist is not None else None, n, L_)

    def msg(e=None):
        return (lib.dm_last_error((e or eng)._h) or b"").decode()
    try:
        eng.load_weights_deepfm(J.weights(E, L), E, L, D.NI)
        din.load_weights_din_synthetic(32, D.NI, 9, tree_depth=J.DEPTH, rho=0.9)
        want = one_shot(eng, row_off, h, node, old_level, gap)
        assert prep(eng._h) == 0
        assert eng.deepfm_otm_tree_weights(node, old_level, level).tobytes() == want.tobytes()      # (the partial sums' buffer exists from here on)
        base = live_allocs()

        def good():
            assert live_allocs() == base, msg()
            assert one_shot(eng, row_off, h, node, old_level, gap).tobytes() == want.tobytes()
            assert eng.deepfm_otm_tree_weights(node, old_level, level).tobytes() == want.tobytes()
            assert live_allocs() == base
        assert shot(None) == INVALID and step(None) == INVALID and prep(None) == INVALID and lib.dm_deepfm_otm_tree_release(None) == INVALID
        bad_node = node.copy(); bad_node[3] = (2 << old_level) - 1                         # the first node of the next level
        low_node = node.copy(); low_node[0] = (1 << old_level) - 2                         # the last node of the level above
        bad_h = h.copy(); bad_h[5, 2] = D.NI
        neg_h = h.copy(); neg_h[6, 0] = -2
        for name, call, code in [
                ("null row_off", lambda: shot(eng._h, off=None), INVALID), ("null item_node", lambda: shot(eng._h, nd=None), INVALID),
                ("null weights", lambda: shot(eng._h, w=None), INVALID), ("null histories", lambda: shot(eng._h, hist=None), INVALID),
                ("n_items < 0", lambda: shot(eng._h, n=-1), INVALID), ("level = old_level", lambda: shot(eng._h, lv=old_level), INVALID),
                ("level < old_level", lambda: shot(eng._h, lv=old_level - 1), INVALID), ("gap 9", lambda: shot(eng._h, old=0, lv=9, nd=np.zeros(n_items, np.int32)), INVALID),
                ("item_node past its level", lambda: shot(eng._h, nd=bad_node), INVALID), ("item_node before its level", lambda: shot(eng._h, nd=low_node), INVALID),
                ("level past the table", lambda: shot(eng._h, old=10, lv=11, nd=np.full(n_items, 1023, np.int32)), INDEX),
                ("history code = num_index", lambda: shot(eng._h, hist=bad_h), INDEX), ("history code -2", lambda: shot(eng._h, hist=neg_h), INDEX),
                ("use_mask", lambda: shot(eng._h, mask=1), INVALID), ("another L", lambda: shot(eng._h, L_=L - 1), INVALID),
                ("prepare: null row_off", lambda: prep(eng._h, off=None), INVALID), ("prepare: null histories", lambda: prep(eng._h, hist=None), INVALID),
                ("prepare: n_items < 0", lambda: prep(eng._h, n=-1), INVALID), ("prepare: another L", lambda: prep(eng._h, L_=L + 1), INVALID),
                ("prepare: history code", lambda: prep(eng._h, hist=bad_h), INDEX),
                ("weights: null item_node", lambda: step(eng._h, nd=None), INVALID), ("weights: null weights", lambda: step(eng._h, w=None), INVALID),
                ("weights: level = old_level", lambda: step(eng._h, lv=old_level), INVALID), ("weights: gap 9", lambda: step(eng._h, old=0, lv=9, nd=np.zeros(n_items, np.int32)), INVALID),
                ("weights: item_node", lambda: step(eng._h, nd=bad_node), INVALID),
                ("weights: level past the table", lambda: step(eng._h, old=10, lv=11, nd=np.full(n_items, 1023, np.int32)), INDEX)]:
            assert call() == code, (name, msg())
            good()
        # a DIN engine refuses all four entry points; dm_otm_child_weights keeps refusing a DeepFM handle
        d0 = live_allocs()
        for name, rc in (("one-shot", shot(din._h)), ("prepare", prep(din._h)), ("weights", step(din._h))):
            assert rc == STATE and "the loaded scorer is DIN" in msg(din), (name, msg(din))
        assert lib.dm_deepfm_otm_tree_release(din._h) == 0 and live_allocs() == d0
        assert lib.dm_otm_child_weights(eng._h, i64p(row_off), i32p(h), i32p(node), n_items, L, old_level, level, 0, f64p(out)) == -5
        good()
        # a clone serves the one-shot call and is refused the prepared form
        cl = eng.clone()
        try:
            assert cl.deepfm_otm_child_weights(row_off, h, node, old_level, level).tobytes() == want.tobytes()
            assert prep(cl._h) == STATE and step(cl._h) == STATE
        finally:
            cl.close()
        # no items: nothing to do
        assert shot(eng._h, n=0) == 0
        eng.deepfm_otm_tree_release()
    finally:
        eng.close(); din.close()


# --------------------------------------------------------------------------- 6. TreeConstruction
def _construction(n=300, L=10, seed=11):
    rng = np.random.default_rng(seed)
    leaf_level = int(np.ceil(np.log(n) / np.log(2)))
    leaves = rng.permutation(np.arange((1 << leaf_level) - 1, (2 << leaf_level) - 1))[:n]
    mapping = {int(i + 1): int(v) for i, v in enumerate(leaves)}
    seqs = {}
    for it in mapping:
        r = int(rng.integers(0, 6))
        if r:
            hh = rng.integers(0, (2 << leaf_level) - 1, (r, L)).astype(np.int32)
            hh[rng.random((r, L)) < 0.2] = -1
            seqs[it] = hh.ravel()
    return mapping, seqs, leaf_level


@pytest.mark.parametrize("gap", [2, 3])
def test_tree_construction_on_a_deepfm_engine(engines, gap):
    from dismember_amd.otm_tree import TreeConstruction
    mapping, seqs, leaf_level = _construction()
    eng = engines(16, 10)
    tc = TreeConstruction(eng, mapping, seqs, gap=gap, seq_len=10, use_mask=False)
    base = live_allocs()
    a = tc.run()
    assert live_allocs() == base                                                             # released in a finally
    b = tc.run(prepared=False)
    rows = tc.row_codes.reshape(-1, 10)
    c = tc.run(weight_fn=lambda node, old, lv: oracle(eng, tc.row_off, rows, node, lv - old, D.SEG))
    assert a == b == c
    nodes = np.array(sorted(a.values()))
    assert sorted(a) == sorted(mapping) and np.unique(nodes).size == len(mapping)            # one-to-one (max_assign is 1 at the leaves)
    assert nodes[0] >= (1 << leaf_level) - 1 and nodes[-1] <= (2 << leaf_level) - 2
    assert a != mapping
    with pytest.raises(ValueError, match="use_mask"):
        TreeConstruction(eng, mapping, seqs, gap=gap, seq_len=10, use_mask=True)

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="one rank"):
        TreeConstruction(eng, mapping, seqs, gap=gap, seq_len=10, use_mask=False, comm=TwoRanks())


def test_tree_construction_on_a_din_engine_is_unchanged():
    from dismember_amd import Engine
    from dismember_amd.otm_tree import TreeConstruction
    mapping, seqs, leaf_level = _construction(n=120)
    din = Engine(0)
    try:
        din.load_weights_din_synthetic(32, D.NI, 9, tree_depth=J.DEPTH, rho=0.9)
        tc = TreeConstruction(din, mapping, seqs, gap=2, seq_len=10, use_mask=True)
        assert not tc.deepfm
        a = tc.run()
        assert a == tc.run(prepared=False) == tc.run(weight_fn=tc.child_weights)             # the DIN entry point, whatever the keyword
        assert sorted(a.values()) == sorted(set(a.values())) and len(a) == len(mapping)
    finally:
        din.close()


# --------------------------------------------------------------------------- 7. the conf task
def test_conf_task_constructs_the_tree_of_a_deepfm_checkpoint(tmp_path):
    from test_tasks import _otm_conf
    from dismember_amd import Engine, OTM, tasks
    from dismember_amd import otm_data as od
    conf = _otm_conf(tmp_path, **{"model.deep_model": "DeepFM"})
    r = tasks.otm_train_deep_model(conf, time_recommend=False, max_iterations=4)
    r["engine"].close()
    old = od.load_mapping(r["params"]["mapping_path"])
    out = tasks.otm_construct_tree(conf, deepfm=True)
    try:
        new = od.load_mapping(r["params"]["mapping_path"])
        assert new == out["mapping"] and sorted(new) == sorted(old) and new != old
        nodes = np.array(sorted(new.values()))
        assert np.unique(nodes).size == len(old) and nodes[0] >= 4095 and nodes[-1] <= 8190          # a bijection onto leaves of level 12
        q = [0, 0, 2126, 204, 3257, 3439, 996, 1681, 3438, 1882]
        rec = OTM(out["engine"], new, "DeepFM").recommend(q, 10, 20)
        assert len(rec) == 10 and {i for i, _ in rec} <= set(new)
    finally:
        out["engine"].close()
    assert tasks.main(["OTMConstructTree", "--otmConfFile", conf, "--quiet"]) == 0
    again = od.load_mapping(r["params"]["mapping_path"])
    assert sorted(again) == sorted(old) and np.unique(list(again.values())).size == len(old)
