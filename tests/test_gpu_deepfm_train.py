"""The DeepFM training step on the device (csrc/dfm_train.hip.inc): loss and gradient against the float64 restatement
(tests/deepfm_train_ref.py) under |gpu - ref| <= k eps32 A with k from tests/golden/deepfm_train_tolerances.json (CPU-derived), determinism,
the Adam wiring, serving after training, the sampler's twins, refusals, a problem it learns, and the conf task."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import deepfm_ref as R
import deepfm_train_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "deepfm_train_tolerances.json")))["k"]
NI_S = (1 << (R.SEARCH_DEPTH + 1)) - 1
NEG = np.array([0, 1, 2, 3, 4, 4, 4, 4, 4, 4], np.int32)


def live_allocs():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


def padded_view(eng, what):
    """the device's own (padded) vector through the debug view, not in the public header"""
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_deepfm_train_padded
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, N.f32p, N.i64p]
    n = C.c_int64(0)
    assert fn(eng._h, what, None, C.byref(n)) == 0
    out = np.empty(n.value, np.float32)
    assert fn(eng._h, what, out.ctypes.data_as(N.f32p), C.byref(n)) == 0
    return out


def engine(E, L, w, NI=T.NUM_INDEX, tree=None):
    from dismember_amd import Engine
    eng = Engine(0)
    if tree is not None:
        eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
        eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_deepfm(w, E, L, NI)
    return eng


@functools.lru_cache(maxsize=None)
def reference(kind, key):
    """the float64 step of a case, computed once"""
    if kind == "shape":
        E, L, _ = key
        w, codes, seqs, y, _ = T.shape_case(*key)
    else:
        E, L = 16, 10
        w, codes, seqs, y, _ = T.structure_case(key)
    o = T.step(w, E, L, T.NUM_INDEX, codes, seqs, y)
    for v in (o["g"], o["A"]):
        v.setflags(write=False)
    return (w, E, L, codes, seqs, y), o


def check_step(kind, key):
    (w, E, L, codes, seqs, y), ref = reference(kind, key)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init()
        loss = eng.deepfm_train_forward_backward(codes, seqs, y)
        g = eng.deepfm_train_download("grad")
    finally:
        eng.close()
    assert np.isfinite(loss) and np.isfinite(g).all()
    ratios = T.ratios(g, ref["g"], ref["A"], E, L, T.NUM_INDEX)
    ratios["loss"] = abs(loss - ref["loss"]) / (T.EPS32 * ref["A_loss"])
    print("%s %s: share of the bound " % (kind, key) + " ".join("%s %.3f" % (t, ratios[t] / K[t]) for t in sorted(ratios)))
    for t, v in ratios.items():
        assert v <= K[t], (t, v, K[t])


# --------------------------------------------------------------------------- gradient and loss
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "E%d-L%d-B%d" % s)
def test_step_shapes(shape):
    check_step("shape", shape)


def test_step_grid_stride_second_partial_round(monkeypatch):
    monkeypatch.setenv("DM_DFM_TRAIN_GRID", "2")           # 13 tiles over 2 workgroups of 4 waves: 8 + 5
    check_step("shape", T.GRID_CASE)


@pytest.mark.parametrize("name", T.STRUCTURES)
def test_step_structures(name):
    check_step("structure", name)


# --------------------------------------------------------------------------- determinism and Adam wiring
def _run(eng, batches, steps, lr=1e-3, grad_scale=1.0, keep=False):
    eng.deepfm_train_init(lr=lr)
    out = []
    for t in range(steps):
        codes, seqs, y = batches[t % len(batches)]
        eng.deepfm_train_forward_backward(codes, seqs, y)
        g = eng.deepfm_train_download("grad")
        eng.deepfm_adam_step(grad_scale)
        out.append((g, eng.deepfm_train_download("weights"), eng.deepfm_train_download("s"), eng.deepfm_train_download("r")) if keep or t == steps - 1
                   else (g,))
    return out


def _ulps(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.float32(1e-45)).astype(np.float64)


def test_determinism_adam_rows_dense_and_scale(monkeypatch):
    E, L = 16, 10
    w, c2, s2, y2, _ = T.structure_case("item_in_own_history")
    _, c3, s3, y3, _ = T.structure_case("all_pad_history")
    batches = [(c2, s2, y2), (c3, s3, y3), (c2[:17], s2[:17], y2[:17])]
    eng = engine(E, L, w)
    try:
        a = _run(eng, batches, 3, keep=True)
        eng.load_weights_deepfm(w, E, L, T.NUM_INDEX)
        b = _run(eng, batches, 3, keep=True)
        for x, z in zip(a, b):
            for u, v in zip(x, z):
                assert u.tobytes() == v.tobytes()
        # untouched rows keep their bytes
        touched = np.zeros(T.NUM_INDEX, bool)
        for c, s, _ in batches:
            touched[c[c >= 0]] = True; touched[s[s >= 0]] = True
        w_end = a[-1][1]
        emb0, emb1 = w[:T.NUM_INDEX * E].reshape(-1, E), w_end[:T.NUM_INDEX * E].reshape(-1, E)
        assert (~touched).sum() > 500 and emb0[~touched].tobytes() == emb1[~touched].tobytes()
        assert (emb0[touched] != emb1[touched]).any(axis=1).all()
        # numpy Adam on the device's own gradients: moments within 2 ulp
        wn, sn, rn = w.copy(), np.zeros_like(w), np.zeros_like(w)
        for t, (g, wd, sd, rd) in enumerate(a, 1):
            T.adam_update(wn, g, sn, rn, t, 1e-3)
            assert _ulps(sd, sn).max() <= 2 and _ulps(rd, rn).max() <= 2
            assert np.allclose(wd, wn, rtol=1e-5, atol=1e-7)
            wn[:] = wd; sn[:] = sd; rn[:] = rd
        # dense path = rows path, byte for byte
        monkeypatch.setenv("DM_ADAM_DENSE", "1")
        eng.load_weights_deepfm(w, E, L, T.NUM_INDEX)
        d = _run(eng, batches, 3, keep=True)
        monkeypatch.delenv("DM_ADAM_DENSE")
        for x, z in zip(a, d):
            for u, v in zip(x, z):
                assert u.tobytes() == v.tobytes()
        # grad_scale
        eng.load_weights_deepfm(w, E, L, T.NUM_INDEX)
        (g, wd, sd, rd), = _run(eng, batches, 1, grad_scale=0.5, keep=True)
        wn, sn, rn = w.copy(), np.zeros_like(w), np.zeros_like(w)
        T.adam_update(wn, g, sn, rn, 1, 1e-3, grad_scale=0.5)
        assert np.abs(sn).max() > 0 and _ulps(sd, sn).max() <= 2 and _ulps(rd, rn).max() <= 2
        # a second init zeroes the state (and the time step)
        eng.deepfm_train_init(lr=1e-3)
        for what in ("grad", "s", "r"):
            assert not eng.deepfm_train_download(what).any()
        wb = eng.deepfm_train_download("weights")
        eng.deepfm_train_forward_backward(c2, s2, y2)
        g = eng.deepfm_train_download("grad")
        eng.deepfm_adam_step()
        wn, sn, rn = wb.copy(), np.zeros_like(w), np.zeros_like(w)
        T.adam_update(wn, g, sn, rn, 1, 1e-3)
        assert _ulps(eng.deepfm_train_download("s"), sn).max() <= 2 and np.allclose(eng.deepfm_train_download("weights"), wn, rtol=1e-5, atol=1e-7)
        # forward_backward replaces the gradient: a second batch leaves nothing of the first
        eng.deepfm_train_forward_backward(c2, s2, y2)
        eng.deepfm_train_forward_backward(c3, s3, y3)
        g3 = eng.deepfm_train_download("grad")
        eng.deepfm_train_init(lr=1e-3)
        eng.deepfm_train_forward_backward(c3, s3, y3)
        assert g3.tobytes() == eng.deepfm_train_download("grad").tobytes()
    finally:
        eng.close()


def test_padded_columns_stay_exact_zeros():
    E, L, Ep = 24, 1, 32
    w, codes, seqs, y, _ = T.shape_case(24, 1, 1)
    rng = np.random.default_rng(3)
    codes = rng.integers(0, T.NUM_INDEX, 300).astype(np.int32); seqs = rng.integers(-1, T.NUM_INDEX, (300, L)).astype(np.int32)
    y = (rng.random(300) < 0.4).astype(np.float32)
    eng = engine(E, L, w)
    try:
        eng.deepfm_train_init(lr=0.01)
        for _ in range(5):
            eng.deepfm_train_forward_backward(codes, seqs, y)
            gp = padded_view(eng, 1)
            eng.deepfm_adam_step()
        NI, Tt = T.NUM_INDEX, L + 1
        for what, v in ((0, padded_view(eng, 0)), (1, gp), (2, padded_view(eng, 2)), (3, padded_view(eng, 3))):
            assert v.size == NI * Ep + Tt * Tt * Ep + 2 * Tt + 1
            blocks = v[:NI * Ep + Tt * Tt * Ep].reshape(-1, Ep)
            assert not blocks[:, E:].any(), what
            assert blocks[:, :E].any(), what
        # and the unpadded download is the padded vector without those columns
        assert eng.deepfm_train_download("weights").tobytes() == np.concatenate(
            [padded_view(eng, 0)[:NI * Ep + Tt * Tt * Ep].reshape(-1, Ep)[:, :E].ravel(), padded_view(eng, 0)[NI * Ep + Tt * Tt * Ep:]]).tobytes()
    finally:
        eng.close()


# --------------------------------------------------------------------------- serving after training
def _search_dev(eng, seqs, beam, topk):
    U, L = seqs.shape
    d_seq, d_ids, d_sc, d_cnt = eng.dev_alloc(U * L * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * topk * 4), eng.dev_alloc(U * 4)
    try:
        eng.h2d(d_seq, np.ascontiguousarray(seqs, np.int32))
        eng.tdm_beam_search_dev(d_seq, U, L, beam, topk, d_ids, d_sc, d_cnt, use_mask=False)
        eng.synchronize()
        ids, sc, cnt = np.empty((U, topk), np.int32), np.empty((U, topk), np.float32), np.empty(U, np.int32)
        eng.d2h(ids, d_ids); eng.d2h(sc, d_sc); eng.d2h(cnt, d_cnt)
    finally:
        for p in (d_seq, d_ids, d_sc, d_cnt):
            eng.dev_free(p)
    return ids, sc, cnt


def _valid(ids, sc, cnt):
    m = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    return ids[m].tobytes() + sc[m].tobytes() + cnt.tobytes()


def test_serving_after_training_matches_a_fresh_load(tmp_path):
    E, L = 16, 10
    tree, w, seqs = R.search_case(E, L)
    rng = np.random.default_rng(11)
    tgt = rng.choice(tree["leaf_ids"], seqs.shape[0]).astype(np.int32)
    eng = engine(E, L, w, NI_S, tree)
    clone = eng.clone()
    fresh = None
    try:
        before = clone.tdm_beam_search(seqs, 8, 5, use_mask=False)
        eng.deepfm_train_init(lr=0.01)
        for it in range(5):
            loss = eng.deepfm_train_step_sampled(seqs, tgt, NEG, 1, seed=it)
            assert np.isfinite(loss) and loss > 0
            eng.deepfm_adam_step()
        wt = eng.deepfm_train_download("weights")
        assert wt.tobytes() != w.tobytes()
        fresh = engine(E, L, wt, NI_S, tree)
        codes, hist, _ = eng.deepfm_make_train_batch(seqs, tgt, NEG, 1, seed=99)
        assert eng.deepfm_forward(codes, hist).tobytes() == fresh.deepfm_forward(codes, hist).tobytes()
        want = fresh.tdm_beam_search(seqs, 8, 5, use_mask=False)
        assert _valid(*eng.tdm_beam_search(seqs, 8, 5, use_mask=False)) == _valid(*want)
        assert _valid(*_search_dev(eng, seqs, 8, 5)) == _valid(*want)
        after = clone.tdm_beam_search(seqs, 8, 5, use_mask=False)             # a clone made before training serves the new weights
        assert _valid(*after) == _valid(*want) and _valid(*after) != _valid(*before)
        path = str(tmp_path / "trained.bin")
        eng.save_model(path)
        fresh.load_model(path)
        assert fresh.scorer_kind() == ("deepfm", L)
        assert fresh.deepfm_train_download("weights").tobytes() == wt.tobytes()
        assert _valid(*fresh.tdm_beam_search(seqs, 8, 5, use_mask=False)) == _valid(*want)
    finally:
        clone.close()
        eng.close()
        if fresh is not None:
            fresh.close()


# --------------------------------------------------------------------------- sampler twins
def test_sampler_twins_equal_the_din_sampler_without_mask():
    from dismember_amd import DismemberError, Engine, _native as N
    E, L = 16, 10
    tree, w, seqs = R.search_case(E, L)
    rng = np.random.default_rng(12)
    tgt = rng.choice(tree["leaf_ids"], seqs.shape[0]).astype(np.int32)
    tgt[3] = 0                                                   # a padding target: no rows
    din = Engine(0)
    din.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
    din.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng = engine(E, L, w, NI_S, tree)
    try:
        codes, rseq, mask, lab = din.make_train_batch(seqs, tgt, NEG, 1, seed=5, use_mask=False)
        assert codes.size > 100 and not mask.any()
        c2, s2, l2 = eng.deepfm_make_train_batch(seqs, tgt, NEG, 1, seed=5)
        assert (c2.tobytes(), s2.tobytes(), l2.tobytes()) == (codes.tobytes(), rseq.tobytes(), lab.tobytes())
        eng.deepfm_train_init()
        loss, (c3, s3, l3) = eng.deepfm_train_step_sampled(seqs, tgt, NEG, 1, seed=5, return_rows=True)
        assert (c3.tobytes(), s3.tobytes(), l3.tobytes()) == (codes.tobytes(), rseq.tobytes(), lab.tobytes())
        ref = T.step(w, E, L, NI_S, codes, rseq, lab, loss_only=True)
        assert abs(loss - ref["loss"]) <= K["loss"] * T.EPS32 * ref["A_loss"]
        # use_mask = 1 is refused by both twins
        o = N.SampleOpts(1, 0, 20, 1, 5)
        n = C.c_int64(0)
        sq, tg = np.ascontiguousarray(seqs, np.int32), np.ascontiguousarray(tgt, np.int32)
        rc = N.lib().dm_deepfm_make_train_batch(eng._h, sq.ctypes.data_as(N.i32p), tg.ctypes.data_as(N.i32p), len(tg), L, NEG.ctypes.data_as(N.i32p),
                                                NEG.size, C.byref(o), None, None, None, 0, C.byref(n))
        assert rc == -1 and b"no mask" in N.lib().dm_last_error(eng._h)
        rc = N.lib().dm_deepfm_sample_train_batch_dev(eng._h, None, None, len(tg), L, NEG.ctypes.data_as(N.i32p), NEG.size, C.byref(o), None, None, None,
                                                      0, C.byref(n))
        assert rc == -1 and b"no mask" in N.lib().dm_last_error(eng._h)
        # the DIN entry points keep refusing a DeepFM model, and the twins a DIN handle
        with pytest.raises(DismemberError) as e:
            eng.make_train_batch(seqs, tgt, NEG, 1, seed=5, use_mask=False)
        assert e.value.code == -5 and "DeepFM" in str(e.value)
        with pytest.raises(DismemberError) as e:
            din.deepfm_make_train_batch(seqs, tgt, NEG, 1, seed=5)
        assert e.value.code == -3
    finally:
        din.close()
        eng.close()


# --------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_usable_and_memory_returns():
    from dismember_amd import DismemberError, Engine, _native as N
    import helpers
    E, L = 16, 10
    (w, _, _, codes, seqs, y), ref = reference("structure", "item_in_own_history")

    def refused(code, fn, *a, **k):
        with pytest.raises(DismemberError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))

    eng = Engine(0)
    try:
        # no model; a DIN model
        refused(-3, eng.deepfm_train_init)
        refused(-3, eng.deepfm_train_param_count)
        eng.load_weights_din(helpers.random_din_weights(np.random.default_rng(1), E, T.NUM_INDEX), E, T.NUM_INDEX)
        for fn, a in ((eng.deepfm_train_init, ()), (eng.deepfm_train_forward_backward, (codes, seqs, y)), (eng.deepfm_adam_step, ()),
                      (eng.deepfm_train_param_count, ()), (eng.deepfm_train_download, ())):
            refused(-3, fn, *a)
        eng.deepfm_train_free()                                  # nothing to free: fine
        eng.load_weights_deepfm(w, E, L, T.NUM_INDEX)
        # before the init
        refused(-3, eng.deepfm_train_forward_backward, codes, seqs, y)
        refused(-3, eng.deepfm_adam_step)
        refused(-3, eng.deepfm_train_download, "grad")
        assert eng.deepfm_train_download("weights").tobytes() == w.tobytes() and eng.deepfm_train_param_count() == w.size
        base = live_allocs()
        refused(-1, eng.deepfm_train_init, lr=0.0)
        assert live_allocs() == base
        eng.deepfm_train_init()
        assert live_allocs()[0] > base[0]
        # on a clone
        cl = eng.clone()
        try:
            for fn, a in ((cl.deepfm_train_init, ()), (cl.deepfm_train_free, ()), (cl.deepfm_train_forward_backward, (codes, seqs, y)),
                          (cl.deepfm_adam_step, ()), (cl.deepfm_train_param_count, ()), (cl.deepfm_train_download, ())):
                refused(-3, fn, *a)
        finally:
            cl.close()
        # arguments
        refused(-1, eng.deepfm_train_forward_backward, codes, seqs[:, :9], y)          # L != the model's
        refused(-1, eng.deepfm_train_forward_backward, codes[:0], seqs[:0], y[:0])     # B = 0
        lib = N.lib()
        loss = C.c_double(0)
        assert lib.dm_deepfm_train_forward_backward(eng._h, None, seqs.ctypes.data_as(N.i32p), y.ctypes.data_as(N.f32p), len(y), L, C.byref(loss)) == -1
        assert lib.dm_deepfm_train_forward_backward_dev(eng._h, None, None, None, 5, L, C.byref(loss)) == -1
        out = np.empty(w.size, np.float32)
        assert lib.dm_deepfm_train_download(eng._h, 0, out.ctypes.data_as(N.f32p), w.size - 1) == -1
        assert lib.dm_deepfm_train_download(eng._h, 4, out.ctypes.data_as(N.f32p), w.size) == -1
        bad = codes.copy(); bad[7] = T.NUM_INDEX
        refused(-4, eng.deepfm_train_forward_backward, bad, seqs, y)
        bad = seqs.copy(); bad[3, 2] = -2
        refused(-4, eng.deepfm_train_forward_backward, codes, bad, y)
        # too large: refused before anything is read (the arrays are not touched)
        big = (1 << 31) // (L + 1) + 1
        assert lib.dm_deepfm_train_forward_backward_dev(eng._h, C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), big, L, C.byref(loss)) == -5
        assert lib.dm_deepfm_train_forward_backward_dev(eng._h, C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), 65535 * 64 + 1, L, C.byref(loss)) == -5
        # ... and the handle still trains
        got = eng.deepfm_train_forward_backward(codes, seqs, y)
        assert abs(got - ref["loss"]) <= K["loss"] * T.EPS32 * ref["A_loss"]
        eng.deepfm_adam_step()
        eng.deepfm_train_free()
        assert live_allocs() == base
        eng.deepfm_train_free()
        refused(-3, eng.deepfm_adam_step)
        z = eng.deepfm_forward(codes, seqs)                    # the model keeps serving
        assert np.isfinite(z).all()
        # a later load drops the training state
        base = live_allocs()                                   # (the forward's request buffer stays with the handle)
        eng.deepfm_train_init()
        eng.deepfm_train_forward_backward(codes, seqs, y)
        eng.load_weights_deepfm(w, E, L, T.NUM_INDEX)
        assert live_allocs() == base
        refused(-3, eng.deepfm_adam_step)
        eng.deepfm_train_init()
        eng.load_weights_din(helpers.random_din_weights(np.random.default_rng(1), E, T.NUM_INDEX), E, T.NUM_INDEX)
        refused(-3, eng.deepfm_adam_step)
    finally:
        eng.close()


# --------------------------------------------------------------------------- a problem it learns, and the task
def test_learns_the_teacher():
    w0, batches, NI = T.learning_case()
    eng = engine(T.LEARN["E"], T.LEARN["L"], w0, NI)
    try:
        eng.deepfm_train_init(lr=T.LEARN["lr"])
        losses = []
        for _ in range(T.LEARN["steps"]):
            losses.append(eng.deepfm_train_forward_backward(*batches[0]))
            eng.deepfm_adam_step()
    finally:
        eng.close()
    assert min(losses) <= 0.8 * losses[0], losses


def test_tdm_train_deep_model_task_with_deepfm(tmp_path):
    from dismember_amd import Engine, TDM, tasks
    from test_tasks import _conf
    conf = _conf(tmp_path, **{"model.iteration_number": 60, "model.show_progress_interval": 30, "model.deep_model": "DeepFM"})
    tasks.tdm_initialize_tree(conf)
    r = tasks.tdm_train_deep_model(conf, time_recommend=False)
    losses = r["losses"]
    assert len(losses) == 60 and np.mean(losses[-10:]) < np.mean(losses[:10])
    assert [it for it, _ in r["eval"]] == [30, 60] and np.isfinite(r["eval"][-1][1]["loss"])
    eng = r["engine"]
    L = r["params"]["seq_len"]
    assert eng.scorer_kind() == ("deepfm", L)
    e2 = Engine(0)
    try:
        tdm = TDM.load_model(e2, r["params"]["model_path"])
        assert e2.scorer_kind() == ("deepfm", L)
        q = np.array([0, 0, 2126, 204, 3257, 3439, 996, 1681, 3438, 1882], np.int32)
        rec = tdm.recommend(q, 10, 20)
        assert len(rec) > 0 and rec == TDM(eng, "DeepFM").recommend(q, 10, 20)
    finally:
        e2.close()
        eng.close()
