"""GPU tests of the resident Deep-Retrieval mapping and training set (dm_dr_set_item_paths, dm_dr_train_set_*).  Every
comparison is an integer or a byte equality: the CSR against the host inversion behind dm_dr_load_path_items, the shuffle against the
restatement on Python integers (tests/dr_resident_ref.py), the resident steps against the host-batch entry points fed the same samples,
the resident M-step against dm_dr_mstep_optimize."""
import ctypes as C
import functools
import multiprocessing as mp
import socket
import traceback

import numpy as np
import pytest

import dr_resident_ref as RR
from dismember_amd import DismemberError, synth
from dismember_amd.dr_train import DRTrainer, expand_batch

pytestmark = pytest.mark.gpu
OK, INVALID, STATE, INDEX, UNSUPPORTED = 0, -1, -3, -4, -5
DTYPES = {"f32": np.float32, "f64": np.float64}
E, L = 16, 4


def live():
    from dismember_amd import _native as N
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return c.value, b.value


def bare_engine(ni, K, D, dtype=np.float32):
    """a model whose weights nobody reads (generated on the device, no rerank arrays): the mapping alone is under test"""
    from dismember_amd import Engine
    eng = Engine(0)
    eng.dr_load_model_synthetic(E, L, K, D, ni, seed=1, rerank=False, dtype=dtype)
    return eng


@functools.lru_cache(maxsize=None)
def problem(D=2, K=16, ni=64, N=70, J=2):
    """the small model of tests/dr_train_ref.py with its rerank arrays, a mapping and a training set; sample 3 is all padding"""
    rng = np.random.default_rng(100 * D + K)
    w = synth.make_dr_model(ni, K, D, L, E, rng)
    item_paths = rng.integers(0, K, size=(ni, J, D), dtype=np.int32)
    seqs = rng.integers(0, ni, size=(N, L), dtype=np.int32)
    seqs[rng.random((N, L)) < 0.2] = -1
    seqs[3] = -1
    targets = rng.integers(0, ni, N).astype(np.int32)
    for a in (item_paths, seqs, targets):
        a.setflags(write=False)
    return dict(w=w, dims=(E, L, K, D, ni), item_paths=item_paths, seqs=seqs, targets=targets, N=N, J=J)


def model_engine(p, dt, train=True, rerank=False):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.dr_load_model(p["w"], *p["dims"], dtype=DTYPES[dt])
    if train:
        eng.dr_train_init(lr=1e-2)
    if rerank:
        eng.dr_rerank_train_init(8, seed=5, lr=1e-2)
    return eng


def err(fn, *a, **kw):
    with pytest.raises(DismemberError) as e:
        fn(*a, **kw)
    return e.value.code


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)) and len(a) == len(b)


# ------------------------------------------------------------------------------------------------------------------------ mapping
def check_mapping(eng, p, K, ref):
    eng.dr_load_path_items(*ref)
    want = eng.dr_path_items_download()
    eng.dr_set_item_paths(p)
    got = eng.dr_path_items_download()
    assert same(got, want)
    assert np.array_equal(eng.dr_item_paths_download(), p)
    return got


@pytest.mark.parametrize("name", sorted(RR.MAPPING_CASES))
def test_csr_equals_the_host_inversion(name):
    p, K, D = RR.mapping_case(name)
    eng = bare_engine(p.shape[0], K, D)
    got = check_mapping(eng, p, K, synth.dr_path_items(p))
    eng.close()
    assert same(got, RR.csr(p, K))
    kind = RR.MAPPING_CASES[name][4]
    if kind == "one-path":
        assert len(got[0]) == 1 and np.array_equal(got[2], np.arange(p.shape[0]))
    if kind == "distinct":
        assert len(got[0]) == p.shape[0] * p.shape[1]
    if kind == "twice":
        assert len(got[2]) == p.shape[0] * p.shape[1] - 3
    if name == "wide-codes":
        assert got[0].max() >= 1 << 32


@pytest.mark.parametrize("m", RR.BIG_MAPPING_SIZES)
def test_csr_at_the_chunk_edges_of_sort_and_compaction(m):
    p, K, D = RR.big_mapping_case(m)
    eng = bare_engine(m, K, D)
    got = check_mapping(eng, p, K, synth.dr_path_items_fast(p, K))
    eng.close()
    assert len(got[2]) == m and got[1][-1] == m and (np.diff(got[0]) > 0).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_recommend_after_either_loader(dt):
    p = problem()
    eng = model_engine(p, dt, train=False)
    one = np.ascontiguousarray(np.broadcast_to(np.array([3, 11], np.int32), p["item_paths"].shape))      # max_bucket = num_item
    for paths in (p["item_paths"], one):
        eng.dr_load_path_items(*synth.dr_path_items(paths))
        want = eng.dr_recommend(p["seqs"], 8, 10)
        eng.dr_set_item_paths(paths)
        got = eng.dr_recommend(p["seqs"], 8, 10)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and got[2].sum() > 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ shuffle
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_shuffle_is_the_restated_order(n):
    p = problem()
    eng = model_engine(p, "f32", train=False)
    rng = np.random.default_rng(n)
    eng.dr_train_set_load(rng.integers(-1, 64, size=(n, L)), rng.integers(0, 64, n))
    assert np.array_equal(eng.dr_train_set_order(), np.arange(n))
    for seed in RR.SHUFFLE_SEEDS:
        for epoch in RR.SHUFFLE_EPOCHS:
            eng.dr_train_set_shuffle(seed, epoch)
            assert np.array_equal(eng.dr_train_set_order(), RR.shuffle_order(seed, epoch, n)), (seed, epoch)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ steps
RANGES = ((0, 9), (65, 5), (17, 1), (0, 70))      # both ends of the set, one sample, all of it (with the all-padding history)


def resident_pair(p, dt, rerank=False):
    a, b = model_engine(p, dt, rerank=rerank), model_engine(p, dt, rerank=rerank)
    a.dr_set_item_paths(p["item_paths"])
    a.dr_train_set_load(p["seqs"], p["targets"])
    a.dr_train_set_shuffle(11, 1)
    order = a.dr_train_set_order()
    assert not np.array_equal(order, np.arange(p["N"]))
    return a, b, order


@pytest.mark.parametrize("D,K", [(2, 16), (3, 7)])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_layer_step_equals_the_host_batch_step(dt, D, K):
    p = problem(D, K)
    a, b, order = resident_pair(p, dt)
    for grouped in (True, False):
        for off, n in RANGES:
            idx = order[off:off + n]
            la = a.dr_train_set_forward_backward(off, n, grouped=grouped)
            if grouped:
                lb = b.dr_train_forward_backward_grouped(p["seqs"][idx], p["item_paths"][p["targets"][idx]])
            else:
                lb = b.dr_train_forward_backward(*expand_batch(p["seqs"][idx], p["targets"][idx], p["item_paths"]))
            ga, gb = a.dr_train_download("grad"), b.dr_train_download("grad")
            assert ga.tobytes() == gb.tobytes() and la.tobytes() == lb.tobytes() and ga.any(), (grouped, off, n)
    a.close(); b.close()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rerank_step_equals_the_host_batch_step_with_the_sampled_negatives(dt):
    p = problem()
    a, b, order = resident_pair(p, dt, rerank=True)
    for step, (off, n) in enumerate(RANGES):
        idx = order[off:off + n]
        la = a.dr_train_set_rerank_forward_backward(off, n)
        neg = b.dr_rerank_sample(p["targets"][idx], step)
        lb = b.dr_rerank_forward_backward(p["seqs"][idx], p["targets"][idx], neg)
        assert la == lb and np.isfinite(la)
        for vec in ("graph", "softmax"):
            assert a.dr_rerank_download(vec, "grad").tobytes() == b.dr_rerank_download(vec, "grad").tobytes(), (vec, off, n)
    a.close(); b.close()


def trainer_state(eng):
    return (eng.dr_train_download("weights"),) + tuple(eng.dr_rerank_download(v, "weights") for v in ("graph", "softmax"))


@pytest.mark.parametrize("grouped", [False, True])
def test_five_resident_steps_equal_five_trainer_steps(grouped):
    p = problem()
    a, b = model_engine(p, "f64", train=False), model_engine(p, "f64", train=False)
    kw = dict(lr=1e-2, rerank=True, num_sampled=8, seed=1, grouped=grouped)
    ta, tb = DRTrainer(a, p["item_paths"], resident=True, **kw), DRTrainer(b, p["item_paths"], **kw)
    w0 = trainer_state(a)
    ta.load_set(p["seqs"], p["targets"])
    ta.shuffle(3)
    order = a.dr_train_set_order()
    assert np.array_equal(order, RR.shuffle_order(3, 1, p["N"]))
    for k in range(5):
        idx = order[k * 14:(k + 1) * 14]
        la, lb = ta.step_range(k * 14, 14), tb.step(p["seqs"][idx], p["targets"][idx])
        assert np.array_equal(la[0], lb[0]) and la[1] == lb[1]
    sa, sb = trainer_state(a), trainer_state(b)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(sa, sb)) and all(x.tobytes() != y.tobytes() for x, y in zip(sa, w0))
    # the trained handle serves from the CSR the device built: evaluate_dr needs no host inversion
    b.dr_load_path_items(*synth.dr_path_items(p["item_paths"]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.dr_recommend(p["seqs"], 8, 5), b.dr_recommend(p["seqs"], 8, 5)))
    with pytest.raises(ValueError):
        tb.step_range(0, 4)
    a.close(); b.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_main(rank, world, port, q):
    try:
        from dismember_amd.comm import Comm
        comm = Comm(world, rank, "127.0.0.1", port, transport="host")
        p = problem()
        out = {}
        order = RR.shuffle_order(3, 1, p["N"])
        for name in ("resident", "host"):
            eng = model_engine(p, "f64", train=False)
            tr = DRTrainer(eng, p["item_paths"], lr=1e-2, comm=comm, resident=name == "resident")
            if name == "resident":
                tr.load_set(p["seqs"], p["targets"])
                tr.shuffle(3)
                losses = [tr.step_range(k * 13, 13) for k in range(3)]
            else:
                losses = [tr.step(p["seqs"][order[k * 13:(k + 1) * 13]], p["targets"][order[k * 13:(k + 1) * 13]]) for k in range(3)]
            out[name] = (eng.dr_train_download("weights"), np.array(losses))
            eng.attach_comm(None)
            eng.close()
        q.put((rank, "ok", out))
        comm.barrier()
        comm.close()
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
        raise


def test_two_ranks_stay_identical_to_each_other_and_to_the_host_batch_trainer():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    try:
        [pr.start() for pr in procs]
        out = {}
        for _ in range(2):
            rank, status, res = q.get(timeout=120)
            assert status == "ok", "rank %d failed:\n%s" % (rank, res)
            out[rank] = res
        [pr.join(30) for pr in procs]
        assert all(pr.exitcode == 0 for pr in procs)
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.terminate()
                pr.join(5)
    w0 = out[0]["resident"][0]
    for r in (0, 1):
        for name in ("resident", "host"):
            w, losses = out[r][name]
            assert w.tobytes() == w0.tobytes() and np.array_equal(losses, out[0]["resident"][1]), (r, name)


# ------------------------------------------------------------------------------------------------------------------------ M-step
@pytest.mark.parametrize("mode", ["batch", "streaming"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mstep_equals_optimize_on_the_same_arrays(dt, mode):
    p = problem()
    E_, L_, K, D, ni = p["dims"]
    a, b = model_engine(p, dt, train=False), model_engine(p, dt, train=False)
    a.dr_set_item_paths(p["item_paths"])
    a.dr_train_set_load(p["seqs"], p["targets"])
    kw = dict(num_iteration=3, train_mode=mode, decay_factor=0.9, seed=9)
    want = b.dr_mstep_optimize(p["seqs"], p["targets"], 6, p["J"], **kw)
    for shuffled in (False, True):
        if shuffled:
            a.dr_set_item_paths(p["item_paths"])
            a.dr_train_set_shuffle(5, 2)          # storage order: the shuffle changes nothing
        got = a.dr_train_set_mstep(6, **kw)
        assert np.array_equal(got, want) and got.dtype == want.dtype
        table = a.dr_item_paths_download()
        assert np.array_equal(table, RR.decode(want, K, D))
        b.dr_load_path_items(*synth.dr_path_items(table))
        assert same(a.dr_path_items_download(), b.dr_path_items_download())
    assert not np.array_equal(RR.decode(want, K, D), p["item_paths"])
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable_and_allocate_nothing():
    from dismember_amd import Engine, _native as N
    p = problem()
    E_, L_, K, D, ni = p["dims"]
    lib = N.lib()
    fresh = Engine(0)
    assert err(fresh.dr_set_item_paths.__func__, _Dims(fresh, p), p["item_paths"]) == STATE      # no model
    fresh.close()
    eng = model_engine(p, "f32", train=False)
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(N.i32p)
    base = live()
    # ---- mapping
    assert err(eng.dr_path_items_download) == STATE and err(eng.dr_item_paths_download) == STATE
    bad = p["item_paths"].copy(); bad[7, 1, 0] = K
    assert err(eng.dr_set_item_paths, bad) == INDEX
    bad[7, 1, 0] = -1
    assert err(eng.dr_set_item_paths, bad) == INDEX
    assert lib.dm_dr_set_item_paths(eng._h, i32(p["item_paths"]), 0) == INVALID
    assert lib.dm_dr_set_item_paths(eng._h, None, 2) == INVALID
    assert lib.dm_dr_set_item_paths(eng._h, i32(p["item_paths"]), (1 << 31) // ni) == UNSUPPORTED
    # ---- training set
    assert err(eng.dr_train_set_shuffle, 1, 1) == STATE and err(eng.dr_train_set_order) == STATE
    assert err(eng.dr_train_set_forward_backward, 0, 4) == STATE and err(eng.dr_train_set_rerank_forward_backward, 0, 4) == STATE
    assert err(eng.dr_train_set_mstep, 6) == STATE
    seqs = p["seqs"].copy(); seqs[5, 1] = ni
    assert err(eng.dr_train_set_load, seqs, p["targets"]) == INDEX
    seqs[5, 1] = -2
    assert err(eng.dr_train_set_load, seqs, p["targets"]) == INDEX
    tg = p["targets"].copy(); tg[2] = ni
    assert err(eng.dr_train_set_load, p["seqs"], tg) == INDEX
    tg[2] = -1
    assert err(eng.dr_train_set_load, p["seqs"], tg) == INDEX
    assert lib.dm_dr_train_set_load(eng._h, i32(p["seqs"]), i32(p["targets"]), 0) == INVALID
    assert lib.dm_dr_train_set_load(eng._h, i32(p["seqs"]), i32(p["targets"]), 1 << 31) == UNSUPPORTED
    assert live() == base                                           # nothing of all that allocated
    clone = eng.clone()
    assert err(clone.dr_set_item_paths.__func__, _Dims(clone, p), p["item_paths"]) == STATE
    assert lib.dm_dr_train_set_free(clone._h) == STATE
    clone.close()
    # ---- a good call after the refusals; a set without a mapping, a mapping without training state
    eng.dr_train_set_load(p["seqs"], p["targets"])
    assert err(eng.dr_train_set_forward_backward, 0, 4) == STATE and err(eng.dr_train_set_mstep, 6) == STATE      # no mapping
    eng.dr_set_item_paths(p["item_paths"])
    assert err(eng.dr_train_set_forward_backward, 0, 4) == STATE                                                    # no dr_train_init
    assert err(eng.dr_train_set_rerank_forward_backward, 0, 4) == STATE
    eng.dr_train_init(lr=1e-2)
    eng.dr_rerank_train_init(8, seed=5, lr=1e-2)
    for off, n in ((0, 0), (-1, 4), (p["N"], 1), (p["N"] - 3, 4), (0, p["N"] + 1), (0, -2)):
        assert err(eng.dr_train_set_forward_backward, off, n) == INVALID, (off, n)
        assert err(eng.dr_train_set_rerank_forward_backward, off, n) == INVALID, (off, n)
    assert err(eng.dr_train_set_mstep, 0) == INVALID and err(eng.dr_train_set_mstep, 6, num_iteration=0) == INVALID
    assert err(eng.dr_train_set_mstep, 6, train_mode="streaming", decay_factor=1.5) == INVALID
    assert lib.dm_dr_train_set_mstep(eng._h, 6, 2, 0.9, 3, 3e-6, 4, 0, None) == INVALID
    assert eng.dr_train_set_size() == (p["N"], p["J"])
    assert np.isfinite(eng.dr_train_set_forward_backward(p["N"] - 3, 3)).all() and np.isfinite(eng.dr_train_set_rerank_forward_backward(0, p["N"]))
    assert eng.dr_train_set_mstep(6).shape == (ni, p["J"])
    # ---- the set comes and goes without a trace; loading a model drops set and mapping
    eng.dr_train_set_free()
    mark = live()
    eng.dr_train_set_load(p["seqs"], p["targets"])
    assert live()[0] == mark[0] + 3
    eng.dr_train_set_free()
    assert live() == mark
    assert err(eng.dr_train_set_order) == STATE
    eng.dr_train_set_load(p["seqs"], p["targets"])
    eng.dr_load_model(p["w"], *p["dims"], dtype=np.float32)
    assert err(eng.dr_train_set_order) == STATE and err(eng.dr_item_paths_download) == STATE and err(eng.dr_path_items_download) == STATE
    eng.dr_set_item_paths(p["item_paths"])
    assert same(eng.dr_path_items_download(), RR.csr(p["item_paths"], K))
    eng.close()


def test_row_limits_and_the_code_space_are_refused_before_anything_is_allocated():
    """The limits of the steps underneath, reached through the table's J (64 items x 70 000 paths: 60 samples are 4 200 000 rows, over
    the 4 194 240 of one step), the device sampler's 2 num_sampled <= num_item, and K^D: dm_dr_load_model already stops at 4e18, below
    the 2^62 dm_dr_set_item_paths would refuse, so that refusal cannot be reached through a loaded model and the load's is the one
    checked."""
    from dismember_amd import Engine
    p = problem()
    E_, L_, K, D, ni = p["dims"]
    eng = model_engine(p, "f32", rerank=False)
    eng.dr_rerank_train_init(40, seed=5, lr=1e-2)                   # 2 x 40 > 64 items
    eng.dr_train_set_load(p["seqs"], p["targets"])
    wide = np.random.default_rng(3).integers(0, K, size=(ni, 70000, D), dtype=np.int32)
    eng.dr_set_item_paths(wide)
    assert eng.dr_train_set_size() == (p["N"], 70000)
    mark = live()
    for grouped in (True, False):
        assert err(eng.dr_train_set_forward_backward, 0, 60, grouped=grouped) == UNSUPPORTED
    assert err(eng.dr_train_set_rerank_forward_backward, 0, 8) == UNSUPPORTED
    assert live() == mark
    assert np.isfinite(eng.dr_train_set_forward_backward(0, 59, grouped=True)).all()          # 4 130 000 rows: a good call after the refusals
    eng.dr_rerank_train_init(8, seed=5, lr=1e-2)
    assert np.isfinite(eng.dr_train_set_rerank_forward_backward(0, 8))
    eng.close()
    big = Engine(0)
    d = big.dev_alloc(256)                                          # (the sizes are refused before any array is read: one block stands in for all)
    ptrs = dict(layer_emb=d, layer_w=[d] * 4, layer_b=[d] * 4)
    assert err(big.dr_load_model_dev, ptrs, E, L, 65536, 4, 8) == UNSUPPORTED      # K^D = 2^64
    big.dev_free(d)
    big.close()


def test_trainer_mstep_on_the_resident_set_checks_its_arguments():
    p = problem()
    a, b = model_engine(p, "f64", train=False), model_engine(p, "f64", train=False)
    tr = DRTrainer(a, p["item_paths"], lr=1e-2, resident=True)
    tr.load_set(p["seqs"], p["targets"])
    with pytest.raises(ValueError):
        tr.mstep(p["seqs"], p["targets"], 6)
    with pytest.raises(ValueError):
        tr.mstep(None, None, 6, path_scores="device")
    got = tr.mstep(None, None, 6, num_iteration=3, seed=9)
    want = RR.decode(b.dr_mstep_optimize(p["seqs"], p["targets"], 6, p["J"], num_iteration=3, seed=9), p["dims"][2], p["dims"][3])
    assert np.array_equal(got, want) and np.array_equal(a.dr_item_paths_download(), want) and tr.item_paths is got
    a.close(); b.close()


class _Dims:
    """an engine that never loaded a model has no dr_dims: the binding's shape check needs them to reach the library's refusal"""

    def __init__(self, eng, p):
        self._h, self._chk = eng._h, eng._chk
        E_, L_, K, D, ni = p["dims"]
        self.dr_dims = dict(E=E_, L=L_, K=K, D=D, num_item=ni)
