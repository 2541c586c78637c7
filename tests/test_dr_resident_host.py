"""CPU tests of the resident Deep-Retrieval pipeline's host side: the restatements the GPU tests compare against, the
data set (dismember_amd/dr_data.py), the files (dismember_amd/dr_io.py) and the declarations of the new entry points."""
import importlib.util
import os
import re

import numpy as np
import pytest

import dr_resident_ref as RR
from dismember_amd import _native as N
from dismember_amd import dr_data, dr_io, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRY_POINTS = {"dm_dr_set_item_paths": 3, "dm_dr_path_items_size": 3, "dm_dr_path_items_download": 4, "dm_dr_item_paths_download": 3,
                "dm_dr_train_set_load": 4, "dm_dr_train_set_free": 1, "dm_dr_train_set_size": 3, "dm_dr_train_set_shuffle": 3, "dm_dr_train_set_order_download": 2,
                "dm_dr_train_set_forward_backward": 5, "dm_dr_train_set_rerank_forward_backward": 4, "dm_dr_train_set_mstep": 9}


# ------------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_shuffle_is_a_permutation(n):
    orders = [RR.shuffle_order(s, e, n) for s in RR.SHUFFLE_SEEDS for e in RR.SHUFFLE_EPOCHS]
    for o in orders:
        assert o.dtype == np.int32 and sorted(o.tolist()) == list(range(n))
    if n >= 65:                                  # seed and epoch both matter
        assert len({o.tobytes() for o in orders}) == len(orders)


@pytest.mark.parametrize("name", sorted(RR.MAPPING_CASES))
def test_csr_restatement_equals_both_host_inversions(name):
    p, K, D = RR.mapping_case(name)
    codes, off, items = RR.csr(p, K)
    for paths, off2, items2 in (synth.dr_path_items(p), synth.dr_path_items_fast(p, K)):
        assert np.array_equal(RR.encode(paths, K), codes) and np.array_equal(off2, off) and np.array_equal(items2, items)
    assert np.array_equal(RR.decode(codes, K, D), synth.dr_path_items(p)[0]) and (np.diff(codes) > 0).all()


def test_mapping_cases_are_what_their_names_say():
    sizes = {n: RR.MAPPING_CASES[n][0] * RR.MAPPING_CASES[n][1] for n in RR.MAPPING_CASES}
    assert (sizes["m4095"], sizes["m4096"], sizes["m4097"]) == (4095, 4096, 4097)
    assert sorted({RR.MAPPING_CASES[n][1] for n in RR.MAPPING_CASES}) == [1, 2, 3]
    p, K, D = RR.mapping_case("twice")
    assert (p[5, 2] == p[5, 0]).all() and (p[9, 1] == p[9, 0]).all() and (p[9, 2] == p[9, 0]).all()
    p, K, D = RR.mapping_case("distinct")
    assert len(np.unique(RR.encode(p, K))) == p.shape[0] * p.shape[1]
    p, K, D = RR.mapping_case("wide-codes")
    assert K ** D > 1 << 32 and RR.encode(p, K).max() > 1 << 32
    import sort_ref
    assert list(RR.BIG_MAPPING_SIZES) == sort_ref.SORT_BIG_SIZES + sort_ref.SELECT_BIG_SIZES


# ------------------------------------------------------------------------------------------------------------------ the data set
def _sample(rows):
    """rows: (user, item, timestamp)"""
    return dict(user=[r[0] for r in rows], item=[r[1] for r in rows], timestamp=[r[2] for r in rows])


def test_data_set_branches_split_labels_and_ties():
    rows = []
    rows += [(7, 100 + i, i) for i in range(2)]                      # user 7: n = 2 <= min_seq_len: consumed only
    rows += [(5, 200 + i, 10 - i) for i in range(3)]                 # user 5: n = 3 == min_seq_len + 1, timestamps descending
    rows += [(3, 300 + i, i) for i in range(6)] + [(3, 302, 9)]      # user 3: 6 distinct items (302 seen again later: first kept)
    # user 9: equal timestamps keep the file order; item 300 comes first by its timestamp and its later repeat is dropped
    rows += [(9, 400, 1), (9, 401, 1), (9, 402, 1), (9, 300, 0), (9, 403, 2), (9, 300, 5)]
    s = _sample(rows)
    m = dr_data.first_appearance_mapping(s)
    assert [m[k] for k in (100, 101, 200, 201, 202, 300, 305, 400, 403)] == [0, 1, 2, 3, 4, 5, 10, 11, 14] and len(m) == 15
    L, mn = 4, 2
    consumed, train, evals = dr_data.generate_data(s, m, L, mn, 0.6)
    assert list(consumed) == [3, 5, 7, 9]                              # users ascending
    assert consumed[7] == [m[100], m[101]]
    assert consumed[5] == [m[202], m[201], m[200]]                    # sorted by timestamp
    t5 = [t for t in train if t[1] == m[200]]
    assert t5 == [([-1, -1, m[202], m[201]], m[200])]
    # user 3: n = 6, splitPoint = ceil(4 * 0.6) = ceil(2.4) = 3: windows over the first 3 + 4 padded positions, 3 samples
    i3 = [m[300 + i] for i in range(6)]
    full = [-1, -1] + i3
    t3 = [t for t in train if t[1] in i3 and t[0][-1] in i3 + [-1] and t[0] != [-1, -1, m[202], m[201]] and set(t[0]) <= set(full)]
    assert t3 == [(full[a:a + 4], full[a + 4]) for a in range(3)]
    assert consumed[3] == i3[:5]
    e3 = [e for e in evals if e[2] == 3]
    assert e3 == [(full[3:7], [i3[5]], 3)]
    # user 9: items by (timestamp, file order) = 300, 400, 401, 402, 403 (the second 300 dropped): n = 5, splitPoint = ceil(1.8) = 2
    i9 = [m[300], m[400], m[401], m[402], m[403]]
    assert consumed[9] == i9[:4]
    f9 = [-1, -1] + i9
    assert [e for e in evals if e[2] == 9] == [(f9[2:6], [i9[4]], 9)]
    assert len(train) == 1 + 3 + 2 and len(evals) == 2


def test_data_set_label_consumed_and_vanishing_eval_sample():
    # min_seq_len 1, seq_len 2: user 1 has items a b c d with split 0.5: splitPoint = ceil(3 * 0.5) = 2, consumed = a b c, labels = d
    # user 2's tail repeats nothing (distinct), so make the label vanish through the mapping: two original ids sharing one internal id
    rows = [(1, 10, 0), (1, 11, 1), (1, 12, 2), (1, 13, 3), (2, 20, 0), (2, 21, 1), (2, 22, 2), (2, 23, 3), (2, 24, 4)]
    s = _sample(rows)
    m = dr_data.first_appearance_mapping(s)
    m[24] = m[20]; m[23] = m[21]                                      # user 2's labels are items its training part consumed
    consumed, train, evals = dr_data.generate_data(s, m, 2, 1, 0.5)
    assert [e[2] for e in evals] == [1] and evals[0][1] == [m[13]] and evals[0][0] == [m[11], m[12]]
    assert consumed[2] == [m[20], m[21], m[22]] and consumed[1] == [m[10], m[11], m[12]]
    m[23] = 99                                                        # one label left: consumed ones are removed, the other stays
    _, _, evals = dr_data.generate_data(s, m, 2, 1, 0.5)
    assert [e for e in evals if e[2] == 2] == [([m[21], m[22]], [99], 2)]
    with pytest.raises(ValueError):
        dr_data.generate_data(s, m, 1, 2, 0.5)


def test_data_set_object_and_batch_size(tmp_path):
    rows = [(u, 100 * u + i, i) for u in range(1, 6) for i in range(3 + u)]
    ds = dr_data.DRDataSet(_sample(rows), 3, 7, 2, 9, 5, 4, 2, 0.8, rng=np.random.default_rng(1))
    assert ds.num_item == len(rows) and ds.item_paths.shape == (ds.num_item, 2, 3) and ds.item_paths.max() < 7 and ds.item_paths.min() >= 0
    assert ds.num_targets_per_batch == 4 and ds.num_eval_targets_per_batch == 2
    assert dr_data.DRDataSet(_sample(rows), 3, 7, 4, 3, 3, 4, 2, 0.8).num_targets_per_batch == 1
    assert ds.train_seqs.shape == (ds.train_size, 4) and ds.train_seqs.dtype == np.int32 and len(ds.eval_labels) == len(ds.eval_users) == len(ds.eval_seqs)
    assert [l[0] for l in ds.eval_labels] == ds.eval_targets.tolist() and ds.id_item_map[ds.item_id_map[203]] == 203
    # the mapping file instead of a fresh mapping
    items = sorted(ds.item_id_map, key=ds.item_id_map.get)[::-1]
    path = str(tmp_path / "m.bin")
    dr_io.write_mapping(path, items, [ds.item_id_map[i] for i in items], ds.item_paths[[ds.item_id_map[i] for i in items]])
    ds2 = dr_data.DRDataSet(_sample(rows), 3, 7, 2, 9, 5, 4, 2, 0.8, initialize_mapping=False, mapping_path=path)
    assert ds2.item_id_map == ds.item_id_map and np.array_equal(ds2.item_paths, ds.item_paths) and np.array_equal(ds2.train_seqs, ds.train_seqs)


# ------------------------------------------------------------------------------------------------------------------ the files
def _second_reader():
    """tests/golden/make_fixtures.py decodes the reference's mapping file on its own; it is imported only when that has no side effect"""
    path = os.path.join(GOLDEN, "make_fixtures.py")
    text = open(path).read()
    if '__name__ == "__main__"' not in text:
        return None
    spec = importlib.util.spec_from_file_location("make_fixtures_for_dr_io", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.read_dr_mapping


def test_mapping_file_round_trips(tmp_path):
    g = np.load(os.path.join(GOLDEN, "dr_mapping.npz"))
    cases = [(g["items"], g["ids"], g["paths"]),
             (np.array([0, 5, -3, 2 ** 31 - 1], np.int32), np.array([3, 0, 2, 1], np.int32), np.array([[[0, 0]], [[0, 7]], [[300, 0]], [[2 ** 20, 1]]], np.int32))]
    reader = _second_reader()
    assert reader is not None
    for k, (items, ids, paths) in enumerate(cases):
        path = str(tmp_path / ("m%d.bin" % k))
        dr_io.write_mapping(path, items, ids, paths)
        m = dr_io.read_mapping(path)
        assert np.array_equal(m["items"], items) and np.array_equal(m["ids"], ids) and np.array_equal(m["paths"], paths) and m["paths"].dtype == np.int32
        other = reader(path)
        assert np.array_equal(other["items"], items) and np.array_equal(other["ids"], ids) and np.array_equal(other["paths"], paths)
        data = open(path, "rb").read()
        assert int.from_bytes(data[:4], "big") == len(data) - 4 and dr_io.mapping_bytes(m["items"], m["ids"], m["paths"]) == data
    with pytest.raises(ValueError):
        dr_io.parse_mapping(b"\x00\x00\x10\x00abc")


class _FakeEngine:
    """what save_model reads and load_model writes, without a device"""

    def __init__(self, dims, dtype, rerank, rng):
        from dismember_amd.dr_train import init_layer_weights, init_rerank_weights, pack_params, pack_rerank
        E, L, K, D, ni = dims
        self.dr_dims = dict(E=E, L=L, K=K, D=D, num_item=ni, dtype=np.dtype(dtype))
        w = init_layer_weights(ni, L, K, D, E, rng, dtype)
        w["layer_b"] = [rng.standard_normal(K).astype(dtype) for _ in range(D)]
        self.vec = pack_params(w, dtype)
        self.rr = pack_rerank(init_rerank_weights(ni, L, E, rng, dtype), dtype) if rerank else None
        self.loaded = None

    def dr_train_download(self, what):
        assert what == "weights"
        return self.vec

    def dr_rerank_download(self, vec, what="weights"):
        from dismember_amd import DismemberError
        if self.rr is None:
            raise DismemberError(-3, "model was loaded without rerank arrays")
        return self.rr[0 if vec == "graph" else 1]

    def dr_load_model(self, weights, E, L, K, D, num_item, dtype):
        self.loaded = (weights, (E, L, K, D, num_item), np.dtype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rerank", [False, True])
def test_model_file_round_trips(tmp_path, dtype, rerank):
    from dismember_amd.dr_train import init_layer_weights, pack_params, pack_rerank
    dims = (16, 3, 5, 3, 11)
    eng = _FakeEngine(dims, dtype, rerank, np.random.default_rng(4))
    path = str(tmp_path / "model.bin")
    dr_io.save_model(path, eng)
    data = open(path, "rb").read()
    n = eng.vec.size + (eng.rr[0].size + eng.rr[1].size if rerank else 0)
    assert data[:8] == b"DMDRMODL" and len(data) == 8 + 6 * 4 + 8 + 4 + n * np.dtype(dtype).itemsize
    d = dr_io.load_model(eng, path)
    w, got_dims, dt = eng.loaded
    assert got_dims == dims and dt == np.dtype(dtype) and d["num_item"] == 11
    assert pack_params(w, dtype).tobytes() == eng.vec.tobytes()
    assert ("rerank_emb" in w) == rerank
    if rerank:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pack_rerank(w, dtype), eng.rr))
    with open(path, "ab") as f:
        f.write(b"x")
    with pytest.raises(ValueError):
        dr_io.read_model(path)
    lw = init_layer_weights(11, 3, 5, 3, 16, np.random.default_rng(0))
    assert lw["layer_emb"].shape == (11 + 5 * 2, 16) and [w_.shape for w_ in lw["layer_w"]] == [(5, 48), (5, 64), (5, 80)]
    assert all(not b.any() for b in lw["layer_b"]) and 0.03 < lw["layer_emb"].std() < 0.07 and lw["layer_emb"].dtype == np.float64


# ------------------------------------------------------------------------------------------------------------------ declarations
def test_entry_points_are_declared_everywhere():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_jni
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dismember_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "jni", "dismember_jni.c")).read()
    scala = open(os.path.join(ROOT, "scala", "com", "mass", "hip", "Native.scala")).read()
    for name, nargs in ENTRY_POINTS.items():
        decl = re.search(r"\bint %s\(([^)]*)\)" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs, name
        m = gen_jni.camel(name)
        assert "Java_com_mass_hip_Native_%s(" % m in shim and re.search(r"@native def %s\(" % m, scala), name
    from dismember_amd import tasks
    from dismember_amd.engine import Engine
    for meth in ("dr_set_item_paths", "dr_path_items_download", "dr_item_paths_download", "dr_train_set_load", "dr_train_set_free", "dr_train_set_size", "dr_train_set_shuffle",
                 "dr_train_set_order", "dr_train_set_forward_backward", "dr_train_set_rerank_forward_backward", "dr_train_set_mstep"):
        assert callable(getattr(Engine, meth)), meth
    assert tasks.TASK_FUNCS["DRTrainDeepModel"] is tasks.dr_train_deep_model and tasks.TASK_FUNCS["DRCoordinateDescent"] is tasks.dr_coordinate_descent
    assert "TDMClusterTree" not in tasks.TASK_FUNCS
