"""The lazily rebuilt copies of a model never serve stale weights.

The split-fp16 scorer's scales, W1a planes and pre-split table, the general-rows planes, an f64 model's f32 mirror and the fp64 beam
fragments are rebuilt on first use after the weights change (csrc/lazy_copies.hip.inc) — inside a training loop only in the rows the
Adam step visited, when nothing else can have moved.  A wrong transition there does not crash: it answers from old weights.  So after
every sequence of events below, a handle's results must be bit-identical to those of a FRESH handle that loads the first handle's
downloaded weights, under the same scorer mode: the beam search with its level trace, the general forward (B = 300, L = 10) and the
name of the search kernel.

Shapes: a depth-9 tree (1 023 rows), 4 users, L = 10, beam 8, topk 5.  Training batches of 8 rows take their codes and histories from
a pool of 64 row indices, so at most 64 rows are active and 4 * 64 < 1 023: the sparse Adam path.  One row outside the pool holds a
planted 1.5 (the other weights are N(0, 0.05)): the table's scale is pinned to a row no step touches.
"""
import functools

import numpy as np
import pytest

from helpers import random_din_weights, random_histories, synthetic_tree

pytestmark = pytest.mark.gpu

DEPTH, NI, L, BEAM, TOPK, POOL, PLANTED = 9, 1023, 10, 8, 5, 64, 1.5
F32_E = [32, 128]


@functools.lru_cache(maxsize=None)
def _inputs(E, dtype, seed=0):
    rng = np.random.default_rng(4200 + E + seed + (7 if dtype == np.float64 else 0))
    tree = synthetic_tree(rng, DEPTH, 1 << DEPTH)
    rows = rng.permutation(NI)
    pool, planted_row = np.sort(rows[:POOL]), int(rows[POOL])
    w = random_din_weights(rng, E, NI, dtype=dtype)
    w[planted_row * E + 3] = PLANTED
    users = random_histories(rng, tree["leaf_ids"], 4, L)
    otm_codes = rng.integers((1 << DEPTH) - 1, NI, (4, L)).astype(np.int32)
    otm_codes[0, 6:] = -1
    codes = rng.integers(0, NI, 300).astype(np.int32)
    seqs = rng.integers(0, NI, (300, L)).astype(np.int32)
    npad = rng.integers(0, L // 2, 300)
    pad = []
    for r in range(300):
        seqs[r, :npad[r]] = -1
        pad += [r * L + j for j in range(npad[r])]
    fwd = (codes, seqs, np.asarray(pad, np.int32))
    for a in (pool, w, users, otm_codes) + fwd:
        a.setflags(write=False)
    return dict(tree=tree, pool=pool, planted_row=planted_row, w=w, users=users, otm_codes=otm_codes, fwd=fwd, E=E, dtype=dtype)


def _engine(inp, w, mode):
    from dismember_amd import Engine
    t = inp["tree"]
    eng = Engine(0)
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_din(w, inp["E"], NI)
    eng.set_scorer_mode(mode)
    return eng


def _step(eng, inp, seed, pool=None):
    """One forward/backward over 8 rows drawn from the pool and one Adam step; returns the rows that received a gradient."""
    rng = np.random.default_rng(seed)
    pool = inp["pool"] if pool is None else pool
    codes = rng.choice(pool, 8).astype(np.int32)
    hist = rng.choice(pool, (8, L)).astype(np.int32)
    eng.train_forward_backward(codes, hist, None, (rng.random(8) < 0.5).astype(np.float32))
    eng.adam_step()
    return np.unique(np.concatenate([codes, hist.ravel()]))


def _results(eng, inp, f64_entry=False):
    """Everything compared, by name: the search (rows up to each user's count), its kernel, then the general forward."""
    out = {}
    if f64_entry:
        ids, sc, cnt = eng.otm_beam_search_f64(inp["otm_codes"], BEAM, DEPTH)
    elif inp["dtype"] == np.float64:
        ids, sc, cnt = eng.otm_beam_search(inp["otm_codes"], BEAM, DEPTH)
    else:
        ids, sc, cnt, tc, ts, tn = eng.tdm_beam_search_trace(inp["users"], BEAM, TOPK, max_levels=DEPTH + 2)
        out["trace_codes"], out["trace_scores"], out["trace_counts"] = tc, ts, tn
    assert cnt.sum() > 0, "the search returned nothing: the comparison would be empty"
    out["counts"] = cnt
    out["ids"] = np.concatenate([ids[u, :cnt[u]] for u in range(len(cnt))])
    out["scores"] = np.concatenate([sc[u, :cnt[u]] for u in range(len(cnt))])
    out["kernel"] = np.array(eng.last_beam_kernel())
    codes, seqs, pad = inp["fwd"]
    out["forward"] = eng.din_forward(codes, seqs, pad, L)
    return out


def _assert_like_fresh(eng, inp, mode, what, f64_entry=False, reader=None, fresh_mode=None):
    """`reader` (default: eng itself; a clone otherwise) answers under `mode` exactly like a fresh handle holding eng's weights.
    The fresh handle runs in the same scorer mode, with one exception (`fresh_mode`): AUTO inside a training loop keeps the fp32-input
    kernels for a small request, while a fresh AUTO handle, which is not training, takes the split kernels; the reference for that
    request is a fresh handle told to use "f32", and the caller asserts the kernel name.
    Equal results cannot tell a row-wise refresh from a full rescan (both are correct); that the rescan is avoided is
    test_gpu_edges.py::test_small_searches_inside_a_training_loop_skip_the_table_rebuild's subject, not this file's."""
    reader = eng if reader is None else reader
    reader.set_scorer_mode(mode)
    got = _results(reader, inp, f64_entry)
    fresh = _engine(inp, eng.train_download(), fresh_mode or mode)
    want = _results(fresh, inp, f64_entry)
    fresh.close()
    bad = [k for k in want if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not bad, "%s (%s): differs from a fresh handle with the same weights in %s (kernels %s / %s)" % (
        what, mode, bad, got["kernel"], want["kernel"])
    return got


def _rows(w, E, rows):
    return w[:NI * E].reshape(NI, E)[rows]


@pytest.mark.parametrize("E", F32_E)
def test_sparse_step_refreshes_the_active_rows(E):
    inp = _inputs(E, np.float32)
    eng = _engine(inp, inp["w"], "split_f16")
    _results(eng, inp)                                  # the split copies exist and are current
    eng.train_init(lr=1e-3)
    active = _step(eng, inp, 1)
    assert eng.adam_last_step_rows()[1], "expected the active-rows Adam path"
    moved = (_rows(eng.train_download(), E, active) != _rows(inp["w"], E, active)).any(axis=1)
    assert moved.all(), "an active row kept its loaded weights: the comparison below would be empty"
    _assert_like_fresh(eng, inp, "split_f16", "after a sparse step")
    _step(eng, inp, 2)
    assert eng.adam_last_step_rows()[1]
    _assert_like_fresh(eng, inp, "split_f16", "after a second sparse step")
    eng.close()


@pytest.mark.parametrize("E", F32_E)
def test_an_active_row_outgrows_the_scale(E):
    inp = _inputs(E, np.float32)
    eng = _engine(inp, inp["w"], "split_f16")
    _results(eng, inp)
    eng.train_init(lr=4.0)
    active = _step(eng, inp, 3)
    assert eng.adam_last_step_rows()[1]
    assert np.abs(_rows(eng.train_download(), E, active)).max() > 2 * PLANTED      # the scale of the last full scan no longer fits
    _assert_like_fresh(eng, inp, "split_f16", "after a step that outgrew the table's scale")
    _step(eng, inp, 4)
    _assert_like_fresh(eng, inp, "split_f16", "after the step behind it")
    eng.close()


@pytest.mark.parametrize("E", F32_E)
def test_dense_step(E, monkeypatch):
    inp = _inputs(E, np.float32)
    eng = _engine(inp, inp["w"], "split_f16")
    _results(eng, inp)
    eng.train_init(lr=1e-3)
    monkeypatch.setenv("DM_ADAM_DENSE", "1")
    _step(eng, inp, 5)
    assert not eng.adam_last_step_rows()[1], "DM_ADAM_DENSE=1 must take the dense stream"
    _assert_like_fresh(eng, inp, "split_f16", "after a dense step")
    monkeypatch.delenv("DM_ADAM_DENSE")
    _step(eng, inp, 6)                                  # a sparse step behind a dense one
    assert eng.adam_last_step_rows()[1]
    _assert_like_fresh(eng, inp, "split_f16", "after a sparse step behind a dense one")
    eng.close()


@pytest.mark.parametrize("E", F32_E)
def test_auto_mode_inside_a_training_loop(E):
    inp = _inputs(E, np.float32)
    eng = _engine(inp, inp["w"], "auto")
    assert _results(eng, inp)["kernel"].item().startswith("dm_beam_w_kernel")
    eng.train_init(lr=1e-3)
    _step(eng, inp, 7)
    assert eng.adam_last_step_rows()[1]
    # a small request keeps the fp32-input kernels while the split copies are stale: the same answers as a fresh handle told to
    # use that arithmetic
    got = _assert_like_fresh(eng, inp, "auto", "AUTO after a sparse step", fresh_mode="f32")
    assert got["kernel"].item() == "dm_beam_kernel<%d, 3, false>" % E
    got = _assert_like_fresh(eng, inp, "split_f16", "split_f16 after a sparse step")
    assert got["kernel"].item().startswith("dm_beam_w_kernel")
    eng.close()


def test_f64_model_mirror_and_fragments():
    inp = _inputs(32, np.float64)
    eng = _engine(inp, inp["w"], "split_f16")
    _results(eng, inp)
    _results(eng, inp, f64_entry=True)
    eng.train_init(lr=1e-3)
    active = _step(eng, inp, 8)
    assert (_rows(eng.train_download(), 32, active) != _rows(inp["w"], 32, active)).any(axis=1).all()
    for mode in ("f32", "split_f16"):                   # both read the f32 mirror
        _assert_like_fresh(eng, inp, mode, "f64 model after a step")
    _assert_like_fresh(eng, inp, "split_f16", "f64 model after a step, fp64 entry point", f64_entry=True)      # reads the fp64 fragments
    _step(eng, inp, 9)
    for mode in ("auto", "f64"):                        # the fp64 fragments first this time, through the shared entry point
        _assert_like_fresh(eng, inp, mode, "f64 model after a second step")
    _assert_like_fresh(eng, inp, "split_f16", "f64 model after a second step")
    _assert_like_fresh(eng, inp, "f32", "f64 model after a second step, fp64 entry point", f64_entry=True)
    eng.close()


@pytest.mark.parametrize("E", F32_E)
def test_clone_follows_its_parent(E):
    inp = _inputs(E, np.float32)
    eng = _engine(inp, inp["w"], "split_f16")
    eng.train_init(lr=1e-3)
    clone = eng.clone()
    _step(eng, inp, 10)
    _assert_like_fresh(eng, inp, "split_f16", "a clone taken before the step", reader=clone)
    _step(eng, inp, 11)
    _assert_like_fresh(eng, inp, "split_f16", "the clone after its parent's next step", reader=clone)
    _assert_like_fresh(eng, inp, "f32", "the clone under the fp32-input scorer", reader=clone)
    clone.close()
    eng.close()


@pytest.mark.parametrize("E", F32_E)
def test_train_init_twice_and_reload(E):
    inp = _inputs(E, np.float32)
    eng = _engine(inp, inp["w"], "split_f16")
    _results(eng, inp)
    eng.train_init(lr=1e-3)
    first = _step(eng, inp, 12)                         # no search behind it: these rows are stale in the split copies ...
    eng.train_init(lr=1e-3)
    others = np.setdiff1d(np.arange(NI), np.append(first, inp["planted_row"]))[:POOL]
    _step(eng, inp, 13, pool=others)                    # ... and are not among the second run's active rows
    assert eng.adam_last_step_rows()[1]
    _assert_like_fresh(eng, inp, "split_f16", "a step of a second training run")
    eng.train_init(lr=1e-3)                             # on a trained handle whose copies are current
    _assert_like_fresh(eng, inp, "split_f16", "dm_train_init on a trained handle")
    other = _inputs(E, np.float32, seed=100)
    eng.load_weights_din(other["w"], E, NI)
    assert np.array_equal(eng.train_download(), other["w"])
    _assert_like_fresh(eng, inp, "split_f16", "a reload of other weights")
    eng.close()
