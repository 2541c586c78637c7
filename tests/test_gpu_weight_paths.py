"""Every route to the same DIN weights gives bit-identical results.

A model is one compact vector; the fragment orders, transposes, b1 / w2 / b2 and (f64 models) the f32 mirror are derived from it on the
device (csrc/model_weights.hip.inc).  The routes below reach that derivation from the host loader, from a device buffer handed over
through the C ABI, from a checkpoint and from dm_train_init; whatever reads the derived copies afterwards — the general forward in
both history-length regimes and both batch regimes, the beam searches under every scorer arithmetic — must not be able to tell them
apart.  Small shapes: a depth-5 tree (63 nodes), so every case takes well under a second.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import random_din_weights, random_histories, synthetic_tree

pytestmark = pytest.mark.gpu

DEPTH, NI = 5, 63
CASES = [(16, np.float32), (32, np.float32), (128, np.float32), (24, np.float32), (32, np.float64), (128, np.float64)]
NATIVE = (16, 32, 64, 128)


@functools.lru_cache(maxsize=None)
def _inputs(E, dtype):
    rng = np.random.default_rng(1000 + E + (7 if dtype == np.float64 else 0))
    tree = synthetic_tree(rng, DEPTH, 1 << DEPTH)
    w = random_din_weights(rng, E, NI, dtype=dtype)
    users = random_histories(rng, tree["leaf_ids"], 4, 10)
    otm_codes = rng.integers((1 << DEPTH) - 1, NI, (4, 10)).astype(np.int32)
    otm_codes[0, 6:] = -1
    fwd = {}
    for B in (300, 8):
        for L in (10, 20):
            codes = rng.integers(0, NI, B).astype(np.int32)
            seqs = rng.integers(0, NI, (B, L)).astype(np.int32)
            npad = rng.integers(0, L // 2, B)
            pad = []
            for r in range(B):
                seqs[r, :npad[r]] = -1
                pad += [r * L + j for j in range(npad[r])]
            fwd[(B, L)] = (codes, seqs, np.asarray(pad, np.int32))
    for a in (w, users, otm_codes) + tuple(x for v in fwd.values() for x in v):
        a.setflags(write=False)
    return tree, w, users, otm_codes, fwd


def _new_engine(tree):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    return eng


def _load(route, E, dtype, tmp_path):
    """An engine holding the case's weights, reached by `route`."""
    from dismember_amd import _native as N
    tree, w, _, _, _ = _inputs(E, dtype)
    eng = _new_engine(tree)
    if route == "dev":          # a device buffer handed over through the C ABI: the handle owns it afterwards
        d = eng.dev_alloc(w.nbytes)
        eng.h2d(d, w)
        load = N.lib().dm_load_weights_din_dev_f64 if dtype == np.float64 else N.lib().dm_load_weights_din_dev
        eng._chk(load(eng._h, E, NI, d, w.size))
        eng.E, eng.dtype, eng.num_index = E, np.dtype(dtype), NI
        return eng
    eng.load_weights_din(w, E, NI)
    if route == "checkpoint":
        path = str(tmp_path / "model.ck")
        eng.save_model(path)
        eng.close()
        eng = _new_engine(tree)
        eng.load_model(path)
    elif route == "train_init":  # rebuilds every derived copy while the weights have not moved
        eng.train_init()
    else:
        assert route == "host"
    return eng


def _results(eng, E, dtype):
    """name -> array, for everything that reads a derived copy."""
    _, _, users, otm_codes, fwd = _inputs(E, dtype)
    out = {}
    # The explicit split arithmetic runs before "auto": on a handle with training state AUTO keeps the fp32-input kernels for small
    # requests while the split copies are stale; once they are built it is the same arithmetic on every route.
    modes = ["f32", "split_f16", "auto"] if _kernel_embed(E) % 32 == 0 else ["f32", "auto"]      # (no split scorer at E = 16)
    for mode in modes:
        eng.set_scorer_mode(mode)
        if dtype == np.float64:
            ids, sc, cnt = eng.otm_beam_search(otm_codes, 8, DEPTH)
            _put_beam(out, mode + "/otm", ids, sc, cnt)
        else:
            ids, sc, cnt, tc, ts, tn = eng.tdm_beam_search_trace(users, 8, 5)
            _put_beam(out, mode + "/tdm", ids, sc, cnt)
            out[mode + "/tdm/trace_codes"], out[mode + "/tdm/trace_scores"], out[mode + "/tdm/trace_counts"] = tc, ts, tn
        for (B, L), (codes, seqs, pad) in fwd.items():
            out["%s/forward/B%d/L%d" % (mode, B, L)] = eng.din_forward(codes, seqs, pad, L)
    if dtype == np.float64:
        ids, sc, cnt = eng.otm_beam_search_f64(otm_codes, 8, DEPTH)
        _put_beam(out, "otm_f64", ids, sc, cnt)
    return out


def _kernel_embed(E):
    return next(n for n in NATIVE if E <= n)


def _put_beam(out, name, ids, sc, cnt):
    """The result rows up to each user's count (the rest of the caller's buffers is not written)."""
    out[name + "/counts"] = cnt
    out[name + "/ids"] = np.concatenate([ids[u, :cnt[u]] for u in range(len(cnt))])
    out[name + "/scores"] = np.concatenate([sc[u, :cnt[u]] for u in range(len(cnt))])


@functools.lru_cache(maxsize=None)
def _reference(E, dtype):
    """Route (a), the host loader: computed once per case and shared."""
    eng = _load("host", E, dtype, None)
    ref = _results(eng, E, dtype)
    eng.close()
    for v in ref.values():
        v.setflags(write=False)
    return ref


ROUTES = [(E, dt, r) for E, dt in CASES for r in ("dev", "checkpoint", "train_init") if r != "dev" or E in NATIVE]


@pytest.mark.parametrize("E,dtype,route", ROUTES, ids=["E%d-%s-%s" % (E, np.dtype(dt).name, r) for E, dt, r in ROUTES])
def test_every_route_to_the_same_weights_is_bit_identical(E, dtype, route, tmp_path):
    ref = _reference(E, dtype)
    eng = _load(route, E, dtype, tmp_path)
    got = _results(eng, E, dtype)
    eng.close()
    assert sorted(got) == sorted(ref)
    assert any(v.size for k, v in ref.items() if k.endswith("/ids")), "the searches returned nothing: the comparison would be empty"
    bad = [k for k in ref if not (got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]))]
    assert not bad, "route %r differs from the host loader in %s" % (route, bad)
