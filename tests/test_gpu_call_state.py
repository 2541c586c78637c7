"""What a beam-search call needs lives in the call (its plan, its arguments), not on the handle: no call depends on the one before
it, every launch is recorded under its own kind, and the scored-rows counter belongs to the last counted search alone."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import random_din_weights, random_histories, synthetic_tree

pytestmark = pytest.mark.gpu

E, DEPTH, N_ITEMS, L, BEAM, TOPK, U = 32, 8, 200, 10, 20, 10, 64
NI = (1 << (DEPTH + 1)) - 1
KIND_MAIN, KIND_DEFERRED, KIND_ROWS = 0, 1, 30          # dm_kernel_timing_get_kind


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(2024)
    t = synthetic_tree(rng, DEPTH, N_ITEMS)
    first = (1 << DEPTH) - 1
    codes = (first + rng.integers(0, 1 << DEPTH, (U, L))).astype(np.int32)          # OTM histories: node codes of the leaf level
    codes[rng.random((U, L)) < 0.2] = -1
    return SimpleNamespace(tree=t, w=random_din_weights(rng, E, NI), seqs=random_histories(rng, t["leaf_ids"], U, L), codes=codes)


def make_engine(world):
    from dismember_amd import Engine
    eng = Engine(0)
    t = world.tree
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_din(world.w, E, NI)
    return eng


@pytest.fixture(scope="module")
def eng(world):
    e = make_engine(world)
    yield e
    e.close()


def tdm(eng, world):
    return eng.tdm_beam_search(world.seqs, BEAM, TOPK)


def brute(eng, world):
    return eng.tdm_bruteforce_topk(world.seqs, TOPK)


def otm(eng, world):
    return eng.otm_beam_search(world.codes, BEAM, DEPTH)


# the order of the issue: (scorer mode set before the call, the call)
SEQUENCE = [("auto", tdm), ("auto", brute), ("f32", tdm), ("f32", brute), ("auto", otm)]


@pytest.fixture(scope="module")
def alone(world):
    """Every call of SEQUENCE on a fresh handle that makes no other call.  The brute-force oracle always scores with the fp32-input
    MFMA, whatever the mode: one reference, taken in the default mode."""
    ref = {}
    for mode, call in SEQUENCE:
        key = ("any", call) if call is brute else (mode, call)
        if key in ref:
            continue
        e = make_engine(world)
        if call is not brute:
            e.set_scorer_mode(mode)
        ref[key] = call(e, world)
        e.close()
    return ref


def bits(result):
    return tuple(np.ascontiguousarray(a).tobytes() for a in result)


def run_sequence(e, world, alone, steps):
    got_brute = []
    for mode, call in steps:
        e.set_scorer_mode(mode)
        got = call(e, world)
        want = alone[("any", call) if call is brute else (mode, call)]
        assert bits(got) == bits(want), (mode, call.__name__)
        if call is brute:
            got_brute.append(got)
    assert len(got_brute) == 2 and bits(got_brute[0]) == bits(got_brute[1])


def test_no_call_depends_on_the_one_before_it(eng, world, alone):
    try:
        run_sequence(eng, world, alone, SEQUENCE)
        assert eng.last_beam_kernel() != ""
    finally:
        eng.set_scorer_mode("auto")
    other = make_engine(world)
    try:
        run_sequence(other, world, alone, SEQUENCE[::-1])
    finally:
        other.close()


def counts(eng):
    return eng.timing_get_kind(KIND_MAIN)[0], eng.timing_get_kind(KIND_DEFERRED)[0], eng.timing_get()[0]


def test_auto_search_records_the_main_kernel_and_the_deferred_pass(eng, world):
    eng.set_scorer_mode("auto")
    eng.timing_reset()
    tdm(eng, world)
    assert counts(eng) == (1, 1, 2)
    assert eng.last_beam_kernel().startswith("dm_beam_w_kernel")          # the deferred pass does not overwrite the name


def test_refused_call_leaves_nothing_behind(eng, world):
    from dismember_amd import DismemberError
    eng.set_scorer_mode("auto")
    with pytest.raises(DismemberError):
        eng.tdm_beam_search(world.seqs, BEAM, 0)
    eng.timing_reset()
    tdm(eng, world)
    assert counts(eng) == (1, 1, 2)
    assert eng.last_beam_kernel().startswith("dm_beam_w_kernel")


def test_f32_search_is_one_main_launch_and_the_single_request_path_records_nothing(eng, world):
    try:
        eng.set_scorer_mode("f32")
        eng.timing_reset()
        many = tdm(eng, world)
        assert counts(eng) == (1, 0, 1)
        eng.timing_reset()
        one = eng.tdm_beam_search(world.seqs[:1], BEAM, TOPK)
        timed_direct = os.environ.get("DM_TIME_DIRECT") == "1" or os.environ.get("DM_NO_DIRECT") == "1"
        assert eng.timing_get()[0] == (1 if timed_direct else 0)
        assert bits(one) == bits(tuple(a[:1] for a in many))
    finally:
        eng.set_scorer_mode("auto")


def test_general_rows_are_their_own_kind(eng, world):
    eng.set_scorer_mode("auto")
    rng = np.random.default_rng(7)
    node = rng.integers(0, NI, 64).astype(np.int32)
    eng.timing_reset()
    out = eng.din_forward(node, world.codes[:64])
    assert out.shape == (64,) and np.isfinite(out).all()
    assert eng.timing_get_kind(KIND_ROWS)[0] == 1
    assert eng.timing_get_kind(KIND_MAIN)[0] == 0 and eng.timing_get_kind(KIND_DEFERRED)[0] == 0


def test_scored_rows_belong_to_the_last_counted_search(eng, world):
    d_seq, d_ids, d_sc, d_cnt = eng.dev_alloc(U * L * 4), eng.dev_alloc(U * TOPK * 4), eng.dev_alloc(U * TOPK * 4), eng.dev_alloc(U * 4)
    try:
        eng.set_scorer_mode("f32")
        eng.h2d(d_seq, world.seqs)
        eng.tdm_beam_search_dev(d_seq, U, L, BEAM, TOPK, d_ids, d_sc, d_cnt)
        eng.synchronize()
        rows_dev = eng.last_scored_rows()
        assert rows_dev > 0
        tdm(eng, world)
        assert eng.last_scored_rows() == rows_dev
        eng.tdm_beam_search(world.seqs[:1], BEAM, TOPK)          # single-request path: counts into the sink slot
        if os.environ.get("DM_NO_DIRECT") != "1":
            assert eng.last_scored_rows() == rows_dev
        tdm(eng, world)
        assert eng.last_scored_rows() == rows_dev
    finally:
        eng.set_scorer_mode("auto")
        for d_ in (d_seq, d_ids, d_sc, d_cnt):
            eng.dev_free(d_)
