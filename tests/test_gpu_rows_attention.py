"""The general-rows DIN forward (dm_din_forward and what shares its kernels: JTM child weights, OTM pseudo targets, the training forward)
against the oracle at PEAKED attention: models of attention_cases.peaked_din_weights (embedding table N(0, 1): scores O(1), about
sqrt(E) where a key equals the query) and the rows of attention_cases.rows_case — random rows with masked and unmasked pads and masked
live keys, and the named rows (all keys masked, all pads, q = 0, the running maximum jumping at the first / last position, scores
sorted both ways, a mask bit at position L - 1, ...).  test_attention_cases_host.py proves on the CPU that these inputs stay inside fp32 and
that a softmax scale off by 5 %, a dropped position, an ignored mask bit or a leaked sixteenth position moves at least 40 % of the
rows it concerns (measured: 66 % .. 100 %) out of the tolerance; here EVERY row is held to it.

One test per kernel the dispatch can select (dm_hip.hip: dm_din_forward -> din_rows_dev -> launch_rows_split_E, din_forward_t); each
docstring names its kernel.  f32 models: ATOL + RTOL |ref| of test_gpu_parity.py against the f32 C oracle; f64 models: 1e-10 / 1e-9."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_cases as ac
import jtm_ref
from test_gpu_parity import ATOL, RTOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_ROWS, WAVES = 16, 8                       # rows of a wave's tile, waves of a workgroup (DM_NWAVES)


def _engine(d, mode=None):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_weights_din(d["w"], d["E"], ac.NI)
    if mode is not None:
        eng.set_scorer_mode(mode)
    return eng


def _check(got, ref, what, atol=ATOL, rtol=RTOL):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / (atol + rtol * np.abs(ref.astype(np.float64)))
    print("%s: max |err| / tolerance = %.3f over %d rows, max |ref| = %.3f" % (what, float(np.nanmax(err)), ref.size, float(np.abs(ref).max())))
    bad = np.flatnonzero(~(err <= 1.0))
    assert bad.size == 0, "%s: %d rows outside the tolerance, first %s: got %s, oracle %s" % (what, bad.size, bad[:6].tolist(), got[bad[:6]], ref[bad[:6]])


def _oracle_ref(oracle, d):
    return oracle.Din(d["w"], d["E"], d["L"], ac.NI).forward(d["codes"], d["seqs"], d["pad"])


def _named(d, bad_rows):
    inv = {i: n for n, i in d["names"].items()}
    return [inv.get(int(i), "random") for i in bad_rows]


@pytest.mark.parametrize("E,L", ac.MFMA_F32)
def test_fp32_input_mfma_kernel(oracle, E, L):
    """set_scorer_mode("f32"): din_rows_dev takes its second branch, launch_rows_E -> dm_din_rows_kernel<E> (fp32 inputs on
    v_mfma_f32_16x16x4_f32, attention with expf on the VALU); E = 16 has no other kernel."""
    d = ac.inputs(E, L)
    eng = _engine(d, "f32")
    try:
        assert eng.scorer_mode()["mode"] == "f32"
        got = eng.din_forward(d["codes"], d["seqs"], d["pad"])
    finally:
        eng.close()
    _check(got, _oracle_ref(oracle, d), "dm_din_rows_kernel<%d>, L = %d" % (E, L))


@pytest.mark.parametrize("E,L", ac.SPLIT_GENERIC)
def test_generic_split_kernel(oracle, E, L):
    """default (auto) mode at E = 32 / 64 / 128: din_rows_dev -> launch_rows_split_E, whose switch has no case for these L ->
    dm_din_rows_split_kernel<E> (fp16 hi / lo planes, attention with v_exp_f32 on pre-scaled scores, key ring filled by plain loads)."""
    d = ac.inputs(E, L)
    eng = _engine(d)
    try:
        assert eng.scorer_mode()["mode"] == "split_f16"
        got = eng.din_forward(d["codes"], d["seqs"], d["pad"])
    finally:
        eng.close()
    _check(got, _oracle_ref(oracle, d), "dm_din_rows_split_kernel<%d>, L = %d" % (E, L))


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from dismember_amd import Engine
w, codes, seqs, pad = (np.load(sys.argv[i]) for i in (1, 2, 3, 4)); out = sys.argv[5]
E, NI = int(sys.argv[6]), int(sys.argv[7])
eng = Engine(0); eng.load_weights_din(w, E, NI)
assert eng.scorer_mode()["mode"] == "split_f16"
np.save(out, eng.din_forward(codes, seqs, pad))
eng.close()
"""


def _generic_in_a_child(tmp_path, d):
    """the same request in a fresh process under DM_ROWS_GENERIC=1 (read once per process)"""
    files = [str(tmp_path / f) for f in ("w.npy", "c.npy", "s.npy", "p.npy", "o.npy")]
    for f, a in zip(files, (d["w"], d["codes"], d["seqs"], d["pad"])):
        np.save(f, a)
    env = dict(os.environ, DM_ROWS_GENERIC="1")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT] + files + [str(d["E"]), str(ac.NI)], env=env, check=True, timeout=300)
    return np.load(files[4])


@pytest.mark.parametrize("E,L", ac.SPLIT_COUNTED)
def test_counted_load_kernel(oracle, tmp_path, E, L):
    """default mode, L = 8 / 10 / 16: launch_rows_split_E -> launch_rows_split_EL<E, L> -> dm_din_rows_split_l_kernel<E, L> (indices
    staged in LDS one tile ahead, inline-assembly gathers with counted waits).  DM_ROWS_GENERIC=1 in a fresh process sends the same
    request to dm_din_rows_split_kernel<E>: the same arithmetic in the same order, so the same bits — masks and named rows included."""
    d = ac.inputs(E, L)
    eng = _engine(d)
    try:
        assert eng.scorer_mode()["mode"] == "split_f16"
        got = eng.din_forward(d["codes"], d["seqs"], d["pad"])
        again = eng.din_forward(d["codes"], d["seqs"], d["pad"])
    finally:
        eng.close()
    _check(got, _oracle_ref(oracle, d), "dm_din_rows_split_l_kernel<%d, %d>" % (E, L))
    assert np.array_equal(got, again)
    generic = _generic_in_a_child(tmp_path, d)
    differ = np.flatnonzero(got != generic)
    assert np.array_equal(got, generic), "counted-load and generic kernel differ in %d rows, first %s (%s)" % (differ.size, differ[:6].tolist(), _named(d, differ[:6]))


def _compute_units():
    """multiProcessorCount of device 0, what dm_create reads into n_cu: hipDeviceGetAttribute through the library's own HIP runtime
    (dlsym on the library's handle searches its dependencies); 63 = hipDeviceAttributeMultiprocessorCount of hip_runtime_api.h"""
    import ctypes as C
    from dismember_amd import _native
    fn = _native.lib().hipDeviceGetAttribute
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int(0)
    assert fn(C.byref(v), 63, 0) == 0 and 16 <= v.value <= 1024, v.value
    return v.value


@pytest.mark.parametrize("E,L", [(128, 8), (128, 10), (128, 16), (32, 8)])
def test_counted_load_kernel_second_tile_of_a_wave(oracle, E, L):
    """dm_din_rows_split_l_kernel<E, L> with more than one tile per wave: the grid is min(ceil(tiles / 8), CUs) workgroups, so
    B = 2 * 16 * 8 * CUs + 21 rows give every wave two tiles and the first two waves a third (a full tile and a partial one of 5 rows):
    only then the index staging of the NEXT tile (stage_idx(buf ^ 1)) is read.  The oracle checks a fixed sample of 3 000 rows with
    rows of first, second and third (last, partial) tiles; every row must equal, bit for bit, the same rows sent in chunks of at most
    16 * 8 * CUs rows, in which every wave takes one tile."""
    cus = _compute_units()
    per_pass = TILE_ROWS * WAVES * cus
    n_named = len(ac.inputs(E, L)["names"])
    d = ac.inputs(E, L, np.float32, 2 * per_pass + 21 - n_named)
    B = len(d["codes"])
    assert B == 2 * per_pass + 21
    rng = np.random.default_rng(77)
    sample = np.unique(np.concatenate([np.arange(64), rng.choice(per_pass, 1400, replace=False), per_pass + rng.choice(per_pass, 1400, replace=False),
                                       np.arange(2 * per_pass, B)]))
    rest = np.setdiff1d(np.arange(B), sample)
    sample = np.sort(np.concatenate([sample, rng.choice(rest, 3000 - sample.size, replace=False)]))
    assert sample.size == 3000 and np.unique(sample).size == 3000
    tile_pass = (sample // TILE_ROWS) // (WAVES * cus)
    assert (tile_pass == 0).sum() > 1000 and (tile_pass == 1).sum() > 1000 and (sample >= B - 5).sum() == 5 and tile_pass.max() == 2
    eng = _engine(d)
    try:
        assert eng.scorer_mode()["mode"] == "split_f16"
        got = eng.din_forward(d["codes"], d["seqs"], d["pad"])
        parts = []
        for a in range(0, B, per_pass):
            b = min(a + per_pass, B)
            parts.append(eng.din_forward(d["codes"][a:b], d["seqs"][a:b], ac.pad_flat(d["mask"][a:b])))
    finally:
        eng.close()
    ref = oracle.Din(d["w"], E, L, ac.NI).forward(d["codes"][sample], d["seqs"][sample], ac.pad_flat(d["mask"][sample]))
    _check(got[sample], ref, "dm_din_rows_split_l_kernel<%d, %d>, %d rows on %d CUs" % (E, L, B, cus))
    chunks = np.concatenate(parts)
    differ = np.flatnonzero(got != chunks)
    assert np.array_equal(got, chunks), "%d rows differ from the one-tile-per-wave run, first %s (tile passes %s)" % (
        differ.size, differ[:6].tolist(), ((differ[:6] // TILE_ROWS) // (WAVES * cus)).tolist())


@pytest.mark.parametrize("E,L", ac.LONG)
def test_long_history_forward(oracle, E, L):
    """f32 model, L = 17 .. 32: dm_din_forward skips din_rows_dev (L > DM_MAXL) -> din_forward_t<float> -> dm_din_forward_kernel<float>,
    one wave per row, mask bits 16 .. 31 in use."""
    d = ac.inputs(E, L)
    assert d["mask"][:, 16:].any() and d["mask"][d["names"]["mask_bit_last"], L - 1]
    eng = _engine(d)
    try:
        got = eng.din_forward(d["codes"], d["seqs"], d["pad"])
    finally:
        eng.close()
    _check(got, _oracle_ref(oracle, d), "dm_din_forward_kernel<float>, E = %d, L = %d" % (E, L))


@pytest.mark.parametrize("E,L", ac.F64)
def test_f64_model_both_kernels(oracle, E, L):
    """f64 model: din_forward_t<double>.  A request of at least 256 rows -> rows_fwd64 (the training kernel's forward half on
    v_mfma_f64_16x16x4_f64); the first 100 rows alone -> dm_din_forward_kernel<double>, one wave per row.  1e-10 / 1e-9 of the f64 oracle."""
    d = ac.inputs(E, L, np.float64)
    B = len(d["codes"])
    assert B >= 256 + 44 and d["w"].dtype == np.float64
    ref = _oracle_ref(oracle, d)
    eng = _engine(d)
    try:
        big = eng.din_forward(d["codes"], d["seqs"], d["pad"])
        small = eng.din_forward(d["codes"][:100], d["seqs"][:100], ac.pad_flat(d["mask"][:100]))
    finally:
        eng.close()
    _check(big, ref, "rows_fwd64, E = %d, L = %d, %d rows" % (E, L, B), atol=1e-10, rtol=1e-9)
    _check(small, ref[:100], "dm_din_forward_kernel<double>, E = %d, L = %d, 100 rows" % (E, L), atol=1e-10, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- seq_div > 1
J_DEPTH, J_LEAVES, J_E, J_L = 9, 300, 64, 8


@functools.lru_cache(maxsize=None)
def _jtm_world():
    from dismember_amd import synth
    tree = synth.make_tree(J_LEAVES, J_DEPTH, np.random.default_rng(78))
    cat = jtm_ref.make_catalogue(np.random.default_rng(1001), tree["leaf_ids"], tree["leaf_codes"], J_L)
    w = ac.peaked_din_weights(np.random.default_rng(79), J_E, ac.NI)
    return tree, cat, w


def test_history_shared_by_consecutive_rows(oracle):
    """seq_div > 1: JTM child weights over a cached catalogue read ONE history and one mask word per training row for its
    nchain = 6 chain nodes (two-level gap), din_rows_dev(..., seq_div = nchain) -> dm_din_rows_split_l_kernel<64, 8> with
    srow = row / seq_div; the uncached dm_jtm_child_weights expands the pairs and scores them with seq_div = 1.  Both against
    jtm_ref.sum_weights_f32 over the ORACLE's logits of the expanded pairs, within the sum of ATOL + RTOL |logit| over a weight's
    rows x gap logits (test_gpu_jtm_scoring.py (b)), and equal to each other bit for bit ((a) there)."""
    from dismember_amd import Engine
    from test_gpu_jtm_scoring import _cache, _cached, _uncache, _uncached
    assert (1 << (J_DEPTH + 1)) - 1 == ac.NI
    tree, cat, w = _jtm_world()
    old_level, level = 4, 6
    gap = level - old_level
    node = jtm_ref.ancestor_at_level(cat["item_code"], old_level).astype(np.int32)
    px = jtm_ref.expand_pairs(cat["row_off"], cat["row_ids"], node, J_L, old_level, level, cat["id_to_code"], cat["non_leaf_offset"], cat["max_code"],
                              num_index=ac.NI)
    assert not px["bad"] and px["mask"].any() and ((px["seqs"] < 0) & ~px["mask"]).any()          # masked pads and an unmasked zero key
    ref_logits = oracle.Din(w, J_E, J_L, ac.NI).forward(px["codes"], px["seqs"], jtm_ref.pad_flat(px["mask"]))
    w_ref = jtm_ref.sum_weights_f32(ref_logits, cat["row_off"], gap)
    bound = jtm_ref.chain_sum(ATOL + RTOL * np.abs(ref_logits.astype(np.float64)), cat["row_off"], gap)
    seen = np.diff(cat["row_off"]) > 0
    eng = Engine(0)
    try:
        eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], J_DEPTH)
        eng.load_id_maps(cat["map_ids"], cat["map_codes"])
        eng.load_weights_din(w, J_E, ac.NI)
        assert eng.scorer_mode()["mode"] == "split_f16"
        n = cat["items"].size
        uncached = _uncached(eng, cat, J_L, node, old_level, level, False, 0, True)
        _cache(eng, cat, J_L)
        try:
            cached = _cached(eng, node, 0, n, old_level, level, False, 0, True)
        finally:
            _uncache(eng, J_L)
    finally:
        eng.close()
    for name, got in (("cached (seq_div = 6)", cached), ("uncached (seq_div = 1)", uncached)):
        err = np.abs(got.astype(np.float64) - w_ref.astype(np.float64))
        print("%s: max err / bound = %.3f, max |w| = %.3f" % (name, float((err[seen] / bound[seen]).max()), float(np.abs(w_ref[seen]).max())))
        assert (got[~seen] == np.float32(-1e6)).all() and (w_ref[~seen] == np.float32(-1e6)).all()
        assert (err[seen] <= bound[seen]).all(), name
    assert np.array_equal(cached, uncached)
