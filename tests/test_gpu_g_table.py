"""The per-row setup table of the one-wave-per-SIMD beam kernel (DM_G_TABLE, csrc/lazy_copies.hip.inc: ensure_g_table).

Row c of the table is W1b (att.W emb[c]): what the kernel's per-user setup computes, with two products on the fp32 matrix pipe, for
a history position that holds code c.  The table is built by the same two-stage product (dmw_gemm16, beam_kernel_w.hip.inc), so a
search that gathers its rows must return what the search that multiplies returns, BIT FOR BIT: ids, scores, counts and every level
of the trace are compared with array_equal, DM_G_TABLE=1 against DM_G_TABLE=0 (the knob is read per call).  A wrong transition of the
table's stale flag does not crash, it answers from old weights: after every event of DESIGN.md §2's table a handle must answer like
a fresh handle that loads its weights.

Shapes: a depth-10 tree with 700 items (2 047 table rows) and 1 500 users, so that each of the 1 024 waves of a launch takes several
users in a row and a stale slot of the G planes, left by a longer history, would show.  E = 128 with L = 10 (the folded
attention-combine) and L = 12 (unfolded), E = 32 with L = 4 (the generic tile).  l1.b is kept small in these cases and every user's
max |G + b1| is checked in numpy to stay in the fp16 range, so that no user is handed to the LDS-fed kernel, whose setup the table
does not touch; the deferral test plants a bias that sends about half of the users there.
"""
import functools

import numpy as np
import pytest

from helpers import random_din_weights, random_histories, synthetic_tree

pytestmark = pytest.mark.gpu

DEPTH, N_ITEMS, U = 10, 700, 1500
NI = (1 << (DEPTH + 1)) - 1
CASES = [(128, 10), (128, 12), (32, 4)]          # (E, L): FOLD, unfolded, generic tile


def _histories(rng, tree, n, L):
    """Item-id histories with everything idToCode distinguishes: id 0 pads at the front (random_histories), at the back and in the
    middle, all-pad users, one item repeated, ancestor (non-leaf) ids, ids the tree does not know."""
    seqs = random_histories(rng, tree["leaf_ids"], n, L, unknown_prob=0.03)
    off = int(tree["leaf_ids"].max()) + 1                    # ancestors: id = code + offset (synthetic_tree)
    for u in range(n):
        k = u % 8
        if k == 1:
            seqs[u, L - 1 - (u // 8) % 2:] = 0               # pads at the back
        elif k == 2:
            seqs[u, (u // 8) % L] = 0                        # ... and in the middle
        elif k == 3 and u % 64 == 3:
            seqs[u] = 0                                      # all padding
        elif k == 4:
            seqs[u, L // 2:] = seqs[u, L - 1]                # one item repeated
        elif k == 5:
            seqs[u, (u // 8) % L] = off + 1 + (u * 7) % 900  # an ancestor's id (codes 1 .. 900 are inner nodes of a depth-10 tree)
    return seqs


@functools.lru_cache(maxsize=None)
def _world(E, L, bias_std=0.01):
    rng = np.random.default_rng(9100 + E + L)
    tree = synthetic_tree(rng, DEPTH, N_ITEMS)
    w = random_din_weights(rng, E, NI, bias_std=bias_std)
    seqs = _histories(rng, tree, U, L)
    first = (1 << DEPTH) - 1
    codes = rng.integers(0, NI, (U, L)).astype(np.int32)     # OTM histories: node codes of any level, -1 pads anywhere
    codes[rng.random((U, L)) < 0.2] = -1
    codes[7] = -1
    codes[8, :] = first + 5
    for a in (w, seqs, codes):
        a.setflags(write=False)
    return dict(tree=tree, w=w, seqs=seqs, codes=codes, E=E, L=L)


def _engine(tree, w, E, mode="split_f16"):
    from dismember_amd import Engine
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_din(w, E, NI)
    eng.set_scorer_mode(mode)
    return eng


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(E, L):
        if (E, L) not in made:
            wd = _world(E, L)
            made[(E, L)] = _engine(wd["tree"], wd["w"], E)
        return made[(E, L)]
    yield get
    for e in made.values():
        e.close()


NAMES = ("ids", "scores", "counts", "trace_codes", "trace_scores", "trace_counts")


def _search(eng, monkeypatch, knob, tdm_seqs=None, otm_codes=None, beam=20, topk=10, use_mask=True, depth=DEPTH):
    """One traced search under DM_G_TABLE = knob (None: unset).  Returns the six arrays and whether the setup read the table."""
    if knob is None:
        monkeypatch.delenv("DM_G_TABLE", raising=False)
    else:
        monkeypatch.setenv("DM_G_TABLE", knob)
    if tdm_seqs is not None:
        out = eng.tdm_beam_search_trace(tdm_seqs, beam, topk, use_mask=use_mask, max_levels=depth + 2)      # (explicit: a clone has no tree of its own to ask)
    else:
        out = eng.otm_beam_search_trace(otm_codes, beam, depth, depth + 1)
    assert out[2].sum() > 0, "the search returned nothing: the comparison would be empty"
    return out, eng.g_table_state()["used_last"]


def _assert_equal(got, want, what):
    bad = [n for n, a, b in zip(NAMES, got, want) if not (a.dtype == b.dtype and np.array_equal(a, b))]
    assert not bad, "%s: differs in %s" % (what, bad)


def _live(out):
    """The defined part of a search's six arrays: result rows up to each user's count, trace rows up to each level's count.  Two
    searches on ONE handle are compared whole (_assert_equal); two handles have two trace buffers, and the OTM trace leaves the
    slots past a level's count as it found them."""
    ids, sc, cnt, tc, ts, tn = out
    r = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    t = np.arange(tc.shape[2])[None, None, :] < tn[:, :, None]
    return ids[r], sc[r], cnt, tc[t], ts[t], tn


def _assert_equal_live(got, want, what):
    _assert_equal(_live(got), _live(want), what)


def _gm_and_threshold(eng, w, E, codes):
    """Per user max |G + b1| over the history positions (float64 restatement of the setup) and the bound from which the kernel hands
    a user to the LDS-fed kernel: (G + b1) 2^(S - sp) must fit fp16 with sp <= 15, S = shift_emb + shift_w, i.e. max |G + b1| < 2^(29 - S)."""
    w = w.astype(np.float64)
    emb = w[:NI * E].reshape(NI, E)
    att = w[NI * E:NI * E + E * E].reshape(E, E)
    l1 = w[NI * E + E * E:NI * E + 3 * E * E].reshape(E, 2 * E)
    b1 = w[NI * E + 3 * E * E:NI * E + 3 * E * E + E]
    K = np.where((codes >= 0)[..., None], emb[np.maximum(codes, 0)], 0.0)          # [U][L][E]; a pad's key row is zero
    G = (K @ att.T) @ l1[:, E:].T + b1
    s = eng.scorer_mode()
    return np.abs(G).max(axis=(1, 2)), 2.0 ** (29 - s["shift_emb"] - s["shift_w"])


def _tdm_codes(tree, seqs):
    """TDMTree.idToCode in numpy for synthetic_tree's id convention: 0 and unknown ids -> -1, leaf ids -> their code, ancestor ids ->
    id - offset."""
    off = int(tree["leaf_ids"].max()) + 1
    lut = np.full(off, -1, np.int64)
    lut[tree["leaf_ids"]] = tree["leaf_codes"]
    out = np.full(seqs.shape, -1, np.int64)
    leaf = (seqs > 0) & (seqs < off)
    out[leaf] = lut[seqs[leaf]]
    anc = (seqs >= off) & (seqs - off <= int(tree["leaf_codes"].max()))
    out[anc] = seqs[anc] - off
    return out


# --------------------------------------------------------------------------- on / off bit identity
@pytest.mark.parametrize("use_mask", [True, False])
@pytest.mark.parametrize("beam,topk", [(20, 10), (200, 100)])
@pytest.mark.parametrize("E,L", CASES)
def test_table_on_equals_table_off(engines, monkeypatch, E, L, beam, topk, use_mask):
    wd = _world(E, L)
    eng = engines(E, L)
    off_, used_off = _search(eng, monkeypatch, "0", tdm_seqs=wd["seqs"], beam=beam, topk=topk, use_mask=use_mask)
    on_, used_on = _search(eng, monkeypatch, "1", tdm_seqs=wd["seqs"], beam=beam, topk=topk, use_mask=use_mask)
    assert eng.last_beam_kernel() == "dm_beam_w_kernel<%d, %d, %s>" % (E, (L + 3) // 4, "true" if L <= 10 else "false")
    assert used_on and not used_off
    gm, bound = _gm_and_threshold(eng, wd["w"], E, _tdm_codes(wd["tree"], wd["seqs"]))
    assert gm.max() < 0.9 * bound, "a user would be deferred to the LDS-fed kernel: this case is about the W kernel's own setup"
    _assert_equal(on_, off_, "E = %d, L = %d, beam %d, use_mask %s" % (E, L, beam, use_mask))


@pytest.mark.parametrize("E,L", CASES)
def test_table_on_equals_table_off_otm(engines, monkeypatch, E, L):
    wd = _world(E, L)
    eng = engines(E, L)
    off_, used_off = _search(eng, monkeypatch, "0", otm_codes=wd["codes"])
    on_, used_on = _search(eng, monkeypatch, "1", otm_codes=wd["codes"])
    assert eng.last_beam_kernel().startswith("dm_beam_w_kernel<%d," % E)
    assert used_on and not used_off
    gm, bound = _gm_and_threshold(eng, wd["w"], E, wd["codes"].astype(np.int64))
    assert gm.max() < 0.9 * bound
    _assert_equal(on_, off_, "OTM mode, E = %d, L = %d" % (E, L))


# --------------------------------------------------------------------------- against the oracle
def test_table_on_against_the_oracle(oracle, engines, monkeypatch):
    """The existing contract with the table on: every score within 1e-5 + 1e-4 |s| of the oracle scorer, tree indices and item ids
    the exact replay of the oracle's integer logic on the device's scores (test_gpu_parity.replay_and_check)."""
    from test_gpu_parity import replay_and_check
    E, L = 128, 10
    wd = _world(E, L)
    t = wd["tree"]
    otree = oracle.TdmTree(t["codes"], t["ids"], t["is_leaf"], t["leaf_ids"], t["leaf_codes"], t["max_level"])
    odin = oracle.Din(wd["w"], E, L, NI)
    eng = engines(E, L)
    monkeypatch.setenv("DM_G_TABLE", "1")
    seqs = np.ascontiguousarray(wd["seqs"][:48])          # one of every kind of history (_histories cycles through them in 8s; user 3 is all padding)
    replay_and_check(otree, odin, eng, seqs, 20, 10)
    assert eng.g_table_state()["used_last"] and eng.last_beam_kernel() == "dm_beam_w_kernel<128, 3, true>"


# --------------------------------------------------------------------------- staleness
S_DEPTH, S_NI, S_L, S_BEAM, S_TOPK, S_POOL = 9, 1023, 10, 8, 5, 64


@functools.lru_cache(maxsize=None)
def _small(E, dtype, seed=0):
    rng = np.random.default_rng(7300 + E + seed + (5 if dtype == np.float64 else 0))
    tree = synthetic_tree(rng, S_DEPTH, 1 << S_DEPTH)
    w = random_din_weights(rng, E, S_NI, dtype=dtype)
    users = random_histories(rng, tree["leaf_ids"], 6, S_L)
    codes = rng.integers((1 << S_DEPTH) - 1, S_NI, (6, S_L)).astype(np.int32)
    codes[0, 6:] = -1
    pool = np.sort(rng.permutation(S_NI)[:S_POOL])
    for a in (w, users, codes, pool):
        a.setflags(write=False)
    return dict(tree=tree, w=w, users=users, codes=codes, pool=pool, E=E, dtype=dtype)


def _small_engine(inp, w):
    from dismember_amd import Engine
    t = inp["tree"]
    eng = Engine(0)
    eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    eng.load_weights_din(w, inp["E"], S_NI)
    eng.set_scorer_mode("split_f16")          # the W kernel also inside a training session
    return eng


def _small_search(eng, inp, monkeypatch, knob):
    if inp["dtype"] == np.float64:             # an f64 model's throughput search: the OTM entry point on its f32 mirror
        out, used = _search(eng, monkeypatch, knob, otm_codes=inp["codes"], beam=S_BEAM, depth=S_DEPTH)
    else:
        out, used = _search(eng, monkeypatch, knob, tdm_seqs=inp["users"], beam=S_BEAM, topk=S_TOPK, depth=S_DEPTH)
    assert eng.last_beam_kernel().startswith("dm_beam_w_kernel")
    return out, used


def _step(eng, inp, seed):
    rng = np.random.default_rng(seed)
    codes = rng.choice(inp["pool"], 8).astype(np.int32)
    hist = rng.choice(inp["pool"], (8, S_L)).astype(np.int32)
    eng.train_forward_backward(codes, hist, None, (rng.random(8) < 0.5).astype(np.float32))
    eng.adam_step()


def _assert_like_fresh(eng, inp, monkeypatch, what, reader=None):
    """`reader` (default: eng) answers with the table on exactly like a fresh handle that loads eng's weights, table on as well —
    and like that fresh handle with the table off."""
    got, used = _small_search(eng if reader is None else reader, inp, monkeypatch, "1")
    assert used, what
    fresh = _small_engine(inp, eng.train_download())
    want, used_f = _small_search(fresh, inp, monkeypatch, "1")
    plain, used_p = _small_search(fresh, inp, monkeypatch, "0")
    fresh.close()
    assert used_f and not used_p
    _assert_equal_live(got, want, what + " (against a fresh handle, table on)")
    _assert_equal_live(got, plain, what + " (against a fresh handle, table off)")
    return got


@pytest.mark.parametrize("E", [32, 128])
def test_table_follows_training_and_reload(monkeypatch, E):
    inp = _small(E, np.float32)
    eng = _small_engine(inp, inp["w"])
    first, used = _small_search(eng, inp, monkeypatch, None)          # DM_G_TABLE unset on a handle that is not training: built and read
    assert used and eng.g_table_state() == {"used_last": True, "current": True, "bytes": S_NI * E * 4}
    eng.train_init(lr=1e-3)
    # dm_train_init moved no weight: the table stays current and serves the next search, knob unset or not
    assert eng.g_table_state()["current"]
    again, used = _small_search(eng, inp, monkeypatch, None)
    assert used
    _assert_equal(again, first, "after dm_train_init")
    _assert_like_fresh(eng, inp, monkeypatch, "load, search, dm_train_init, search")
    _step(eng, inp, 1)
    assert not eng.g_table_state()["current"], "an Adam step moves att.W and W1b: every row of the table is stale"
    # knob unset inside the training session: the stale table is not rebuilt, the search multiplies — and answers like the table-off route
    auto, used_auto = _small_search(eng, inp, monkeypatch, None)
    off_, used_off = _small_search(eng, inp, monkeypatch, "0")
    assert not used_auto and not used_off and not eng.g_table_state()["current"]
    _assert_equal(auto, off_, "knob unset inside a training session")
    got = _assert_like_fresh(eng, inp, monkeypatch, "after one Adam step")
    _assert_equal(got, off_, "DM_G_TABLE=1 after one Adam step against DM_G_TABLE=0 on the same handle")
    assert not all(np.array_equal(a, b) for a, b in zip(got, first)), "the step changed no result: the comparisons above would be empty"
    assert eng.g_table_state()["current"]
    _step(eng, inp, 2)
    _assert_like_fresh(eng, inp, monkeypatch, "after a second Adam step")
    other = _small(E, np.float32, seed=50)
    eng.load_weights_din(other["w"], E, S_NI)
    eng.set_scorer_mode("split_f16")
    st = eng.g_table_state()
    assert not st["current"] and st["bytes"] == 0, "a load frees the old model's table"
    _assert_like_fresh(eng, inp, monkeypatch, "load of a second model")
    eng.close()


@pytest.mark.parametrize("E", [32, 128])
def test_clone_reads_its_owners_table(monkeypatch, E):
    inp = _small(E, np.float32)
    eng = _small_engine(inp, inp["w"])
    clone = eng.clone()
    clone.set_scorer_mode("split_f16")
    _assert_like_fresh(eng, inp, monkeypatch, "a clone's first search builds the owner's table", reader=clone)
    assert eng.g_table_state()["current"] and clone.g_table_state()["bytes"] == S_NI * E * 4
    eng.train_init(lr=1e-3)
    _step(eng, inp, 3)
    auto, used = _small_search(clone, inp, monkeypatch, None)          # the owner is training and its table is stale
    assert not used
    got = _assert_like_fresh(eng, inp, monkeypatch, "the clone after its owner's Adam step", reader=clone)
    _assert_equal_live(auto, got, "the clone with the knob unset")
    own, used = _small_search(eng, inp, monkeypatch, "1")
    assert used
    _assert_equal_live(own, got, "the owner reads the table its clone had built")
    clone.close()
    eng.close()


def test_f64_model_builds_from_its_mirror(monkeypatch):
    inp = _small(32, np.float64)
    eng = _small_engine(inp, inp["w"])
    first = _assert_like_fresh(eng, inp, monkeypatch, "f64 model after the load")
    eng.train_init(lr=1e-3)
    _step(eng, inp, 4)
    got = _assert_like_fresh(eng, inp, monkeypatch, "f64 model after a step (mirror rebuilt)")
    assert not all(np.array_equal(a, b) for a, b in zip(got, first))
    eng.close()


# --------------------------------------------------------------------------- deferred users
def test_deferred_users(monkeypatch):
    """A bias entry planted so that max |G + b1| of about half of the users leaves the fp16 range: those users are handed to the
    LDS-fed kernel (which keeps its own setup), the others stay.  Table on == table off for all of them."""
    E, L, n = 128, 10, 400
    wd = _world(E, L)
    codes = _tdm_codes(wd["tree"], wd["seqs"][:n])
    probe = _engine(wd["tree"], wd["w"], E)
    _search(probe, monkeypatch, "0", tdm_seqs=wd["seqs"][:8])          # (the scales exist after a search)
    _, bound = _gm_and_threshold(probe, wd["w"], E, codes)
    probe.close()
    # feature 3 of G without the bias, per user the largest value over the positions; the planted bias puts the bound at the median
    w = wd["w"].copy()
    w64 = w.astype(np.float64)
    emb, att = w64[:NI * E].reshape(NI, E), w64[NI * E:NI * E + E * E].reshape(E, E)
    w1b = w64[NI * E + E * E:NI * E + 3 * E * E].reshape(E, 2 * E)[:, E:]
    g3 = (np.where((codes >= 0)[..., None], emb[np.maximum(codes, 0)], 0.0) @ att.T @ w1b[3]).max(axis=1)
    w[NI * E + 3 * E * E + 3] = np.float32(bound - np.median(g3))
    eng = _engine(wd["tree"], w, E)
    seqs = np.ascontiguousarray(wd["seqs"][:n])
    off_, used_off = _search(eng, monkeypatch, "0", tdm_seqs=seqs)
    on_, used_on = _search(eng, monkeypatch, "1", tdm_seqs=seqs)
    gm, bound2 = _gm_and_threshold(eng, w, E, codes)
    assert bound2 == bound
    assert (gm > 1.001 * bound).sum() >= n // 4 and (gm < 0.999 * bound).sum() >= n // 4, "expected users on both sides of the fp16 bound"
    assert used_on and not used_off and eng.last_beam_kernel() == "dm_beam_w_kernel<128, 3, true>"
    _assert_equal(on_, off_, "with deferred users")
    eng.close()
