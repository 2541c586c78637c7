"""The host-buffer search front ends over one request layout (csrc/host_request.hip.inc, ReqLayout): every front end, in every serving
mode it offers, gives byte for byte what the device-buffer entry point gives for the same users — the same plan and the same kernel run,
only the way the request goes up and the results come down differs (in place in the host-mapped block, through the pinned staging
block, plain copies).  Trace variants: the outputs of the untraced call, the live slots as the existing replays expect them, every
slot past a level's count zero.  Refusals: the texts of the history / target / index checks.

Run as a program (`python tests/test_gpu_host_request.py OUT.npz`) the file writes the one-user results of every front end: the test
of DM_NO_DIRECT=1 starts that as a fresh child process and compares."""
import ctypes as C
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dfm_otm_ref as D
from helpers import random_din_weights, random_histories, synthetic_tree

pytestmark = pytest.mark.gpu

E, DEPTH, N_ITEMS, L, BEAM, TOPK = 32, 8, 200, 8, 20, 16
NI = (1 << (DEPTH + 1)) - 1
DFM_E, DFM_LEAF = 16, 9
DR = dict(K=8, D=3, E=16, num_item=300, beam=8, topk=10)          # 512 paths, 4 per item: every path holds items
KIND_MAIN = 0                                    # dm_kernel_timing_get_kind
STAGE_BYTES = 256 << 10
ERR_INDEX = -4


def up(n):
    return (n + 255) & ~255


def head_bytes(U, stride, score_bytes, id_width=1):
    """[seq | ids | scores | counts] of the request layout: every array starts at a multiple of 256 bytes"""
    return up(U * L * 4) + up(U * stride * id_width * 4) + up(U * stride * score_bytes) + up(U * 4)


def first_plain_users(stride, score_bytes):
    """the smallest U whose head no longer fits the staging block"""
    U = 1
    while head_bytes(U, stride, score_bytes) <= STAGE_BYTES:
        U += 1
    assert head_bytes(U - 1, stride, score_bytes) <= STAGE_BYTES < head_bytes(U, stride, score_bytes)
    return U


def direct_expected():
    """the single-request path serves U <= 8 in place and records no event pair, unless the environment says otherwise"""
    return os.environ.get("DM_NO_DIRECT") != "1" and os.environ.get("DM_TIME_DIRECT") != "1"


@functools.lru_cache(maxsize=None)
def world():
    rng = np.random.default_rng(77)
    tree = synthetic_tree(rng, DEPTH, N_ITEMS)
    w64 = random_din_weights(rng, E, NI, dtype=np.float64)
    n_max = first_plain_users(TOPK, 4)
    items = random_histories(rng, tree["leaf_ids"], n_max, L)
    codes = rng.integers((1 << DEPTH) - 1, NI, (n_max, L)).astype(np.int32)          # OTM histories: node codes of the leaf level
    codes[rng.random(codes.shape) < 0.2] = -1
    codes[1] = -1
    dfm_w, dfm_ni = D.model(DFM_E, L, DFM_LEAF)
    dr_seqs = rng.integers(0, DR["num_item"], (9, L)).astype(np.int32)
    dr_seqs[rng.random(dr_seqs.shape) < 0.2] = -1
    return SimpleNamespace(tree=tree, w32=w64.astype(np.float32), w64=w64, items=items, codes=codes, dfm_w=dfm_w, dfm_ni=dfm_ni,
                           dfm_codes=D.histories(L, dfm_ni, 9), dr_seqs=dr_seqs)


def make_engines():
    from dismember_amd import Engine, synth
    wd = world()
    engs = {}
    e = engs["din32"] = Engine(0)
    t = wd.tree
    e.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
    e.load_id_maps(t["leaf_ids"], t["leaf_codes"])
    e.load_weights_din(wd.w32, E, NI)
    e = engs["din64"] = Engine(0)
    e.load_weights_din(wd.w64, E, NI)
    e = engs["dfm"] = Engine(0)
    e.load_weights_deepfm(wd.dfm_w, DFM_E, L, wd.dfm_ni)
    for name, dt in (("dr32", np.float32), ("dr64", np.float64)):
        rng = np.random.default_rng(9)
        e = engs[name] = Engine(0)
        e.dr_load_model(synth.make_dr_model(DR["num_item"], DR["K"], DR["D"], L, DR["E"], rng), DR["E"], L, DR["K"], DR["D"], DR["num_item"], dtype=dt)
        e.dr_load_path_items(*synth.dr_path_items(synth.make_dr_paths(DR["num_item"], DR["K"], DR["D"], 4, rng)))
    return engs


def on_device(eng, seqs, outs, launch, extra=()):
    """launch(d_seq, *d_outs, *d_extra) on device copies of seqs and of the `extra` arrays; outs: (shape, dtype) of the result arrays"""
    bufs = []
    try:
        for a in (seqs,) + tuple(extra):
            bufs.append(eng.dev_alloc(a.nbytes))
            eng.h2d(bufs[-1], a)
        d_outs = []
        for shape, dt in outs:
            d_outs.append(eng.dev_alloc(int(np.prod(shape)) * np.dtype(dt).itemsize))
            bufs.append(d_outs[-1])
        launch(bufs[0], *d_outs, *bufs[1:1 + len(extra)])
        eng.synchronize()
        res = []
        for (shape, dt), d in zip(outs, d_outs):
            res.append(np.empty(shape, dt))
            eng.d2h(res[-1], d)
        return tuple(res)
    finally:
        for b in bufs:
            eng.dev_free(b)


def search_outs(U, stride, score_dtype=np.float32):
    return [((U, stride), np.int32), ((U, stride), score_dtype), ((U,), np.int32)]


# ---- the front ends: (engine, host entry, device entry), each on seqs [U, L]
def tdm_host(engs, seqs, **kw):
    engs["din32"].set_scorer_mode("f32")
    return engs["din32"].tdm_beam_search(seqs, BEAM, TOPK, **kw)


def tdm_dev(engs, seqs):
    e, U = engs["din32"], len(seqs)
    e.set_scorer_mode("f32")
    return on_device(e, seqs, search_outs(U, TOPK), lambda d_seq, *o: e.tdm_beam_search_dev(d_seq, U, L, BEAM, TOPK, *o))


def otm32_host(engs, seqs):
    engs["din32"].set_scorer_mode("auto")
    return engs["din32"].otm_beam_search(seqs, BEAM, DEPTH)


def otm_dev(name, leaf_level):
    def run(engs, seqs):
        e, U = engs[name], len(seqs)
        if name == "din32":
            e.set_scorer_mode("auto")
        return on_device(e, seqs, search_outs(U, 2 * BEAM), lambda d_seq, *o: e.otm_beam_search_dev(d_seq, U, L, BEAM, leaf_level, *o))
    return run


def otm64_host(engs, seqs):
    return engs["din64"].otm_beam_search_f64(seqs, BEAM, DEPTH)


def otm64_host_f32_scores(engs, seqs):
    return engs["din64"].otm_beam_search(seqs, BEAM, DEPTH)


def dfm_host(engs, seqs):
    return engs["dfm"].otm_beam_search(seqs, BEAM, DFM_LEAF)


def dr_beam_host(name):
    return lambda engs, seqs: engs[name].dr_beam_search(seqs, DR["beam"])


def dr_beam_dev(name):
    def run(engs, seqs):
        e, U, b = engs[name], len(seqs), DR["beam"]
        return on_device(e, seqs, [((U, b, DR["D"]), np.int32), ((U, b), np.float64), ((U,), np.int32)],
                         lambda d_seq, *o: e.dr_beam_search_dev(d_seq, U, b, *o))
    return run


def dr_rec_host(name):
    return lambda engs, seqs: engs[name].dr_recommend(seqs, DR["beam"], DR["topk"])


def dr_rec_dev(name):
    def run(engs, seqs):
        e, U = engs[name], len(seqs)
        return on_device(e, seqs, search_outs(U, DR["topk"], np.float64), lambda d_seq, *o: e.dr_recommend_dev(d_seq, U, DR["beam"], DR["topk"], *o))
    return run


def bits(result):
    return tuple(np.ascontiguousarray(a).tobytes() for a in result)


def one_user_results(engs):
    """every front end on its first user alone: what DM_NO_DIRECT=1 must not change"""
    wd = world()
    calls = {"tdm": (tdm_host, wd.items), "otm32": (otm32_host, wd.codes), "otm64": (otm64_host, wd.codes),
             "otm64_f32_scores": (otm64_host_f32_scores, wd.codes), "dfm": (dfm_host, wd.dfm_codes)}
    for name in ("dr32", "dr64"):
        calls["beam_" + name] = (dr_beam_host(name), wd.dr_seqs)
        calls["rec_" + name] = (dr_rec_host(name), wd.dr_seqs)
    out = {}
    for name, (call, seqs) in calls.items():
        for i, a in enumerate(call(engs, seqs[:1])):
            out["%s.%d" % (name, i)] = a
    return out


@pytest.fixture(scope="module")
def engs():
    engines = make_engines()
    yield engines
    for e in engines.values():
        e.close()


# ---------------------------------------------------------------------------------------------- host entry == device entry
@pytest.mark.parametrize("users", ["one", "nine", "last_staged", "first_plain"])
def test_tdm_host_equals_device(engs, users):
    """f32 scorer mode.  U = 1: served in place, no event pair; U = 9: through the staging block, the main launch recorded; the two
    sizes on either side of the staging block's 256 KiB: the last staged request and the first plain one."""
    U = {"one": 1, "nine": 9, "last_staged": first_plain_users(TOPK, 4) - 1, "first_plain": first_plain_users(TOPK, 4)}[users]
    seqs = world().items[:U]
    eng = engs["din32"]
    eng.timing_reset()
    host = tdm_host(engs, seqs)
    recorded = eng.timing_get()[0]
    try:
        assert bits(host) == bits(tdm_dev(engs, seqs))
        if direct_expected():
            assert recorded == (0 if U == 1 else 1)
    finally:
        eng.set_scorer_mode("auto")


def test_tdm_consumed_lists_host_equals_device(engs):
    """consumed lists ride behind the head of the request: such a request is never staged"""
    from dismember_amd import _native as N
    U = 9
    wd = world()
    seqs = wd.items[:U]
    eng = engs["din32"]
    consumed = [[int(i) for i in wd.tree["leaf_ids"][u:u + 1 + u % 3]] for u in range(U)]
    off, cids = eng._csr(consumed, U)
    opts = N.SearchOpts(BEAM, TOPK, 1, 0)
    try:
        host = tdm_host(engs, seqs, consumed=consumed)
        dev = on_device(eng, seqs, search_outs(U, TOPK), extra=(off, cids), launch=lambda d_seq, d_ids, d_sc, d_cnt, d_off, d_cids: eng._chk(
            N.lib().dm_tdm_beam_search_dev(eng._h, d_seq, U, L, C.byref(opts), C.cast(d_off, N.i64p), C.cast(d_cids, N.i32p), d_ids, d_sc, d_cnt)))
        assert bits(host) == bits(dev)
        plain = tdm_host(engs, seqs)
        assert not np.array_equal(plain[0], host[0])                                  # the lists took part
    finally:
        eng.set_scorer_mode("auto")


@pytest.mark.parametrize("U", [1, 9])
def test_otm_fp32_host_equals_device(engs, U):
    """plain at every size: the main launch is recorded for one user too"""
    seqs = world().codes[:U]
    eng = engs["din32"]
    eng.timing_reset()
    host = otm32_host(engs, seqs)
    assert eng.timing_get_kind(KIND_MAIN)[0] == 1
    assert bits(host) == bits(otm_dev("din32", DEPTH)(engs, seqs))


@pytest.mark.parametrize("users", ["one", "nine", "last_staged", "first_plain"])
def test_otm_fp64_host_equals_device(engs, users):
    """fp64 model.  The device entry returns scores rounded to float: ids and counts exact, the f64 scores after the same rounding,
    and the host entry that returns float scores byte for byte."""
    n = first_plain_users(2 * BEAM, 8)
    U = {"one": 1, "nine": 9, "last_staged": n - 1, "first_plain": n}[users]
    seqs = world().codes[:U]
    eng = engs["din64"]
    eng.timing_reset()
    ids, sc, cnt = otm64_host(engs, seqs)
    recorded = eng.timing_get()[0]
    assert sc.dtype == np.float64
    dev = otm_dev("din64", DEPTH)(engs, seqs)
    assert bits((ids, sc.astype(np.float32), cnt)) == bits(dev)
    assert bits(otm64_host_f32_scores(engs, seqs)) == bits(dev)
    if direct_expected() and eng.last_beam_kernel().startswith("dm_beam64_kernel"):
        assert recorded == (0 if U == 1 else 1)


@pytest.mark.parametrize("U", [1, 9])
def test_otm_deepfm_host_equals_device(engs, U):
    seqs = world().dfm_codes[:U]
    assert bits(dfm_host(engs, seqs)) == bits(otm_dev("dfm", DFM_LEAF)(engs, seqs))


@pytest.mark.parametrize("U", [1, 9])
@pytest.mark.parametrize("name", ["dr32", "dr64"])
def test_deep_retrieval_host_equals_device(engs, name, U):
    """dr_beam_search (plain) and dr_recommend (U = 1: request and results in the host-mapped block; U = 9: plain)"""
    seqs = world().dr_seqs[:U]
    beam = dr_beam_host(name)(engs, seqs)
    assert bits(beam) == bits(dr_beam_dev(name)(engs, seqs))
    assert (beam[2] > 0).all()
    rec = dr_rec_host(name)(engs, seqs)
    assert bits(rec) == bits(dr_rec_dev(name)(engs, seqs))
    assert (rec[2] > 0).any()


def test_no_direct_child_gives_the_same_single_user_results(engs, tmp_path):
    """DM_NO_DIRECT=1 is read when a handle is created: a fresh child process"""
    out = str(tmp_path / "one_user.npz")
    env = dict(os.environ, DM_NO_DIRECT="1")
    done = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    here = one_user_results(engs)
    with np.load(out) as there:
        assert sorted(there.files) == sorted(here)
        for k, a in here.items():
            assert a.dtype == there[k].dtype and a.tobytes() == there[k].tobytes(), k


# ---------------------------------------------------------------------------------------------- traces
def dead_slots_are_zero(tc, ts, tn):
    live = np.arange(tc.shape[2])[None, None, :] < tn[:, :, None]
    assert (tc[~live] == 0).all() and (ts[~live] == 0).all()


def dirty_request_buffer(eng, seqs, otm):
    """a larger untraced search first: the handle's request buffer holds ids and scores where the trace arrays will lie"""
    big = np.tile(seqs, (8, 1))
    eng.otm_beam_search(big, BEAM, otm) if otm else eng.tdm_beam_search(big, BEAM, TOPK)


def test_tdm_trace(engs, oracle):
    from test_gpu_parity import replay_and_check
    wd = world()
    t = wd.tree
    seqs = wd.items[:9]
    eng = engs["din32"]
    try:
        plain = tdm_host(engs, seqs)
        dirty_request_buffer(eng, seqs, 0)
        ids, sc, cnt, tc, ts, tn = eng.tdm_beam_search_trace(seqs, BEAM, TOPK)
        assert bits((ids, sc, cnt)) == bits(plain)
        dead_slots_are_zero(tc, ts, tn)
        otree = oracle.TdmTree(t["codes"], t["ids"], t["is_leaf"], t["leaf_ids"], t["leaf_codes"], t["max_level"])
        replayed = replay_and_check(otree, oracle.Din(wd.w32, E, L, NI), eng, seqs, BEAM, TOPK)
        assert bits(replayed) == bits(plain)
    finally:
        eng.set_scorer_mode("auto")


@pytest.mark.parametrize("route", ["fp32", "fp64", "fp64_f32_scores"])
def test_otm_trace(engs, oracle, route):
    from test_gpu_precision import _otm_replay
    seqs = world().codes[:9]
    start_level = BEAM.bit_length() - 1
    levels = DEPTH - start_level
    eng = engs["din32" if route == "fp32" else "din64"]
    plain = (otm64_host if route == "fp64" else otm64_host_f32_scores if route == "fp64_f32_scores" else otm32_host)(engs, seqs)
    dirty_request_buffer(eng, seqs, DEPTH)
    if route == "fp64":
        ids, sc, cnt, tc, ts, tn = eng.otm_beam_search_f64(seqs, BEAM, DEPTH, trace_levels=levels + 1)
    else:
        ids, sc, cnt, tc, ts, tn = eng.otm_beam_search_trace(seqs, BEAM, DEPTH, levels + 1)
    assert bits((ids, sc, cnt)) == bits(plain)
    assert (tn[:, levels:] == 0).all()                                                # a level more than the search has
    dead_slots_are_zero(tc, ts, tn)
    _otm_replay(oracle, tc[:, :levels], ts[:, :levels], tn[:, :levels], BEAM, start_level, DEPTH, ids)
    for u in range(len(seqs)):
        n = int(tn[u, levels - 1])
        assert cnt[u] == n and np.array_equal(sc[u, :n], ts[u, levels - 1, :n].astype(sc.dtype))


def test_otm_deepfm_trace(engs):
    wd = world()
    seqs = wd.dfm_codes
    eng = engs["dfm"]
    levels = len(D.level_counts(BEAM, DFM_LEAF))
    plain = dfm_host(engs, seqs)
    dirty_request_buffer(eng, seqs, DFM_LEAF)
    r = eng.otm_beam_search_trace(seqs, BEAM, DFM_LEAF, levels + 1)
    assert bits(r[:3]) == bits(plain)
    dead_slots_are_zero(*r[3:])
    D.replay(seqs, BEAM, DFM_LEAF, r[:3], r[3:], lambda u, codes: D.ref_scores(wd.dfm_w, DFM_E, L, wd.dfm_ni, codes, seqs[u]))


# ---------------------------------------------------------------------------------------------- refusals
# the texts of the parent commit, byte for byte: "<entry point>: <noun> outside the embedding table"
HISTORY = "%s: history code outside the embedding table"
REFUSALS_DIN32 = {"otm_beam_search": HISTORY % "dm_otm_beam_search", "otm_beam_search_trace": HISTORY % "dm_otm_beam_search"}
REFUSALS_DIN64 = {"otm_beam_search": HISTORY % "dm_otm_beam_search", "otm_beam_search_f64": HISTORY % "dm_otm_beam_search",
                  "otm_beam_search_trace_f64": HISTORY % "dm_otm_beam_search"}
REFUSALS_DFM = {"otm_beam_search": HISTORY % "dm_deepfm_otm_beam_search", "otm_beam_search_trace": HISTORY % "dm_deepfm_otm_beam_search_trace"}
REFUSALS_TRAIN = {False: {"train_batch": HISTORY % "dm_otm_train_batch", "pseudo_targets": HISTORY % "dm_otm_pseudo_targets",
                          "pseudo_targets_target": "dm_otm_pseudo_targets: target outside the embedding table"},
                  True: {"train_batch": HISTORY % "dm_deepfm_otm_train_batch", "pseudo_targets": HISTORY % "dm_deepfm_otm_pseudo_targets",
                         "pseudo_targets_target": "dm_deepfm_otm_pseudo_targets: target outside the embedding table"}}
REFUSALS_ROWS = {"item": "dm_train_forward_backward: item index outside the embedding table",
                 "history": "dm_train_forward_backward: history index outside the embedding table"}


def refused(text, call):
    from dismember_amd import DismemberError
    with pytest.raises(DismemberError) as e:
        call()
    assert e.value.code == ERR_INDEX and str(e.value) == "dismember_hip error %d: %s" % (ERR_INDEX, text)


def bad_histories(seqs, num_index):
    """one bad code each: just past the table, and below the padding id"""
    for bad in (num_index, -2):
        s = seqs.copy()
        s[len(s) // 2, 3] = bad
        yield s


def test_search_refusals(engs):
    wd = world()
    levels = 3
    for s in bad_histories(wd.codes[:9], NI):
        e = engs["din32"]
        refused(REFUSALS_DIN32["otm_beam_search"], lambda: e.otm_beam_search(s, BEAM, DEPTH))
        refused(REFUSALS_DIN32["otm_beam_search_trace"], lambda: e.otm_beam_search_trace(s, BEAM, DEPTH, levels))
        e = engs["din64"]
        refused(REFUSALS_DIN64["otm_beam_search"], lambda: e.otm_beam_search(s, BEAM, DEPTH))
        refused(REFUSALS_DIN64["otm_beam_search_f64"], lambda: e.otm_beam_search_f64(s, BEAM, DEPTH))
        refused(REFUSALS_DIN64["otm_beam_search_trace_f64"], lambda: e.otm_beam_search_f64(s, BEAM, DEPTH, trace_levels=levels))
    for s in bad_histories(wd.dfm_codes, wd.dfm_ni):
        e = engs["dfm"]
        refused(REFUSALS_DFM["otm_beam_search"], lambda: e.otm_beam_search(s, BEAM, DFM_LEAF))
        refused(REFUSALS_DFM["otm_beam_search_trace"], lambda: e.otm_beam_search_trace(s, BEAM, DFM_LEAF, levels))
    good = otm32_host(engs, wd.codes[:9])                                             # a refused call leaves a handle that serves
    assert bits(good) == bits(otm_dev("din32", DEPTH)(engs, wd.codes[:9]))


@pytest.mark.parametrize("deepfm", [False, True], ids=["din", "deepfm"])
def test_training_refusals(deepfm):
    from dismember_amd import Engine
    from dismember_amd.otm_train import OTMTrainer
    wd = world()
    eng = Engine(0)
    try:
        if deepfm:
            eng.load_weights_deepfm(wd.dfm_w, DFM_E, L, wd.dfm_ni)
            seqs, ni, leaf = wd.dfm_codes, wd.dfm_ni, DFM_LEAF
        else:
            eng.load_weights_din(wd.w32, E, NI)
            seqs, ni, leaf = wd.codes[:9], NI, DEPTH
        tr = OTMTrainer(eng, leaf, BEAM, seq_len=L)
        first_leaf = (1 << leaf) - 1
        targets = [[first_leaf + 3 * u, first_leaf + 3 * u + 1] for u in range(len(seqs))]
        texts = REFUSALS_TRAIN[deepfm]
        for s in bad_histories(seqs, ni):
            refused(texts["train_batch"], lambda: tr.train_batch(s, targets))
            refused(texts["pseudo_targets"], lambda: tr.optimal_pseudo_targets(targets, s))
        for bad in (0, -1, ni):                                                       # a target is a node: the root's children at least, and -1 pads nothing
            refused(texts["pseudo_targets_target"], lambda: tr.optimal_pseudo_targets([[bad]] + targets[1:], seqs))
        if not deepfm:
            rng = np.random.default_rng(3)
            codes = rng.integers(0, NI, 9).astype(np.int32)
            labels = np.ones(9, np.float32)
            for bad in (NI, -2):
                c = codes.copy()
                c[4] = bad
                refused(REFUSALS_ROWS["item"], lambda: eng.train_forward_backward(c, seqs, None, labels))
            for s in bad_histories(seqs, NI):
                refused(REFUSALS_ROWS["history"], lambda: eng.train_forward_backward(codes, s, None, labels))
        assert len(tr.train_batch(seqs, targets)) == leaf - tr.start_level            # the handle still trains
    finally:
        eng.close()


if __name__ == "__main__":
    engines = make_engines()
    np.savez(sys.argv[1], **one_user_results(engines))
    for e_ in engines.values():
        e_.close()
