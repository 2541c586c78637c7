"""Device-memory ownership (csrc/dev_mem.hip.inc): every allocation of the library is counted at dm_alloc and at dm_release, so a leak
on any path shows as an exact difference of dm_debug_live_device_allocs.  The counters are the process's own: other tenants of the
card do not move them."""
import ctypes as C
import os

import numpy as np
import pytest

from dismember_amd import Engine
from dismember_amd import _native as N
from helpers import random_din_weights, random_histories, synthetic_tree

pytestmark = pytest.mark.gpu

L = 10
NUM_INDEX = 1023         # a complete tree of depth 9


def live():
    fn = N.lib().dm_debug_live_device_allocs
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    c, b = C.c_ulonglong(0), C.c_ulonglong(0)
    assert fn(C.byref(c), C.byref(b)) == 0
    return int(c.value), int(b.value)


@pytest.fixture(scope="module")
def tree():
    rng = np.random.default_rng(11)
    return synthetic_tree(rng, 9, 300)        # a few hundred items, missing nodes


def make_engine(tree, E, dtype=np.float32, seed=3):
    rng = np.random.default_rng(seed)
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_din(random_din_weights(rng, E, NUM_INDEX, dtype=dtype), E, NUM_INDEX)
    return eng


def p32(a):
    return a.ctypes.data_as(N.i32p)


class Jtm:
    """A small JTM catalogue over the tree's first items: two training rows of L history item ids per item, a gap step from level 6
    to level 8 (every item's current node is its level-6 ancestor).  `bad`: one history id whose leaf code is outside the table."""
    OLD, NEW = 6, 8

    def __init__(self, tree, n_items=40, known=80, bad=None):
        rng = np.random.default_rng(21)
        order = np.argsort(tree["leaf_codes"])
        ids, codes = tree["leaf_ids"][order], tree["leaf_codes"][order].astype(np.int64)
        self.n = n_items
        self.off = (2 * np.arange(n_items + 1)).astype(np.int64)
        self.rows = np.ascontiguousarray(rng.choice(ids[:known], size=(2 * n_items, L)).astype(np.int32))
        if bad is not None:
            self.rows[5, 3] = bad
        c1 = codes[:n_items] + 1
        self.node = np.ascontiguousarray(((c1 >> (9 - self.OLD)) - 1).astype(np.int32))
        self.old = np.ascontiguousarray((((c1 >> (9 - self.NEW)) - 1)).astype(np.int32))
        self.nchild = 1 << (self.NEW - self.OLD)

    def host(self, eng):
        w = np.empty((self.n, self.nchild), np.float32)
        rc = N.lib().dm_jtm_child_weights(eng._h, self.off.ctypes.data_as(N.i64p), p32(self.rows), p32(self.node), self.n, L, self.OLD, self.NEW,
                                          0, 0, 1, w.ctypes.data_as(N.f32p))
        return rc, w

    def cache(self, eng):
        assert N.lib().dm_jtm_cache_rows(eng._h, self.off.ctypes.data_as(N.i64p), p32(self.rows), self.n, L) == 0

    def cached(self, eng):
        w = np.empty((self.n, self.nchild), np.float32)
        rc = N.lib().dm_jtm_child_weights_cached(eng._h, p32(self.node), 0, self.n, self.OLD, self.NEW, 0, 0, 1, w.ctypes.data_as(N.f32p))
        return rc, w

    def step(self, eng):
        out = np.empty(self.n, np.int32)
        rc = N.lib().dm_jtm_step_cached(eng._h, p32(self.node), p32(self.old), self.n, self.OLD, self.NEW, 0, 0, 1, self.n, p32(out))
        return rc, out


def per_call_entry_points(eng, tree, rng_seed=5):
    """the entry points that allocate per call or grow a buffer, each once, on fixed inputs"""
    rng = np.random.default_rng(rng_seed)
    seqs = random_histories(rng, tree["leaf_ids"], 6, L)
    eng.tdm_beam_search(seqs, 8, 5)
    eng.tdm_beam_search_trace(seqs, 8, 5)
    eng.tdm_beam_search(seqs, 8, 5, consumed=[[int(tree["leaf_ids"][0])]] * 6)
    eng.tdm_bruteforce_topk(seqs, 5)
    codes = rng.integers(0, NUM_INDEX, 7).astype(np.int32)
    hist = rng.integers(0, NUM_INDEX, (7, L)).astype(np.int32)
    eng.din_forward(codes, hist, pad_flat_idx=np.array([1, 12, 69], np.int32), L=L)
    labels = (rng.random(7) < 0.5).astype(np.float32)
    eng.train_forward_backward(codes, hist, np.array([3], np.int32), labels)
    eng.adam_step()
    neg = np.zeros(int(tree["max_level"]) + 1, np.int32)
    neg[1:] = 1
    eng.make_train_batch(seqs, tree["leaf_ids"][:6].astype(np.int32), neg, start_level=1, seed=2)
    j = Jtm(tree)
    assert j.host(eng)[0] == 0
    j.cache(eng)
    assert j.cached(eng)[0] == 0
    assert j.step(eng)[0] == 0


def other_handles(tree, path, engines=None):
    """the entry points that live on handles of their own: fp64 OTM search (E = 16), Deep-Retrieval search, checkpoint load"""
    rng = np.random.default_rng(8)
    if engines is None:
        e64 = Engine(0)
        e64.load_weights_din(random_din_weights(rng, 16, 255, dtype=np.float64, std=0.2), 16, 255)
        dr = Engine(0)
        dr.dr_load_model_synthetic(16, 4, 7, 3, 500, seed=1)
        ck = Engine(0)
        engines = (e64, dr, ck)
    e64, dr, ck = engines
    e64.otm_beam_search_f64(np.random.default_rng(1).integers(127, 255, (3, L)).astype(np.int32), 6, 7)
    dr.dr_beam_search(np.random.default_rng(2).integers(0, 500, (3, 4)).astype(np.int32), 5)
    ck.load_model(path)
    return engines


def test_lifecycle_returns_every_byte(tree, tmp_path):
    start = live()
    eng = make_engine(tree, 32)
    assert live()[0] > start[0]
    eng.train_init()
    eng.train_init()                              # a second dm_train_init replaces the first one's buffers
    per_call_entry_points(eng, tree)
    path = os.path.join(str(tmp_path), "m.dmck")
    eng.save_model(path)
    eng.load_model(path)
    clone = eng.clone()
    rng = np.random.default_rng(8)
    clone.tdm_beam_search(random_histories(rng, tree["leaf_ids"], 3, L), 8, 5)
    clone.close()
    for e in other_handles(tree, path):
        e.close()
    eng.close()
    assert live() == start


def test_per_call_paths_leave_nothing(tree, tmp_path):
    eng = make_engine(tree, 32)
    eng.train_init()
    path = os.path.join(str(tmp_path), "m.dmck")
    eng.save_model(path)
    per_call_entry_points(eng, tree)              # warm-up: the grow-only buffers reach their size
    others = other_handles(tree, path)
    before = live()
    for _ in range(5):
        per_call_entry_points(eng, tree)
        other_handles(tree, path, others)
    assert live() == before
    for e in others:
        e.close()
    eng.close()


def test_jtm_refusals_after_allocation(tree):
    """DM_ERR_INDEX of dm_jtm_child_weights is reported after the device pass, with every temporary allocated: the refusal must leave
    what a successful call leaves, the handle's cached catalogue must survive it, and the next call's weights must not move."""
    rng = np.random.default_rng(4)
    eng = Engine(0)
    eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], int(tree["max_level"]))
    eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
    eng.load_weights_din(random_din_weights(rng, 32, 600), 32, 600)      # a table that ends inside the leaf level: codes 511 .. 599 are in it
    far = int(tree["leaf_ids"][np.argmax(tree["leaf_codes"])])            # leaf code 810: outside
    good, bad = Jtm(tree), Jtm(tree, bad=far)
    # from host rows
    rc, w0 = good.host(eng)
    assert rc == 0
    ok = live()
    rc, _ = bad.host(eng)
    assert rc == -4 and live() == ok
    rc, w1 = good.host(eng)
    assert rc == 0 and live() == ok and w1.tobytes() == w0.tobytes()
    # cached, and the fused gap step: the per-row code cache is dropped by the refusal, so compare after the next successful call
    for call in (Jtm.cached, Jtm.step):
        good.cache(eng)
        rc, r0 = call(good, eng)
        assert rc == 0
        ok = live()
        bad.cache(eng)
        rc, _ = call(bad, eng)
        assert rc == -4
        rc, _ = call(bad, eng)
        assert rc == -4                           # (a retry reports the same error: the cache was not kept with the bad position cleared)
        good.cache(eng)
        rc, r1 = call(good, eng)
        assert rc == 0 and live() == ok and r1.tobytes() == r0.tobytes()
    eng.close()


def up(v):
    return (v + 255) & ~255


def grown(need, div):
    return need + need // div


def test_grow_only_buffers(tree):
    """Request, then one twice as large, then the first again: the count never moves, bytes rise once, by what the slack table says.
    The search workspace and the deferred-user list depend on the launch plan, so they are brought to the large request's size first,
    through the device-buffer entry point (same users, same plan, no request arena); what then grows is the request arena alone:
    [seq | ids | scores | counts] in 256-byte steps, by half again."""
    eng = make_engine(tree, 32)
    rng = np.random.default_rng(9)
    U1, U2, topk = 40, 80, 5
    small = random_histories(rng, tree["leaf_ids"], U1, L)
    large = random_histories(rng, tree["leaf_ids"], U2, L)
    d = [eng.dev_alloc(n) for n in (U2 * L * 4, U2 * topk * 4, U2 * topk * 4, U2 * 4)]
    eng.h2d(d[0], large)
    eng.tdm_beam_search_dev(d[0], U2, L, 8, topk, d[1], d[2], d[3])
    eng.synchronize()
    for q in d:
        eng.dev_free(q)

    def req_need(U):
        return up(U * L * 4) + 2 * up(U * topk * 4) + up(U * 4)

    c0, b0 = live()
    eng.tdm_beam_search(small, 8, topk)
    c1, b1 = live()
    assert (c1, b1) == (c0 + 1, b0 + grown(req_need(U1), 2))
    eng.tdm_beam_search(large, 8, topk)
    c2, b2 = live()
    assert c2 == c1 and b2 - b1 == grown(req_need(U2), 2) - grown(req_need(U1), 2)
    eng.tdm_beam_search(small, 8, topk)
    assert live() == (c2, b2)
    eng.tdm_beam_search(large, 8, topk)
    assert live() == (c2, b2)                     # no allocation once the handle has seen its largest request
    # the sampler's per-call block [neg | lvl_off | tcode | cnt | row_off], by half again
    nl = int(tree["max_level"]) + 1
    neg = np.zeros(nl, np.int32)
    neg[1:] = 1

    def samp_need(T):
        return up(nl * 4) + up((nl + 1) * 4) + up(T * 4 + 4) + up(T * 8 + 8) + up((T + 1) * 8)

    def sample(T):
        eng.make_train_batch(random_histories(rng, tree["leaf_ids"], T, L), rng.choice(tree["leaf_ids"], T).astype(np.int32), neg, start_level=1, seed=2)

    sample(30)
    c3, b3 = live()
    assert (c3, b3) == (c2 + 1, b2 + grown(samp_need(30), 2))
    sample(300)
    assert live() == (c3, b3 + grown(samp_need(300), 2) - grown(samp_need(30), 2))
    sample(30)
    assert live() == (c3, b3 + grown(samp_need(300), 2) - grown(samp_need(30), 2))
    eng.close()
