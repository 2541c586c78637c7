"""TEST INFRASTRUCTURE — synthetic per-item CSRs for the path assignment of the Deep-Retrieval M-step: the shapes
tests/test_gpu_dr_assign.py runs on the device; tests/test_dr_assign_host.py checks that each has the structure it names and which of
them are "exact" (every decision of the reference trajectory is won by more than 8 tolerances).  A case is a dict: off, codes, scores, occ
(the CSR), K, D (num_node, num_layer), J, T, pf, p.  Scores are sums of probabilities: positive, at most the item's occurrence."""
import numpy as np

import dr_assign_ref as ref

K, D = 64, 3                     # 262 144 path codes


def build(lists, occ, J, T=3, pf=3e-6, p=4, K_=K, D_=D):
    """lists: per item a list of (code, score) (empty for an item without candidates); occ: per item its occurrence"""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    codes = np.array([c for l in lists for c, _ in l], np.int64)
    scores = np.array([s for l in lists for _, s in l], np.float64)
    return dict(off=off, codes=codes, scores=scores, occ=np.asarray(occ, np.int64), K=K_, D=D_, J=J, T=T, pf=pf, p=p)


def _list(rng, c, nv, pool):
    """c distinct codes of the pool with distinct scores in (0, nv), descending as the path-score routes hand them out"""
    codes = rng.choice(pool, size=c, replace=False)
    scores = np.sort(rng.uniform(0.02, 1.0, size=c) * nv)[::-1]
    return list(zip(codes.tolist(), scores.tolist()))


def generic(seed, n_items, c, J, pool_size, **kw):
    rng = np.random.default_rng(seed)
    pool = rng.choice(K ** D, size=pool_size, replace=False)
    occ = rng.integers(1, 6, size=n_items)
    return build([_list(rng, c, int(nv), pool) for nv in occ], occ, J, **kw)


def shared_case():
    """every item lists the same candidates in the same order: item i + 1 reads the words item i has just changed"""
    rng = np.random.default_rng(11)
    codes = rng.choice(K ** D, size=8, replace=False).tolist()
    occ = rng.integers(1, 4, size=40)
    lists = [list(zip(codes, np.sort(rng.uniform(0.1, 0.9, size=8) * nv)[::-1].tolist())) for nv in occ]
    return build(lists, occ, 3, pf=0.05, p=2)


def alternating_case():
    rng = np.random.default_rng(12)
    pools = [rng.choice(K ** D // 2, size=6, replace=False), K ** D // 2 + rng.choice(K ** D // 2, size=6, replace=False)]
    occ = rng.integers(1, 4, size=30)
    lists = [list(zip(pools[i & 1].tolist(), np.sort(rng.uniform(0.1, 0.9, size=6) * nv)[::-1].tolist())) for i, nv in enumerate(occ)]
    return build(lists, occ, 2, pf=0.05, p=2)


def crowd_case():
    """one path leads the list of 300 items; the penalty grows until the choice moves off it"""
    rng = np.random.default_rng(13)
    pool = rng.choice(np.arange(1, K ** D), size=2000, replace=False)
    lists = []
    for _ in range(300):
        rest = _list(rng, 4, 0.5, pool)
        lists.append([(0, float(rng.uniform(0.8, 0.9)))] + rest)
    return build(lists, np.ones(300, np.int64), 2, pf=1e-3, p=4)


def tie_case():
    """bit-equal scores inside an item, on paths of equal size: the first maximum wins"""
    rng = np.random.default_rng(14)
    lists = []
    for i in range(12):
        codes = (1000 * i + np.arange(6)).tolist()
        s = rng.uniform(0.2, 0.8)
        lists.append(list(zip(codes, [s, s, s, 0.5 * s, 0.5 * s, 0.25 * s])))
    return build(lists, np.full(12, 2, np.int64), 3)


def sparse_case():
    """hit items separated by long runs of unhit ones; the first and the last item are hit"""
    rng = np.random.default_rng(15)
    n = 5000
    pool = rng.choice(K ** D, size=40, replace=False)
    occ = np.zeros(n, np.int64)
    lists = [[] for _ in range(n)]
    for v in (0, 1700, 1701, 4999):
        occ[v] = int(rng.integers(1, 5))
        lists[v] = _list(rng, 7, int(occ[v]), pool)
    return build(lists, occ, 3, pf=0.02, p=2)


def stop_case():
    """item 3 is the first whose accumulated gain reaches -1: the penalty of an empty path alone is 100"""
    c = generic(16, 6, 4, 2, 30, pf=100.0, p=1)
    c["occ"][:3] = 0
    return c


CASES = {
    "c1_j1": lambda: generic(1, 5, 1, 1, 3),
    "j_eq_c": lambda: generic(2, 6, 4, 4, 9, pf=0.05, p=2),
    "C63": lambda: generic(3, 4, 63, 3, 100, pf=0.01, p=2),
    "C64": lambda: generic(4, 4, 64, 3, 100, pf=0.01, p=2),
    "C65": lambda: generic(5, 4, 65, 3, 100, pf=0.01, p=2),
    "C130": lambda: generic(6, 4, 130, 3, 200, pf=0.01, p=2),
    "C2048": lambda: generic(7, 3, 2048, 3, 3000, pf=0.01, p=2),
    "T1": lambda: generic(8, 20, 20, 3, 60, T=1, pf=0.02, p=2),
    "p1": lambda: generic(8, 20, 20, 3, 60, pf=0.02, p=1),
    "p4": lambda: generic(8, 20, 20, 3, 60, pf=1e-3, p=4),
    "pf0": lambda: generic(8, 20, 20, 3, 60, pf=0.0),
    "shared": shared_case,
    "alternating": alternating_case,
    "crowd": crowd_case,
    "tie": tie_case,
    "sparse": sparse_case,
    "hit1": lambda: generic(9, 1, 20, 3, 60),
    "hit2": lambda: generic(10, 2, 20, 3, 30, pf=0.02, p=2),
    "hit257": lambda: generic(17, 257, 20, 3, 400, pf=0.02, p=2),
}
NOT_EXACT = ("tie",)                 # decided by position, not by margin: judged by the replay alone
_cache = {}


def get(name):
    """(case, assign_ref(case)): built once, shared, left unchanged"""
    if name not in _cache:
        case = CASES[name]()
        _cache[name] = (case, ref.assign_ref(case))
    return _cache[name]
