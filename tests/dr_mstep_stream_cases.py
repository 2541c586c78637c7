"""TEST INFRASTRUCTURE — the inputs of the streaming M-step tests, shared by the GPU file (test_gpu_dr_mstep_stream.py) and
the CPU file that checks each case has the structure it names (test_dr_mstep_stream_host.py), and the replay of the fold on given beams
with oracle/dr_mstep_oracle.streaming_path_score (its Python loop is the sequential merge).  Cases of tests/dr_mstep_cases.py are used
as they are where they serve."""
from fractions import Fraction

import numpy as np

import dr_mstep_cases as cs
from dismember_amd import dr_mstep, synth
from oracle import dr_mstep_oracle as mo

WAVE_C = 32            # DMS_WAVE_C of csrc/dr_mstep_stream.hip.inc: up to this C a wave folds an item, above it a workgroup
BOUNDARY_C = (31, 32, 33)


def boundary_case(C):
    return cs.model_case(8, 3, 5, 16, 120, 300, C)


def long_chain_case(n=3000):
    """item 3 gets n samples of ONE history: after the first, every merge meets the list's own codes ("in both"); ordinary samples on
    other items lie in between"""
    K, D, L, E, items, C = 8, 3, 5, 16, 80, 6
    rng = np.random.default_rng(51)
    w = synth.make_dr_model(items, K, D, L, E, rng)
    hist = cs._seqs(rng, 1, L, items, pad=0.0)
    n_ord = 200
    seqs = np.concatenate([np.repeat(hist, n, axis=0), cs._seqs(rng, n_ord, L, items)])
    tg = np.concatenate([np.full(n, 3, np.int32), rng.integers(4, items, size=n_ord).astype(np.int32)])
    order = rng.permutation(len(tg))
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=np.ascontiguousarray(seqs[order]), targets=np.ascontiguousarray(tg[order]), long_item=3)


def alternating_case(n=40):
    """item 5's samples alternate between two histories whose beams share no path (the two are searched for with the numpy oracle among
    random histories; the GPU file checks the disjointness on its own trace): every merge is beam-only or list-only"""
    K, D, L, E, items, C = 8, 3, 5, 16, 80, 4
    rng = np.random.default_rng(61)
    w = synth.make_dr_model(items, K, D, L, E, rng, scale=0.6)
    pool = cs._seqs(rng, 24, L, items, pad=0.0)
    paths, _, counts = cs.oracle_beams(dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=pool))
    sets = [set(map(tuple, paths[i, :counts[i]].tolist())) for i in range(len(pool))]
    pair = next((i, j) for i in range(len(pool)) for j in range(i + 1, len(pool)) if not (sets[i] & sets[j]))
    alt = np.stack([pool[pair[k % 2]] for k in range(n)])
    n_ord = 100
    seqs = np.concatenate([alt, cs._seqs(rng, n_ord, L, items)])
    tg = np.concatenate([np.full(n, 5, np.int32), rng.integers(6, items, size=n_ord).astype(np.int32)])
    # (the alternation needs the chain's own order: ordinary samples go in between without permuting the chain)
    pos = np.sort(rng.choice(n + n_ord, size=n, replace=False))
    order = np.full(n + n_ord, -1, np.int64)
    order[pos] = np.arange(n)
    order[order < 0] = n + np.arange(n_ord)
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=np.ascontiguousarray(seqs[order]), targets=np.ascontiguousarray(tg[order]), alt_item=5)


def queue_case(n_items=5000, n_long=2000):
    """items 1 .. n_items with 1 to 3 samples each and item 0 with n_long: many more chains than resident workers, one far longer than the
    rest.  The histories come from a pool of 64, so that the CPU file needs 64 oracle searches"""
    K, D, L, E, C = 8, 3, 5, 16, 4
    items = n_items + 1
    rng = np.random.default_rng(71)
    w = synth.make_dr_model(items, K, D, L, E, rng)
    pool = cs._seqs(rng, 64, L, items)
    tg = np.concatenate([np.zeros(n_long, np.int32), np.repeat(np.arange(1, items, dtype=np.int32), rng.integers(1, 4, size=n_items))])
    rng.shuffle(tg)
    seqs = pool[rng.integers(0, len(pool), size=len(tg))]
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=np.ascontiguousarray(seqs), targets=tg)


def contraction_case(n=400, C=8, pool=12, seed=81):
    """canned beams of random doubles on one item: n - 1 merges, most codes met again, so a fused multiply-add would show (one product-sum
    in about six rounds differently when it is rounded once)"""
    rng = np.random.default_rng(seed)
    K, D = 8, 2
    codes = np.stack([rng.permutation(pool)[:C] for _ in range(n)])
    paths = np.stack([codes // K, codes % K], axis=-1).astype(np.int32)
    probs = rng.random((n, C))
    return dict(K=K, D=D, L=1, items=2, C=C, seqs=np.zeros((n, 1), np.int32), targets=np.ones(n, np.int32)), (paths, probs, np.full(n, C, np.int32))


# ---- beams
def oracle_beams_unique(case):
    """cs.oracle_beams, searching every distinct history once"""
    uniq, inv = np.unique(case["seqs"], axis=0, return_inverse=True)
    p, v, c = cs.oracle_beams(dict(case, seqs=uniq))
    inv = inv.reshape(-1)
    return p[inv], v[inv], c[inv]


class CannedEngine:
    """stands in for an Engine in dr_mstep.streaming_path_scores: dr_dims and a dr_beam_search that returns the given beams"""

    def __init__(self, case, beams):
        self.dr_dims = dict(K=case["K"], D=case["D"], L=case["L"], num_item=case["items"])
        self.beams, self.at = beams, 0

    def dr_beam_search(self, seqs, beam):
        o, n = self.at, len(seqs)
        self.at += n
        assert beam == self.beams[0].shape[1] and o + n <= len(self.beams[0])
        return tuple(a[o:o + n] for a in self.beams)


# ---- replay
def replay(targets, C, decay, paths, probs, counts, batch_size=8192):
    """oracle.dr_mstep_oracle.streaming_path_score on given beams -> {item: [(path tuple, score)]}: the samples are (i, target_i) and the
    beam function hands out sample i's beam"""
    pl, vl = paths.tolist(), probs.tolist()

    def bs(i, beam):
        return [(tuple(pl[i][c]), vl[i][c]) for c in range(int(counts[i]))]
    return mo.streaming_path_score([(i, int(t)) for i, t in enumerate(np.asarray(targets).tolist())], bs, C, decay, batch_size)


def assert_result_is_replay(result, case, decay, paths, probs, counts):
    """codes, their order, offsets, occurrences and scores (==, no tolerance) against the replay of the given beams"""
    off, codes, scores, occ = result[:4]
    items, C, K, D = case["items"], case["C"], case["K"], case["D"]
    want = replay(case["targets"], C, decay, paths, probs, counts)
    assert off.shape == (items + 1,) and off[0] == 0 and off[-1] == len(codes) == len(scores)
    assert (np.diff(off) >= 0).all() and (np.diff(off) <= C).all()
    assert occ.tolist() == np.bincount(case["targets"], minlength=items).tolist()
    assert set(np.flatnonzero(np.diff(off)).tolist()) == set(want)
    for v, lst in want.items():
        got_c = codes[off[v]:off[v + 1]].tolist()
        got_s = scores[off[v]:off[v + 1]].tolist()
        assert [dr_mstep._decode(c, K, D) for c in got_c] == [p for p, _ in lst], v
        assert [s.hex() for s in got_s] == [float(s).hex() for _, s in lst], v
    return want


def assert_dicts_equal(got, want, K, D):
    """{item: (codes, scores)} of dr_mstep.streaming_path_scores[_dev] against a replay's {item: [(path, score)]}"""
    assert set(got) == set(want)
    for v, lst in want.items():
        assert [dr_mstep._decode(c, K, D) for c in got[v][0].tolist()] == [p for p, _ in lst], v
        assert [s.hex() for s in got[v][1].tolist()] == [float(s).hex() for _, s in lst], v


def merge_stats(targets, C, decay, paths, probs, counts, K):
    """what the merges of a call look like: the chain length per item; over all merges the largest union, the numbers of beam-only codes,
    of list-only codes and of codes in both, and the number of merges whose cut at C falls inside a group of equal scores (entries C - 1
    and C of the uncut union score alike)"""
    codes = dr_mstep._codes(paths.astype(np.int64), K)
    state, out = {}, dict(chain={}, max_union=0, beam_only=0, list_only=0, both=0, cut_in_tie=0)
    for i, t in enumerate(np.asarray(targets).tolist()):
        beam = {int(codes[i, c]): float(probs[i, c]) for c in range(int(counts[i]))}
        out["chain"][t] = out["chain"].get(t, 0) + 1
        if t not in state:
            state[t] = list(beam.items())
            continue
        old = dict(state[t])
        m = min(old.values())
        out["max_union"] = max(out["max_union"], len(set(old) | set(beam)))
        out["beam_only"] += len(set(beam) - set(old))
        out["list_only"] += len(set(old) - set(beam))
        out["both"] += len(set(old) & set(beam))
        new = [(u, (decay * old[u] + beam[u]) if (u in old and u in beam) else (decay * m + beam[u] if u in beam else decay * old[u])) for u in sorted(set(old) | set(beam))]
        new = sorted(new, key=lambda x: -x[1])
        out["cut_in_tie"] += len(new) > C and new[C - 1][1] == new[C][1]
        state[t] = new[:C]
    return out


def tied_neighbours(want):
    """number of neighbours with equal scores in the lists of a replay (items of one sample left out: their list is a beam as it stands);
    asserts that such neighbours ascend by path"""
    n = 0
    for lst in want.values():
        for (p0, s0), (p1, s1) in zip(lst[:-1], lst[1:]):
            if s0 == s1 and sorted(lst, key=lambda t: -t[1]) == lst:
                assert p0 < p1
                n += 1
    return n


def fold_one_item(C, decay, paths, probs, counts, K, fused):
    """the fold of ONE item's samples in the given order -> [(code, score)]; fused: every product-sum rounded once, as a contracted
    multiply-add would (exact rational arithmetic, one conversion)"""
    codes = dr_mstep._codes(paths.astype(np.int64), K)
    if fused:
        fma = lambda d, o, c: float(Fraction(d) * Fraction(o) + Fraction(c))
    else:
        fma = lambda d, o, c: d * o + c
    state = None
    for i in range(len(counts)):
        beam = {int(codes[i, c]): float(probs[i, c]) for c in range(int(counts[i]))}
        if state is None:
            state = list(beam.items())
            continue
        old = dict(state)
        m = min(old.values())
        new = [(u, fma(decay, old[u], beam[u]) if (u in old and u in beam) else (fma(decay, m, beam[u]) if u in beam else decay * old[u])) for u in sorted(set(old) | set(beam))]
        state = sorted(new, key=lambda x: -x[1])[:C]
    return state
