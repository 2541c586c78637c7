"""TEST INFRASTRUCTURE — the inputs of the Deep-Retrieval M-step path-score tests, shared by the GPU file
(test_gpu_dr_mstep.py) and the CPU file that checks each case has the structure it names (test_dr_mstep_dev_host.py), and the
replay of the aggregation on given beams with oracle/dr_mstep_oracle.py (its Python loop is the sequential fold)."""
import numpy as np

from dismember_amd import dr_mstep, synth
from oracle import dr_mstep_oracle as mo

LANE_MAX = 32          # DRM_LANE_MAX of csrc/dr_mstep.hip.inc: a longer segment is summed by a wave (the CPU file pins the two together)
TILE = 4096            # DSORT_TILE of csrc/dev_sort.hip.inc


def _seqs(rng, N, L, items, pad=0.2):
    s = rng.integers(0, items, size=(N, L)).astype(np.int32)
    s[rng.random((N, L)) < pad] = -1
    return s


def model_case(K, D, L, E, items, N, C, seed=4, scale=0.3):
    """ordinary samples: random histories, targets on the lower half of the items"""
    rng = np.random.default_rng(seed)
    w = synth.make_dr_model(items, K, D, L, E, rng, scale=scale)
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=_seqs(rng, N, L, items),
                targets=rng.integers(0, max(items // 2, 1), size=N).astype(np.int32))


# (K, D, L, E, items, N, C): the existing M-step test's shape, the layer counts the loader takes, one candidate, and both sides of the
# one-wave cut of the sliced search (64)
REPLAY_SHAPES = {
    "base": (8, 3, 5, 16, 120, 300, 6),
    "D2": (8, 2, 5, 16, 120, 300, 6),
    "D4": (6, 4, 5, 16, 120, 300, 6),
    "C1": (8, 3, 5, 16, 120, 300, 1),
    "C64": (8, 3, 5, 16, 120, 300, 64),
    "C65": (8, 3, 5, 16, 120, 300, 65),
}


def short_beam_case():
    """K^D = 4 < C = 8: every beam holds 4 paths"""
    return model_case(2, 2, 5, 16, 60, 200, 8, seed=7)


SEGMENT_LENGTHS = [3000, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 63, 64, 65, 127, 128, 129]


def long_segment_case():
    """item i < len(SEGMENT_LENGTHS) gets SEGMENT_LENGTHS[i] samples of ONE history (its own): each of its paths is a segment of exactly
    that length; ordinary items follow.  The groups are interleaved with the ordinary samples, not laid out one after the other."""
    K, D, L, E, items, C = 8, 3, 5, 16, 80, 4
    rng = np.random.default_rng(11)
    w = synth.make_dr_model(items, K, D, L, E, rng)
    hist = _seqs(rng, len(SEGMENT_LENGTHS), L, items, pad=0.0)
    seqs = [np.repeat(hist[i:i + 1], n, axis=0) for i, n in enumerate(SEGMENT_LENGTHS)]
    tg = [np.full(n, i, np.int32) for i, n in enumerate(SEGMENT_LENGTHS)]
    n_ord = 200
    seqs.append(_seqs(rng, n_ord, L, items))
    tg.append(rng.integers(len(SEGMENT_LENGTHS), items, size=n_ord).astype(np.int32))
    seqs, tg = np.concatenate(seqs), np.concatenate(tg)
    order = rng.permutation(len(tg))
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=np.ascontiguousarray(seqs[order]), targets=np.ascontiguousarray(tg[order]))


# N * C on both sides of the sort's tile and past three tiles (12 289 is prime: one candidate per sample)
EDGE_SHAPES = {"4095": (819, 5), "4096": (1024, 4), "4097": (241, 17), "12289": (12289, 1)}


def edge_case(name):
    """item 0 is never a target, the highest id is"""
    N, C = EDGE_SHAPES[name]
    K, D, L, E, items = 8, 3, 5, 16, 97
    rng = np.random.default_rng(100 + N)
    w = synth.make_dr_model(items, K, D, L, E, rng)
    tg = rng.integers(1, items, size=N).astype(np.int32)
    tg[N // 2] = items - 1
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=_seqs(rng, N, L, items), targets=tg)


def one_item_case():
    """every sample on the highest item, which collects more than 4 096 distinct paths (segments): more than a tile of one item"""
    K, D, L, E, items, N, C = 32, 3, 5, 16, 50, 1100, 16
    rng = np.random.default_rng(21)
    w = synth.make_dr_model(items, K, D, L, E, rng, scale=0.6)
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=_seqs(rng, N, L, items), targets=np.full(N, items - 1, np.int32))


def tie_case():
    """K = 6 with layer-0 nodes 0 = 1 and 2 = 3 (4 and 5 stay single): the same W_0 row and bias, and the same node embedding for the layers
    that follow, so the paths (0, x, y) / (1, x, y) and (2, x, y) / (3, x, y) score alike for every history.  Pairs and singles mix in an
    item's list, so for some items the cut at C falls inside a tie group (test_dr_mstep_dev_host.py checks that it does)"""
    K, D, L, E, items, N, C = 6, 3, 5, 16, 40, 300, 7
    rng = np.random.default_rng(31)
    w = synth.make_dr_model(items, K, D, L, E, rng)
    for a, b in ((0, 1), (2, 3)):
        w["layer_w"][0][b] = w["layer_w"][0][a]
        w["layer_b"][0][b] = w["layer_b"][0][a]
        w["layer_emb"][items + b] = w["layer_emb"][items + a]
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=_seqs(rng, N, L, items), targets=rng.integers(0, 12, size=N).astype(np.int32))


def few_samples_case():
    """at most 2 samples per item (so at most 7): the host route's reduceat cannot sum pairwise, and no segment has the third term from
    which its first + sum(rest) can leave the left-to-right sum (test_dr_mstep_dev_host.py): both routes give the same bytes"""
    K, D, L, E, items, C = 8, 3, 5, 16, 120, 6
    rng = np.random.default_rng(41)
    w = synth.make_dr_model(items, K, D, L, E, rng)
    tg = np.repeat(np.arange(60, dtype=np.int32), rng.integers(1, 3, size=60))
    rng.shuffle(tg)
    return dict(K=K, D=D, L=L, E=E, items=items, C=C, w=w, seqs=_seqs(rng, len(tg), L, items), targets=tg)


# ---- replay
def oracle_beams(case):
    """the numpy serving oracle's beams in the layout of a trace: paths [N, C, D] (-1 past the count), probs [N, C], counts [N]"""
    from oracle import pyoracle as po
    orc = po.DeepRetrieval(case["w"], case["E"], case["L"], case["K"], case["D"], case["items"])
    N, C, D = len(case["seqs"]), case["C"], case["D"]
    paths, probs, counts = np.full((N, C, D), -1, np.int32), np.zeros((N, C)), np.zeros(N, np.int32)
    for i in range(N):
        p, v = orc.beam_search(case["seqs"][i], C)
        counts[i] = len(v)
        paths[i, :len(v)], probs[i, :len(v)] = p, v
    return paths, probs, counts


def replay(targets, C, paths, probs, counts):
    """oracle.dr_mstep_oracle.batch_path_score on given beams -> {item: [(path tuple, score)]}"""
    pl, vl = paths.tolist(), probs.tolist()

    def bs(i, beam):
        return [(tuple(pl[i][c]), vl[i][c]) for c in range(int(counts[i]))]
    return mo.batch_path_score([(i, int(t)) for i, t in enumerate(np.asarray(targets).tolist())], bs, C)


def segments(targets, K, paths, probs, counts):
    """{(item, code): [probabilities in sample order]}"""
    codes = dr_mstep._codes(paths.astype(np.int64), K)
    seg = {}
    for i, t in enumerate(np.asarray(targets).tolist()):
        for c in range(int(counts[i])):
            seg.setdefault((t, int(codes[i, c])), []).append(float(probs[i, c]))
    return seg


def sequential_vs_reduceat(seg):
    """number of segments on which the left-to-right sum and numpy's reduceat differ"""
    n = 0
    for v in seg.values():
        acc = v[0]
        for x in v[1:]:
            acc = acc + x
        n += acc != float(np.add.reduceat(np.asarray(v), [0])[0])
    return n


def assert_result_is_replay(result, case, paths, probs, counts):
    """codes, their order, offsets, occurrences and scores (==, no tolerance) against the replay of the given beams"""
    off, codes, scores, occ = result[:4]
    items, C, K, D = case["items"], case["C"], case["K"], case["D"]
    want = replay(case["targets"], C, paths, probs, counts)
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
