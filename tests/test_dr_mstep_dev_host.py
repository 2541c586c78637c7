"""Deep-Retrieval M-step path scores on the device, the part that needs no GPU: every case of tests/test_gpu_dr_mstep.py
has the structure it names (checked with the numpy serving oracle in place of the device search), numpy's reduceat is not the sequential
sum, the 64-bit sort key holds what the header says it holds, and header and binding declare the entry points."""
import os
import re

import numpy as np
import pytest

import dr_mstep_cases as cs
from dismember_amd import _native, dr_mstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dismember_amd", "csrc")


@pytest.fixture(scope="module")
def oracle_built():
    from oracle import pyoracle
    pyoracle.build()


def _segs(case):
    beams = cs.oracle_beams(case)
    return beams, cs.segments(case["targets"], case["K"], *beams)


def test_thresholds_are_the_kernels():
    src = open(os.path.join(SRC, "dr_mstep.hip.inc")).read()
    assert int(re.search(r"#define DRM_LANE_MAX (\d+)", src).group(1)) == cs.LANE_MAX
    sort = open(os.path.join(SRC, "dev_sort.hip.inc")).read()
    tb, it = (int(re.search(r"#define %s (\d+)" % n, sort).group(1)) for n in ("DSORT_TB", "DSORT_ITEMS"))
    assert tb * it == cs.TILE


def test_reduceat_is_not_the_sequential_sum():
    """numpy's add.reduceat gives first + sum(rest), and sums the rest with eight accumulators once it has eight or more terms: two terms
    always agree with the left-to-right loop, from three on the last bit can differ (seed 4 of this generator does at three), and on this
    fixed vector the two differ at every length the M-step's long segments have"""
    x = np.random.default_rng(1).random(1000) * 1e-3
    for n, same in ((1, True), (2, True), (8, False), (9, False), (64, False), (129, False), (1000, False)):
        acc = float(x[0])
        for v in x[1:n].tolist():
            acc = acc + v
        assert (acc == float(np.add.reduceat(x[:n], [0])[0])) == same, n
    y = np.random.default_rng(4).random(3) * 1e-3
    assert (float(y[0]) + float(y[1])) + float(y[2]) != float(np.add.reduceat(y, [0])[0])


def test_long_segment_case_structure(oracle_built):
    case = cs.long_segment_case()
    (paths, probs, counts), seg = _segs(case)
    lens = {}
    for (item, _), v in seg.items():
        lens.setdefault(item, set()).add(len(v))
    for i, n in enumerate(cs.SEGMENT_LENGTHS):
        assert lens[i] == {n}                       # one history: each of the item's C paths meets every one of its samples
    for n in (3000, cs.LANE_MAX - 1, cs.LANE_MAX, cs.LANE_MAX + 1, 63, 65, 127, 129):
        assert n in cs.SEGMENT_LENGTHS
    assert max(len(v) for v in seg.values()) >= 8 and cs.sequential_vs_reduceat(seg) > 0
    tg = case["targets"]
    assert (np.diff(np.flatnonzero(tg == 0)) > 1).any()      # the long item's samples are not one contiguous run


def test_short_beam_case_structure(oracle_built):
    case = cs.short_beam_case()
    _, _, counts = cs.oracle_beams(case)
    assert case["K"] ** case["D"] == 4 < case["C"] and (counts == 4).all()


def test_edge_case_structure():
    for name, (N, C) in cs.EDGE_SHAPES.items():
        case = cs.edge_case(name)
        assert N * C == int(name) and len(case["targets"]) == N and case["C"] == C
        assert 0 not in case["targets"] and case["items"] - 1 in case["targets"]
    assert sorted(int(n) for n in cs.EDGE_SHAPES) == [cs.TILE - 1, cs.TILE, cs.TILE + 1, 3 * cs.TILE + 1]


def test_one_item_case_structure(oracle_built):
    case = cs.one_item_case()
    _, seg = _segs(case)
    assert set(case["targets"].tolist()) == {case["items"] - 1}
    assert len(seg) > cs.TILE


def test_tie_case_structure(oracle_built):
    case = cs.tie_case()
    (paths, probs, counts), seg = _segs(case)
    K, D, C = case["K"], case["D"], case["C"]
    twin = {0: 1, 1: 0, 2: 3, 3: 2, 4: 4, 5: 5}
    tied = 0
    for i in range(len(counts)):                    # a beam that holds both twins holds them with the same probability, bit for bit
        beam = {tuple(paths[i, c].tolist()): float(probs[i, c]) for c in range(int(counts[i]))}
        for p, v in beam.items():
            other = (twin[p[0]],) + p[1:]
            if other != p and other in beam:
                assert beam[other] == v, (i, p)
                tied += 1
    assert tied > 0
    want = cs.replay(case["targets"], 10 ** 6, paths, probs, counts)      # the uncut lists
    inside = [v for v, lst in want.items() if len(lst) > C and lst[C - 1][1] == lst[C][1]]
    assert inside                                   # a cut at C falls inside a tie group
    for v in inside:
        assert want[v][C - 1][0] < want[v][C][0]    # ... and keeps the smaller path


def test_few_samples_case_structure():
    case = cs.few_samples_case()
    n = np.bincount(case["targets"]).max()
    assert n <= 7           # the pairwise sum cannot engage ...
    assert n <= 2           # ... and no segment has a third term, from where numpy's first + sum(rest) may leave the left-to-right sum


def test_key_packing_and_refusal_bound():
    """(item << cbits) | code round-trips for the largest key the call accepts; the bound is the header's"""
    hdr = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    assert "ceil(log2 num_item) + ceil(log2 num_node^D) > 63" in hdr and "N * C >= 2^31" in hdr
    ceil_log2 = lambda n: (n - 1).bit_length()
    for num_item, space in ((2 ** 20, 2 ** 43), (2 ** 20 - 5, 2 ** 43 - 1), (2 ** 31 - 1, 2 ** 32), (2, 2 ** 62), (1, 4 * 10 ** 18)):
        ibits, cbits = ceil_log2(num_item), ceil_log2(space)
        assert ibits + cbits <= 63
        top = ((num_item - 1) << cbits) | (space - 1)
        dead = num_item << cbits                      # the key of a slot past a beam's count: item `num_item`, behind every item
        assert top < dead < 2 ** 64
        assert top >> cbits == num_item - 1 and top & ((1 << cbits) - 1) == space - 1
        assert dead.bit_length() <= num_item.bit_length() + cbits <= 64
    assert ceil_log2(2 ** 19 + 1) + ceil_log2(2048 ** 4) == 64      # the model the GPU file is refused with
    src = open(os.path.join(SRC, "dr_mstep.hip.inc")).read()
    assert "drm_ceil_log2(s->num_item) + drm_ceil_log2(space) > 63" in src


def test_header_and_binding_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    for name in ("dm_dr_mstep_path_scores", "dm_dr_mstep_path_scores_dev"):
        assert re.search(r"\bint %s\(" % name, hdr)
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 14
    from dismember_amd import Engine
    assert callable(Engine.dr_mstep_path_scores) and callable(dr_mstep.batch_path_scores_dev)
    import inspect
    assert inspect.signature(dr_mstep.optimize).parameters["path_scores"].default == "host"
