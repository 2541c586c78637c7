"""Streaming M-step on the device, the part that needs no GPU: the host mirror dr_mstep.streaming_path_scores equals
oracle/dr_mstep_oracle.streaming_path_score bit for bit on every case's canned beams (the numpy serving oracle's, handed out by a
stand-in engine) — so the GPU file's two yardsticks are one; every case of tests/test_gpu_dr_mstep_stream.py has the structure it names;
the contraction case would show a fused multiply-add; header, binding and generated shim declare the entry points."""
import inspect
import os
import re

import numpy as np
import pytest

import dr_mstep_cases as cs
import dr_mstep_stream_cases as sc
from dismember_amd import _native, dr_mstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dismember_amd", "csrc")

CASES = dict([(n, lambda n=n: cs.model_case(*cs.REPLAY_SHAPES[n])) for n in cs.REPLAY_SHAPES] +
             [("C%d" % c, lambda c=c: sc.boundary_case(c)) for c in sc.BOUNDARY_C] +
             [("short", cs.short_beam_case), ("edge", lambda: cs.edge_case("4095")), ("long", sc.long_chain_case), ("alternating", sc.alternating_case),
              ("tie", cs.tie_case), ("queue", sc.queue_case), ("few", cs.few_samples_case)])
_cache = {}


@pytest.fixture(scope="module")
def oracle_built():
    from oracle import pyoracle
    pyoracle.build()


def _beams(name):
    """(case, the numpy oracle's beams): computed once, shared, left unchanged"""
    if name not in _cache:
        case = CASES[name]()
        _cache[name] = (case, sc.oracle_beams_unique(case))
    return _cache[name]


def _mirror(case, beams, decay, **kw):
    eng = sc.CannedEngine(case, beams)
    got = dr_mstep.streaming_path_scores(eng, case["seqs"], case["targets"], case["C"], decay, **kw)
    assert eng.at == len(case["seqs"])
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_mirror_is_the_oracle(oracle_built, name):
    case, beams = _beams(name)
    for decay in ((0.999, 0.5, 1.0, 0.0) if name in ("base", "tie") else (0.999,)):
        want = sc.replay(case["targets"], case["C"], decay, *beams)
        sc.assert_dicts_equal(_mirror(case, beams, decay), want, case["K"], case["D"])
    if name == "base":          # the mini-batches of the reference do not enter the result
        sc.assert_dicts_equal(_mirror(case, beams, 0.999, batch_size=7), sc.replay(case["targets"], case["C"], 0.999, *beams, batch_size=7), case["K"], case["D"])
        sc.assert_dicts_equal(_mirror(case, beams, 0.999, batch_size=7), sc.replay(case["targets"], case["C"], 0.999, *beams), case["K"], case["D"])


def test_threshold_is_the_kernels():
    src = open(os.path.join(SRC, "dr_mstep_stream.hip.inc")).read()
    assert int(re.search(r"#define DMS_WAVE_C (\d+)", src).group(1)) == sc.WAVE_C
    assert sc.BOUNDARY_C == (sc.WAVE_C - 1, sc.WAVE_C, sc.WAVE_C + 1)
    assert "#pragma clang fp contract(off)" in src and "CoordinateDescent.scala:162-212" in src


def test_base_case_structure(oracle_built):
    case, beams = _beams("base")
    st = sc.merge_stats(case["targets"], case["C"], 0.999, *beams, case["K"])
    assert st["max_union"] > case["C"]                   # a merge whose union exceeds C: the cut does something
    assert st["beam_only"] > 0 and st["list_only"] > 0 and st["both"] > 0      # decay * m is used, and the other two forms
    lens = set(st["chain"].values())
    assert 1 in lens and 2 in lens and max(lens) >= 5    # an item with exactly one sample, one with two, longer chains


def test_boundary_cases_structure(oracle_built):
    for c in sc.BOUNDARY_C:
        case, beams = _beams("C%d" % c)
        assert case["C"] == c and (beams[2] == c).all()
        st = sc.merge_stats(case["targets"], c, 0.999, *beams, case["K"])
        assert c < st["max_union"] <= 2 * c and st["beam_only"] > 0 and st["both"] > 0
    case, beams = _beams("C65")
    assert (beams[2] == 65).all() and sc.merge_stats(case["targets"], 65, 0.999, *beams, case["K"])["max_union"] > 65


def test_short_beam_case_structure(oracle_built):
    case, beams = _beams("short")
    st = sc.merge_stats(case["targets"], case["C"], 0.999, *beams, case["K"])
    assert (beams[2] == 4).all() and st["max_union"] == 4 < case["C"]      # the lists never fill
    assert st["beam_only"] == 0 and st["list_only"] == 0 and st["both"] > 0


def test_edge_case_structure():
    case = cs.edge_case("4095")
    assert 0 not in case["targets"] and case["items"] - 1 in case["targets"]


def test_long_chain_case_structure(oracle_built):
    case, beams = _beams("long")
    v = case["long_item"]
    idx = np.flatnonzero(case["targets"] == v)
    assert len(idx) == 3000 and (np.diff(idx) > 1).any() and len(np.unique(case["seqs"][idx], axis=0)) == 1
    only = [a[idx] for a in beams]
    st = sc.merge_stats(np.full(len(idx), v), case["C"], 0.999, *only, case["K"])
    assert st["both"] == 2999 * case["C"] and st["beam_only"] == 0 and st["list_only"] == 0 and st["max_union"] == case["C"]


def test_alternating_case_structure(oracle_built):
    case, beams = _beams("alternating")
    v = case["alt_item"]
    idx = np.flatnonzero(case["targets"] == v)
    assert len(idx) == 40 and (np.diff(idx) > 1).any()
    only = [a[idx] for a in beams]
    a, b = (set(map(tuple, only[0][k, :only[2][k]].tolist())) for k in (0, 1))
    assert len(a) == len(b) == case["C"] and not (a & b)
    st = sc.merge_stats(np.full(len(idx), v), case["C"], 0.999, *only, case["K"])
    # the first merge: C beam-only, C list-only; from then on the list holds the C best of both beams, each beam meets some of them
    assert st["max_union"] == 2 * case["C"] and st["beam_only"] >= case["C"] and st["list_only"] >= case["C"]


def test_tie_case_structure(oracle_built):
    case, beams = _beams("tie")
    assert sc.merge_stats(case["targets"], case["C"], 1.0, *beams, case["K"])["cut_in_tie"] > 0      # a cut falls inside a tie group
    # decay 0: what only the list held scores +0 and falls behind the full beam, so no cut can split a tie; the list is the last beam by
    # (score descending, path ascending), and the twins inside it are the ties
    assert (beams[2] == case["C"]).all() and sc.merge_stats(case["targets"], case["C"], 0.0, *beams, case["K"])["cut_in_tie"] == 0
    for decay in (1.0, 0.0):
        assert sc.tied_neighbours(sc.replay(case["targets"], case["C"], decay, *beams)) > 0


def test_queue_case_structure():
    case = sc.queue_case()
    n = np.bincount(case["targets"], minlength=case["items"])
    assert n[0] == 2000 and n[1:].min() == 1 and n[1:].max() == 3 and len(n) == 5001
    assert len(np.unique(case["seqs"], axis=0)) <= 64


def test_contraction_case_is_sensitive_to_fusion():
    case, beams = sc.contraction_case()
    got = _mirror(case, beams, 0.999)[1]
    plain = sc.fold_one_item(case["C"], 0.999, *beams, case["K"], fused=False)
    fused = sc.fold_one_item(case["C"], 0.999, *beams, case["K"], fused=True)
    assert got[0].tolist() == [c for c, _ in plain] and [s.hex() for s in got[1].tolist()] == [s.hex() for _, s in plain]
    want = sc.replay(case["targets"], case["C"], 0.999, *beams)
    sc.assert_dicts_equal({1: got}, want, case["K"], case["D"])
    assert len(beams[2]) - 1 >= 300                      # a few hundred merges
    assert any(a != b for (_, a), (_, b) in zip(plain, fused)) or [c for c, _ in plain] != [c for c, _ in fused]


def test_header_binding_and_shim_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    shim = open(os.path.join(ROOT, "jni", "dismember_jni.c")).read()
    scala = open(os.path.join(ROOT, "scala", "com", "mass", "hip", "Native.scala")).read()
    for name, meth in (("dm_dr_mstep_streaming_path_scores", "drMstepStreamingPathScores"), ("dm_dr_mstep_streaming_path_scores_dev", "drMstepStreamingPathScoresDev")):
        assert re.search(r"\bint %s\(" % name, hdr)
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 15
        assert "Java_com_mass_hip_Native_%s(" % meth in shim and "@native def %s(" % meth in scala
    assert "CoordinateDescent.scala:162-212" in hdr
    from dismember_amd import Engine
    assert callable(Engine.dr_mstep_streaming_path_scores) and callable(Engine.dr_mstep_streaming_path_scores_dev)
    assert inspect.signature(dr_mstep.streaming_path_scores_dev).parameters["decay_factor"].default == 0.999
    assert inspect.signature(dr_mstep.optimize).parameters["path_scores"].default == "host"
    with pytest.raises(ValueError):                      # the new spelling serves the streaming mode only (checked before the engine is touched)
        dr_mstep.optimize(type("E", (), {"dr_dims": dict(K=2, D=2)})(), None, None, [], 2, 1, train_mode="batch", path_scores="device_streaming")
