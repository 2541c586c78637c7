"""Path assignment of the Deep-Retrieval M-step on the device, the part that needs no GPU: the CSR restatement
tests/dr_assign_ref.py equals oracle/dr_mstep_oracle.optimize and dr_mstep.assign_paths on the hit items of every case of
tests/dr_assign_cases.py; every case has the structure it names; the "exact" cases are won by more than 8 tolerances at every decision and
keep the integer powers exact; the stop case makes math.log1p raise on the host; the random-draw restatement is in range and depends on
seed, item and slot; header, binding and generated shim declare the entry points."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import dr_assign_cases as ac
import dr_assign_ref as ref
from dismember_amd import _native, dr_mstep
from oracle import dr_mstep_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dicts(case):
    off, codes, scores, occ = (case[k] for k in ("off", "codes", "scores", "occ"))
    hit = ref.hit_items(case).tolist()
    sc = {v: (codes[off[v]:off[v + 1]], scores[off[v]:off[v + 1]]) for v in hit}
    return hit, sc, {v: int(occ[v]) for v in hit}


@pytest.mark.parametrize("name", list(ac.CASES))
def test_restatement_equals_oracle_and_host_route(name):
    case, want = ac.get(name)
    hit, sc, occ = _dicts(case)
    kw = dict(penalty_factor=case["pf"], penalty_poly_order=case["p"])
    o = dr_mstep_oracle.optimize({v: list(zip(sc[v][0].tolist(), sc[v][1].tolist())) for v in hit}, occ, hit, case["T"], case["J"], None, **kw)
    h = dr_mstep.assign_paths(sc, occ, hit, case["T"], case["J"], case["K"], case["D"], **kw)
    assert sorted(o) == hit == sorted(h)
    for v in hit:
        assert want["out"][v].tolist() == o[v]
        assert [tuple(r) for r in dr_mstep.decode_codes(want["out"][v], case["K"], case["D"]).tolist()] == h[v]
    assert len(want["decisions"]) == case["T"] * len(hit) * case["J"]
    assert dr_mstep.pack_csr(sc, occ, len(case["occ"]))[0].tolist()[-1] == sum(len(sc[v][0]) for v in hit)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_margins_and_exact_powers(name):
    case, want = ac.get(name)
    assert (max(want["sizes"].values()) + 2) ** case["p"] < 2 ** 53
    worst = ref.min_margin(case, want)
    if name in ac.NOT_EXACT:
        assert worst == 0.0
    else:
        assert worst > 8.0, worst


def test_cases_have_the_structure_they_name():
    cnt = lambda c: np.diff(c["off"])[ref.hit_items(c)]
    for name, n in (("C63", 63), ("C64", 64), ("C65", 65), ("C130", 130), ("C2048", 2048), ("c1_j1", 1)):
        assert (cnt(ac.get(name)[0]) == n).all()
    assert ac.get("c1_j1")[0]["J"] == 1 and ac.get("j_eq_c")[0]["J"] == 4 and (cnt(ac.get("j_eq_c")[0]) == 4).all()
    assert ac.get("T1")[0]["T"] == 1 and ac.get("p1")[0]["p"] == 1 and ac.get("p4")[0]["p"] == 4 and ac.get("pf0")[0]["pf"] == 0.0
    assert [len(ref.hit_items(ac.get(n)[0])) for n in ("hit1", "hit2", "hit257")] == [1, 2, 257] and len(ac.get("hit1")[0]["occ"]) == 1
    c, w = ac.get("shared")
    lists = [c["codes"][a:b].tolist() for a, b in zip(c["off"][:-1], c["off"][1:])]
    assert all(l == lists[0] for l in lists) and len(lists) == 40
    # the sizes matter there: without the penalty the assignment is another one
    assert not np.array_equal(ref.assign_ref(dict(c, pf=0.0))["out"], w["out"])
    c, _ = ac.get("alternating")
    lists = [set(c["codes"][a:b].tolist()) for a, b in zip(c["off"][:-1], c["off"][1:])]
    assert all(lists[i] == lists[i & 1] for i in range(len(lists))) and not (lists[0] & lists[1])
    c, w = ac.get("crowd")
    assert (c["codes"][c["off"][:-1]] == 0).all() and len(c["occ"]) == 300
    first = w["sel"][0, :, c["J"] - 1]
    assert first[0] == 0 and (first != 0).any() and 0 < w["sizes"][0] < 300          # taken at first, left later
    c, w = ac.get("tie")
    s = c["scores"][c["off"][0]:c["off"][1]]
    assert s[0] == s[1] == s[2] and w["sel"][0, 0, c["J"] - 1] == 0
    c, _ = ac.get("sparse")
    assert ref.hit_items(c).tolist() == [0, 1700, 1701, 4999] and len(c["occ"]) == 5000
    # the ring: 257 items of 20 candidates do not fit one staged batch (64 items, 1 024 entries)
    assert len(ref.hit_items(ac.get("hit257")[0])) > 4 * 51


def test_stop_case_raises_on_the_host():
    case = ac.stop_case()
    hit, sc, occ = _dicts(case)
    assert hit[0] == 3
    with pytest.raises(ValueError):
        dr_mstep.assign_paths(sc, occ, hit, case["T"], case["J"], case["K"], case["D"], penalty_factor=case["pf"], penalty_poly_order=case["p"])
    v = hit[0]
    g0 = max(ref.gain(occ[v], s, 0.0, 0, case["pf"], case["p"]) for s in sc[v][1].tolist())
    assert g0 <= -1.0                                    # the first visit's second round is where log1p has no value
    with pytest.raises(ValueError):
        math.log1p(g0)
    with pytest.raises(ValueError):
        ref.assign_ref(case)


def test_random_draw_restatement():
    base = [ref.random_code(5, v, j, 64, 3) for v in range(50) for j in range(3)]
    assert all(0 <= c < 64 ** 3 for c in base) and len(set(base)) > 140
    assert base != [ref.random_code(6, v, j, 64, 3) for v in range(50) for j in range(3)]
    assert ref.random_code(5, 1, 0, 64, 3) != ref.random_code(5, 2, 0, 64, 3) != ref.random_code(5, 2, 1, 64, 3)
    nodes = [ref.random_node(9, v, 0, 0, 7) for v in range(7000)]
    assert min(nodes) == 0 and max(nodes) == 6 and abs(np.bincount(nodes) - 1000).max() < 150       # five sigma of a fair draw is 146
    assert all(0 <= ref.random_node(1, v, 1, 2, (1 << 31) - 1) < (1 << 31) - 1 for v in range(100))


def test_header_binding_and_shim_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dismember_hip.h")).read()
    shim = open(os.path.join(ROOT, "jni", "dismember_jni.c")).read()
    scala = open(os.path.join(ROOT, "scala", "com", "mass", "hip", "Native.scala")).read()
    for name, meth, nargs in (("dm_dr_mstep_assign_paths", "drMstepAssignPaths", 20), ("dm_dr_mstep_assign_paths_dev", "drMstepAssignPathsDev", 20),
                              ("dm_dr_mstep_optimize", "drMstepOptimize", 13)):
        assert re.search(r"\bint %s\(" % name, hdr)
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
        assert "Java_com_mass_hip_Native_%s(" % meth in shim and "@native def %s(" % meth in scala
    assert "CoordinateDescent.scala:48-82" in hdr
    from dismember_amd import Engine
    from dismember_amd.dr_train import DRTrainer
    assert callable(Engine.dr_mstep_assign_paths) and callable(Engine.dr_mstep_assign_paths_dev) and callable(Engine.dr_mstep_optimize)
    sig = inspect.signature(dr_mstep.optimize).parameters
    assert sig["assign"].default == "host" and sig["path_scores"].default == "host" and sig["as_array"].default is False
    assert inspect.signature(dr_mstep.assign_paths_dev).parameters["as_array"].default is False
    assert inspect.signature(DRTrainer.mstep).parameters["assign"].default == "host"
    with pytest.raises(ValueError):
        dr_mstep.optimize(type("E", (), {"dr_dims": dict(K=2, D=2)})(), None, None, [], 2, 1, assign="gpu")
