"""CPU checks of what tests/test_gpu_train_edges.py stands on: the fp64 numpy restatement of the training step (tests/train_ref.py)
against the C oracle and against finite differences, the conditions its batches are built to meet (so that no GPU case is vacuous),
and the per-tensor constants of the gradient bound (tests/golden/train_tolerances.json, tools/train_tolerances.py)."""
import json
import os
import sys

import numpy as np
import pytest

import train_ref as R
from helpers import random_din_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import train_tolerances as TT  # noqa: E402


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_matches_fp64_oracle(oracle, name):
    """every batch of every GPU case (the -1 candidates included: the C oracle looks them up as zero rows): loss and every tensor of
    the gradient within 1e-12 of the tensor's largest element of orc_din_train_grads_f64 on the same weights widened to fp64"""
    c = R.make_case(name)
    for i, b in enumerate(c["batches"]):
        ref = R.reference(name, i)
        pad = b["pad"] if b["pad"] is not None else np.zeros(0, np.int32)
        oloss, og = oracle.Din(c["w"].astype(np.float64), c["E"], c["L"], c["NI"]).train_grads(b["codes"], b["seqs"], pad, b["y"])
        assert abs(ref["loss"] - oloss) <= 1e-12 * max(1.0, abs(oloss))
        for t, (a, e) in R.sections(c["E"], c["NI"]).items():
            assert np.abs(ref["g"][a:e] - og[a:e]).max() <= 1e-12 * np.abs(og[a:e]).max(), (name, i, t)
        assert np.array_equal(ref["g"][slice(*R.sections(c["E"], c["NI"])["table"])].reshape(c["NI"], c["E"]), ref["g_dq"] + ref["g_dk"])
        assert (ref["A"] >= np.abs(ref["g"])).all()
        A_rows = ref["A"][:c["NI"] * c["E"]].reshape(c["NI"], c["E"]).max(axis=1)
        assert (A_rows[~ref["touched"]] == 0).all()
        # far from the ReLU's kink: 64 roundings of a pre-activation's accumulated magnitude, in the arithmetic of the case
        assert ref["relu_margin"] >= 64 * R.EPS[c["dtype"]], (name, ref["relu_margin"])


def _small_problem(seed=11, E=16, L=10, NI=63, B=40, embed_size=None):
    rng = np.random.default_rng(seed)
    w = random_din_weights(rng, E, NI, std=0.3, bias_std=0.3, dtype=np.float64)
    b = R.independent_batch(rng, B, L, (0, NI), (0, NI))
    b["codes"][3] = -1                                            # a -1 candidate
    b["seqs"][5, :4] = -1                                         # -1 entries that keep their softmax mass: left out of the mask
    b["seqs"][7] = -1                                             # a row whose every position is masked: uniform softmax over zero keys
    b["seqs"][9, 2:] = b["seqs"][9, 9] = 17                       # one key repeated
    pad = R._pads(b["seqs"])
    b["pad"] = pad[~np.isin(pad, 5 * L + np.arange(4))]
    return w, E, L, NI, b


def test_reference_matches_finite_differences():
    """central differences of the fp64 loss on about 50 parameters per tensor (every touched table row is a candidate for the draw),
    on a batch with a -1 candidate, masked and unmasked -1 history entries and a repeated key"""
    w, E, L, NI, b = _small_problem()
    ref = R.step(w, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"])
    assert ref["relu_margin"] >= 1e-4                             # no pre-activation crosses zero within the step below
    rng = np.random.default_rng(0)
    h = 1e-6
    for t, (a, e) in R.sections(E, NI).items():
        pool = np.flatnonzero(np.repeat(ref["touched"], E)) if t == "table" else np.arange(a, e)
        for i in rng.choice(pool, min(50, pool.size), replace=False):
            wp, wm = w.copy(), w.copy()
            wp[i] += h
            wm[i] -= h
            fd = (R.step(wp, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"], loss_only=True) -
                  R.step(wm, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"], loss_only=True)) / (2 * h)
            assert abs(fd - ref["g"][i]) <= 1e-8 * np.abs(ref["g"][a:e]).max() + 1e-9, (t, i, fd, ref["g"][i])
    untouched = ~np.repeat(ref["touched"], E)
    assert (ref["g"][:NI * E][untouched] == 0).all() and (ref["A"][:NI * E][untouched] == 0).all()


def test_reference_pad_and_scale_rules(oracle):
    w, E, L, NI, b = _small_problem()
    ref = R.step(w, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"])
    # an unmasked -1 entry is a zero key that takes softmax mass: masking it changes the loss, and it receives nothing either way
    full = R.step(w, E, L, NI, b["codes"], b["seqs"], R._pads(b["seqs"]), b["y"])
    assert abs(full["loss"] - ref["loss"]) > 1e-6
    # the chunked accumulation is the unchunked one
    one = R.step(w, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"], chunk=7)
    assert np.abs(one["g"] - ref["g"]).max() <= 1e-15 * np.abs(ref["g"]).max() and abs(one["loss"] - ref["loss"]) <= 1e-15
    # a model of embed size 12 zero-padded to 16: same loss, same gradient on the model's own elements, scale 1 / sqrt(12)
    Em = 12
    rng = np.random.default_rng(5)
    wm = random_din_weights(rng, Em, NI, std=0.3, bias_std=0.3, dtype=np.float64)
    sm, sp = R.sections(Em, NI), R.sections(E, NI)
    wpad = np.zeros(sp["l2.b"][1])
    put = lambda dst, t, shape_p, src, shape_m: dst[slice(*sp[t])].reshape(shape_p).__setitem__(tuple(slice(0, n) for n in shape_m), src[slice(*sm[t])].reshape(shape_m))
    put(wpad, "table", (NI, E), wm, (NI, Em))
    put(wpad, "att.W", (E, E), wm, (Em, Em))
    l1m = wm[slice(*sm["l1.W"])].reshape(Em, 2 * Em)
    l1p = wpad[slice(*sp["l1.W"])].reshape(E, 2 * E)
    l1p[:Em, :Em], l1p[:Em, E:E + Em] = l1m[:, :Em], l1m[:, Em:]
    put(wpad, "l1.b", (E,), wm, (Em,))
    put(wpad, "l2.W", (E,), wm, (Em,))
    wpad[sp["l2.b"][0]] = wm[sm["l2.b"][0]]
    gm = R.step(wm, Em, L, NI, b["codes"], b["seqs"], b["pad"], b["y"])
    gp = R.step(wpad, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"], embed_size=Em)
    assert abs(gm["loss"] - gp["loss"]) <= 1e-14
    assert np.abs(gp["g"][:NI * E].reshape(NI, E)[:, :Em] - gm["g"][:NI * Em].reshape(NI, Em)).max() <= 1e-14 * np.abs(gm["g"]).max()
    assert np.abs(gp["g"][slice(*sp["l1.W"])].reshape(E, 2 * E)[:Em, E:E + Em] - gm["g"][slice(*sm["l1.W"])].reshape(Em, 2 * Em)[:, Em:]).max() <= 1e-14
    assert abs(R.step(wpad, E, L, NI, b["codes"], b["seqs"], b["pad"], b["y"])["loss"] - gm["loss"]) > 1e-8       # 1 / sqrt(16) is another model


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["kind"] in ("shared", "wrap", "disjoint")])
def test_replicated_history_batches_meet_their_conditions(name):
    c = R.make_case(name)
    b = c["batches"][0]
    B = len(b["codes"])
    assert (b["seqs"] == b["seqs"][np.searchsorted(b["users"], b["users"])]).all()          # one history per user, rows user-major
    uniform_all, multi, triple, pad_only = R.tile_report(b)
    assert uniform_all >= 1 and multi >= 1 and triple >= 1
    if c["kind"] == "shared":
        assert B % 16 == 9 and set(R.SHARED_ROWS) == {16, 7, 20, 33} and pad_only >= 1
        seq = b["seqs"][np.searchsorted(b["users"], np.arange(len(R.SHARED_ROWS)))]
        assert (seq[R.ALL_PAD_USER] == -1).all() and seq[R.ONE_KEY_USER, 0] >= 0 and (seq[R.ONE_KEY_USER] == seq[R.ONE_KEY_USER, 0]).all()
        u, v = R.PAD_PAIR
        assert v == u + 1 and (seq[[u, v], :3] == -1).all() and (seq[[u, v], 3:] >= 0).all()
    if c["kind"] == "wrap":
        tiles = -(-B // 16)
        assert tiles > R.WAVES[c["dtype"]] * R.MAX_CUS and tiles <= 2 * R.WAVES[c["dtype"]] * 256 and B % 16 == 9
        last = b["seqs"][-1]
        rest = b["seqs"][b["users"] != b["users"][-1]]
        assert (last >= 0).all() and not np.isin(rest, last).any() and not np.isin(b["codes"], last).any()
        assert (b["users"] == b["users"][-1]).sum() == 25                                    # the 9-row tile and the full tile before it
        keys = np.unique(b["seqs"][b["seqs"] >= 0])
        assert not np.isin(keys, b["codes"]).any() and 4 * (keys.size + np.unique(b["codes"]).size) < c["NI"]     # Adam walks its row list
    if c["kind"] == "disjoint":
        for i, bb in enumerate(c["batches"]):
            keys = bb["seqs"][bb["seqs"] >= 0]
            assert not np.isin(keys, bb["codes"]).any() and bb["codes"].max() < c["NI"] // 2 <= keys.min()
            ref = R.reference(name, i)
            assert (ref["g_dk"][:c["NI"] // 2] == 0).all() and (ref["g_dq"][c["NI"] // 2:] == 0).all()
        assert c["batches"][1]["users"] is None


def test_edge_batches_meet_their_conditions():
    for dt in ("f32", "f64"):
        b = R.make_case("T5-%s-same_candidate" % dt)["batches"][0]
        assert (b["codes"] == b["codes"][0]).all()
        b = R.make_case("T5-%s-candidate_is_key" % dt)["batches"][0]
        masked = np.zeros(b["seqs"].size, bool)
        masked[b["pad"]] = True
        assert (((b["seqs"] == b["codes"][:, None]) & ~masked.reshape(b["seqs"].shape)).any(axis=1)).all() and (b["codes"] >= 0).all()
        b = R.make_case("T5-%s-no_candidate" % dt)["batches"][0]
        assert 0.04 <= (b["codes"] == -1).mean() <= 0.06
        b = R.make_case("T5-%s-unmasked_pads" % dt)["batches"][0]
        assert b["pad"] is None and (b["seqs"] == -1).sum() > 100
        assert [R.CASES["T4-%s-B%d" % (dt, B)]["B"] for B in (1, 2, 15, 17, 127, 128, 129, 131)] == [1, 2, 15, 17, 127, 128, 129, 131]
    assert sorted(B % 8 for B in (129, 131, 17, 2)) == [1, 1, 2, 3] and 128 % 128 == 0 and 129 % 128 == 1      # the dm_wgrad_kernel chunk and k-step edges


# tensors whose bound is at least 20 times tighter than the older whole-vector floor at every case / the measured factor of the others
TIGHTENING_MET = {"f32": (), "f64": ("table", "att.W", "l1.W", "l1.b", "l2.b")}


def test_tolerances_are_what_the_tool_measures(oracle):
    """the committed constants are the tool's (8 x the C oracle's own largest error in units of eps A, per tensor and arithmetic);
    the factor by which each bound undercuts the older floor is recorded next to them"""
    disk = json.load(open(TT.PATH))
    now = TT.compute(oracle)
    assert disk["margin"] == now["margin"] == 8
    for dt in ("f32", "f64"):
        assert sorted(disk[dt]["cases"]) == sorted(now[dt]["cases"])
        for t in R.TENSORS:
            worst = max(c[t] for c in disk[dt]["cases"].values())
            assert disk[dt]["k"][t] == pytest.approx(8 * worst) and worst > 0
            # f32: the restatement's own rounding is 2^-29 of these figures.  f64: the figure IS the rounding of two fp64 evaluations
            # against each other, one of them numpy's BLAS — it moves with the BLAS kernel of the host CPU (0.6 x on l1.W between two
            # OpenBLAS core types), so the committed value is held to one bit of the three-bit margin
            for key in ("k", "tightening"):
                if dt == "f32":
                    assert disk[dt][key][t] == pytest.approx(now[dt][key][t], rel=1e-6), (dt, key, t)
                else:
                    assert 0.5 <= disk[dt][key][t] / now[dt][key][t] <= 2.0, (dt, key, t, disk[dt][key][t], now[dt][key][t])
            print("%s %-6s k_T = %10.3f  older floor / largest bound = %.3g" % (dt, t, disk[dt]["k"][t], disk[dt]["tightening"][t]))
            assert (disk[dt]["tightening"][t] >= 20) == (t in TIGHTENING_MET[dt]), (dt, t, disk[dt]["tightening"][t])
