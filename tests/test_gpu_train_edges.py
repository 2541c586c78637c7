"""The training step (dm_train_rows_kernel, dm_wgrad_kernel: dismember_amd/csrc/train_kernel.hip.inc) on the batches production
builds and at the edges of its tiling, every tensor of the gradient under a bound of its own.

Reference: the fp64 numpy restatement tests/train_ref.py (held to the C oracle and to finite differences by tests/test_train_host.py,
which also asserts the conditions every batch below is built to meet).  Bound per element: |g - ref| <= k_T eps A, eps = 2^-24 (f32
model) or 2^-53 (f64), A = the accumulated magnitude of the element's contributions (a table row: its largest), k_T per tensor from
tests/golden/train_tolerances.json = 8 x the C oracle's own largest error in those units (tools/train_tolerances.py; never taken from
the device).  Elements with A == 0 are exactly 0.  Loss: 1e-5 + 1e-4 |x| (f64: 1e-10 + 1e-9 |x|).  Adam: bit-exact on the device's
gradient, which also holds the active-row list to every row reached only as a shared history key.

  T1  histories replicated over a user's rows (the `uniform` reduction of pass D): 16 / 7 / 20 / 33 rows per user in one batch —
      tiles of one user, of two and of three, users straddling tiles; an all-pad user, a one-key user, two neighbours padding the
      same leading positions; B % 16 = 9;  E x L incl. the 32-position instance
  T2  candidates and keys from disjoint halves of the table: the dq and the dk part of the table gradient, each on its own rows
  T3  more tiles than waves x 304 CUs: the grid-stride loop's second round with dead waves beside live ones; the last user's keys
      belong to nobody else, so anything a dead row (a copy of row B - 1) adds lands where A is small
  T4  B = 1 .. 131: the single partial tile, the last dm_wgrad_kernel chunk with B % 8 in 1..3 and B % 128 in {0, 1}
  T5  one candidate for every row; a candidate that is one of its own keys; -1 candidates; -1 history entries left unmasked
"""
import json
import os

import numpy as np
import pytest

import train_ref as R

pytestmark = pytest.mark.gpu
TOL = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "train_tolerances.json")))


def _check_tensor(name, t, got, ref_g, scale, k, eps):
    live = scale > 0
    assert (got[~live] == 0).all(), (name, t, "non-zero where nothing was added", int((got[~live] != 0).sum()))
    ratio = np.abs(got.astype(np.float64) - ref_g)[live] / (eps * scale[live])
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%s %-6s max |g - ref| / (eps A) = %9.3f  (k_T = %.3f)" % (name, t, worst, k))
    assert worst <= k, (name, t, worst, k, int((ratio > k).sum()), int(ratio.size))


def _run_batch(oracle, name, c, i):
    from dismember_amd import Engine
    b, ref = c["batches"][i], R.reference(name, i)
    E, L, NI, f64 = c["E"], c["L"], c["NI"], c["dtype"] == "f64"
    eps, k = R.EPS[c["dtype"]], TOL[c["dtype"]]["k"]
    eng = Engine(0)
    try:
        eng.load_weights_din(c["w"], E, NI)
        eng.train_init(lr=1e-3)
        loss = eng.train_forward_backward(b["codes"], b["seqs"], b["pad"], b["y"])
        g = eng.train_download("grad")
        assert g.dtype == c["w"].dtype
        print("%s loss %.9g  ref %.9g" % (name, loss, ref["loss"]))
        assert abs(loss - ref["loss"]) <= ((1e-10 + 1e-9 * abs(ref["loss"])) if f64 else (1e-5 + 1e-4 * abs(ref["loss"])))
        scale = R.element_scale(ref["A"], E, NI)
        for t, (a, e) in R.sections(E, NI).items():
            _check_tensor(name, t, g[a:e], ref["g"][a:e], scale[a:e], k[t], eps)
        assert (g[:NI * E].reshape(NI, E)[~ref["touched"]] == 0).all()
        if c["kind"] == "disjoint":            # candidate rows hold dq alone and key rows dk alone: each part under the table bound
            half, gt = NI // 2, g[:NI * E].reshape(NI, E)
            for part, rows in (("dq", slice(0, half)), ("dk", slice(half, NI))):
                s = np.repeat(ref["A_" + part][rows].max(axis=1), E)
                _check_tensor(name, "table." + part, gt[rows].reshape(-1), ref["g_" + part][rows].reshape(-1), s, k["table"], eps)
        eng.adam_step(1.0)
        want = c["w"].copy()
        opt = oracle.Adam(want.size, c["w"].dtype.type, lr=1e-3)
        opt.step(want, g.copy())
        assert np.array_equal(eng.train_download("weights"), want)
        assert np.array_equal(eng.train_download("s"), opt.s) and np.array_equal(eng.train_download("r"), opt.r)
        assert (eng.train_download("grad") == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(R.CASES))
def test_train_step_edges(oracle, name):
    c = R.make_case(name)
    for i in range(len(c["batches"])):
        _run_batch(oracle, name, c, i)
