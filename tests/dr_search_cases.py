"""Named cases of the Deep-Retrieval beam search and a float64 model of what its kernels branch on (plain numpy: no GPU, no HIP library).

The search kernels (dismember_amd/csrc/dr_kernel.hip.inc, dr_sliced.hip.inc) choose their path per (user, layer) from the DATA: how far the
column-sliced route's bound Mhat = max S + sum max T sits above a path's largest logit, how small the beam-th candidate probability is,
how many candidates tie with it.  `classify` computes those quantities along the fp64 beam and labels every user-layer; `sliced_cut_model`
restates the sliced route's tabulated-product cut in the case's precision and counts the winners it would lose.

tests/test_dr_search_cases_host.py checks the table on the CPU, tests/test_gpu_dr_search_ranges.py runs it on the device.
"""
import functools

import numpy as np

from dismember_amd import synth
from test_gpu_dr import histories

NUM_ITEM = 500
NP_T = {"f32": np.float32, "f64": np.float64}

# ---- the cases ------------------------------------------------------------------------------------------------------------------
# Seeds are chosen so that tests/test_dr_search_cases_host.py holds (no near-ties in the fp64 lists, enough user-layers of every label
# in the wide cases, no subnormal result); the shapes, scales and types are the point of each case.
CASES = {}


def _case(name, group, K, D, beam, U, scale, dtype, seed, L=4, E=16, zero_layers=False):
    CASES[name] = dict(name=name, group=group, K=K, D=D, L=L, E=E, beam=beam, U=U, scale=scale, dtype=dtype, seed=seed,
                       num_item=NUM_ITEM, zero_layers=zero_layers)


_case("control_f32", "control", 100, 3, 20, 48, 0.3, "f32", 7)
_case("control_f64", "control", 100, 3, 20, 48, 0.3, "f64", 7)
_case("wide_f32_2.0", "wide", 100, 3, 20, 48, 2.0, "f32", 7)
_case("wide_f32_2.25", "wide", 100, 3, 20, 48, 2.25, "f32", 7)
_case("wide_f64_6.0", "wide", 100, 3, 20, 48, 6.0, "f64", 7)
_case("wide_f64_7.0", "wide", 100, 3, 20, 48, 7.0, "f64", 7)
for _dt in ("f32", "f64"):
    for _beam in (7, 64):       # the model of test_gpu_dr.py::test_ties_are_stable: every logit is 0, every candidate of a layer ties
        _case("ties_%s_b%d" % (_dt, _beam), "ties", 70, 3, _beam, 4, 0.3, _dt, 0, L=3, zero_layers=True)
_case("edges_1024x2", "edges", 1024, 2, 64, 8, 0.3, "f64", 7)     # the full eight slices
_case("edges_1001x4", "edges", 1001, 4, 64, 8, 0.3, "f64", 7)     # three tables per path, 16-byte loads that straddle K
_case("edges_129x3", "edges", 129, 3, 64, 8, 0.3, "f64", 7)       # one live column in slice 1


def n2_of(beam):
    n = 1
    while n < beam:
        n <<= 1
    return n


def nl_of(beam):
    """Capacity of the kernels' candidate lists (dr_beam_nl)."""
    return max(4 * n2_of(beam), 256)


@functools.lru_cache(maxsize=None)
def build(name):
    """Weights (float64 arrays holding exactly the values the device holds), histories and the float64 tables S_d [U, K] (history part of
    layer d's logits, bias included) and T_{d,t} [K, K] (row n: what node n at layer t adds to layer d's logits)."""
    c = dict(CASES[name])
    K, D, L, E, n = c["K"], c["D"], c["L"], c["E"], c["num_item"]
    rng = np.random.default_rng(c["seed"])
    w = synth.make_dr_model(n, K, D, L, E, rng, scale=c["scale"])
    if c["zero_layers"]:
        for k in ("layer_w", "layer_b"):
            w[k] = [np.zeros_like(a) for a in w[k]]
    if c["dtype"] == "f32":       # as tests/test_gpu_dr.py::make: the oracle sees exactly the values the device holds
        for k, v in list(w.items()):
            w[k] = [a.astype(np.float32).astype(np.float64) for a in v] if isinstance(v, list) else v.astype(np.float32).astype(np.float64)
    seqs = histories(rng, c["U"], L, n)
    seqs[2] = seqs[1]             # identical users: identical results
    emb = w["layer_emb"]
    X = np.where((seqs >= 0)[:, :, None], emb[np.maximum(seqs, 0)], 0.0).reshape(c["U"], L * E)
    S = [X @ w["layer_w"][d][:, :L * E].T + w["layer_b"][d] for d in range(D)]
    T = {(d, t): emb[n + t * K:n + (t + 1) * K] @ w["layer_w"][d][:, (L + t) * E:(L + t + 1) * E].T for d in range(D) for t in range(d)}
    c.update(w=w, seqs=seqs, S=S, T=T)
    return c


# ---- the search, restated in numpy in either precision ----------------------------------------------------------------------------
def _softmax(lg):
    """package.scala:23-28 per row: max, exp(x - max), sequential sum, divide — in the dtype of `lg`."""
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return e / np.add.accumulate(e, axis=1)[:, -1:]


def _logits(c, u, d, nodes, dt):
    """LayerModel.inference for the paths `nodes` [np, d] of user u: products accumulated per output in ascending column order from 0,
    then the bias (oracle/dr_body.inc) — sequential dots in the precision dt."""
    K, L, E, n = c["K"], c["L"], c["E"], c["num_item"]
    emb, W, b = c["w"]["layer_emb"].astype(dt), c["w"]["layer_w"][d].astype(dt), c["w"]["layer_b"][d].astype(dt)
    acc = np.zeros(K, dt)
    for j in range(L):
        if c["seqs"][u, j] >= 0:
            row = emb[c["seqs"][u, j]]
            for e in range(E):
                acc += W[:, j * E + e] * row[e]
    acc = np.repeat(acc[None, :], len(nodes), axis=0)
    for t in range(d):
        rows = emb[n + t * K + nodes[:, t]]
        for e in range(E):
            acc += W[None, :, (L + t) * E + e] * rows[:, e:e + 1]
    return acc + b


def beam_search(name, dtype=np.float64, layers=False):
    """CandidateSearcher.beamSearch for every user of the case in the precision `dtype`: (paths [U, beam, D], probs [U, beam], counts
    [U]), rows past the count -1 / 0.  layers=True adds, per user, a list over d of dict(nodes, pprob, cand, win): the state entering
    layer d, every candidate's probability [np, K] and the winners' flat indices in output order."""
    c = build(name)
    K, D, beam, U = c["K"], c["D"], c["beam"], c["U"]
    paths = np.full((U, beam, D), -1, np.int32)
    probs = np.zeros((U, beam), np.float64)
    cnt = np.zeros(U, np.int32)
    rec = []
    for u in range(U):
        nodes, pp, lay = np.zeros((1, 0), np.int64), np.ones(1, dtype), []
        for d in range(D):
            cand = pp[:, None] * _softmax(_logits(c, u, d, nodes, dtype))
            win = np.argsort(-cand.reshape(-1), kind="stable")[:beam]          # stable sortBy ... reverse, take(beamSize)
            lay.append(dict(nodes=nodes, pprob=pp, cand=cand, win=win))
            nodes = np.concatenate([nodes[win // K], (win % K)[:, None]], axis=1)
            pp = cand.reshape(-1)[win]
        cnt[u] = len(pp)
        paths[u, :len(pp)] = nodes
        probs[u, :len(pp)] = pp
        rec.append(lay)
    return (paths, probs, cnt, rec) if layers else (paths, probs, cnt)


@functools.lru_cache(maxsize=None)
def beam64(name):
    """The fp64 search with its per-layer records, computed once per case."""
    return beam_search(name, np.float64, layers=True)


def path_probs(name, u, paths, dtype):
    """Probability of each of `paths` [n, D] for user u, walked layer by layer in the precision `dtype` (test_gpu_dr.py::path_prob)."""
    c = build(name)
    paths = np.asarray(paths, np.int64)
    pr = np.ones(len(paths), dtype)
    for d in range(c["D"]):
        sm = _softmax(_logits(c, u, d, paths[:, :d], dtype))
        pr = pr * sm[np.arange(len(paths)), paths[:, d]]
    return pr


# ---- what the kernels branch on -----------------------------------------------------------------------------------------------------
# Labels carry safety margins so that rounding (of the device's tables, of this model) cannot move them.  With the products
# exp(l - Mhat) <= exp(-gap) of a path, gap = Mhat - max logit:
#   f32: smallest normal 2^-126 = exp(-87.3), smallest subnormal 2^-149 = exp(-103.3); a product below half of that, exp(-104.0),
#        rounds to zero.  fp64: 2^-1022 = exp(-708.4), 2^-1074 = exp(-744.4), zero below exp(-745.1).
#   GAP_ZERO: above it every product of the path is zero whether subnormals are kept or not, with a factor exp(6) (f32) / exp(15) (fp64)
#        to spare for the rounding of the tabulated factors, which are subnormal themselves down there: the sum is 0.
#   GAP_FAST: below it the largest product is >= exp(-20) = 2e-9, 29 (f32) / 298 (fp64) decades above the smallest normal.
#   PB_FAST:  the beam-th candidate probability above it keeps the cut score 18 (f32) / 190 (fp64) decades above the kernels' score
#        floors (1e-30 / 1e-290) and, in product space (times the sum >= 2e-9), 14 / 190 decades above the smallest normal.
GAP_FAST = 20.0
GAP_ZERO = {"f32": 110.0, "f64": 760.0}
PB_FAST = {"f32": 1e-12, "f64": 1e-100}


def _mhat_gap(c, u, d, nodes, lg):
    mh = c["S"][d][u].max() + sum(c["T"][(d, t)][nodes[:, t]].max(axis=1) for t in range(d))
    return mh, mh - lg.max(axis=1)


@functools.lru_cache(maxsize=None)
def classify(name):
    """One record per (user, layer d >= 1) along the fp64 beam: dict(u, d, gaps [np] (Mhat - max logit per live path), pb (the beam-th
    candidate probability), ties (candidates exactly equal to pb), label in {"fast", "must_exact", "open"})."""
    c = build(name)
    dt = c["dtype"]
    out = []
    rec = beam64(name)[3]
    for u in range(c["U"]):
        for d in range(1, c["D"]):
            r = rec[u][d]
            lg = c["S"][d][u][None, :] + sum(c["T"][(d, t)][r["nodes"][:, t]] for t in range(d))
            _, gaps = _mhat_gap(c, u, d, r["nodes"], lg)
            flat = r["cand"].reshape(-1)
            pb = flat[r["win"][-1]]
            ties = int((flat == pb).sum())
            if (gaps > GAP_ZERO[dt]).any() or ties > nl_of(c["beam"]):
                label = "must_exact"
            elif (gaps < GAP_FAST).all() and pb > PB_FAST[dt]:
                label = "fast"
            else:
                label = "open"
            out.append(dict(u=u, d=d, gaps=gaps, pb=float(pb), ties=ties, label=label))
    return out


def label_counts(name):
    out = {"fast": 0, "must_exact": 0, "open": 0}
    for r in classify(name):
        out[r["label"]] += 1
    return out


# ---- the sliced route's tabulated-product cut, in the case's precision ----------------------------------------------------------------
# DrsTol of dr_sliced.hip.inc: relative margin of the cut, score floor, and (rule "guarded") the two product-space limits
REL = {"f32": np.float32(1e-3), "f64": np.float64(1e-9)}
FLOOR = {"f32": np.float32(1e-30), "f64": np.float64(1e-290)}
PMAX_MIN = {k: NP_T[k](16384) * np.finfo(NP_T[k]).tiny / REL[k] for k in NP_T}
PROD_MIN = {k: NP_T[k](32) * np.finfo(NP_T[k]).tiny / REL[k] for k in NP_T}


def sliced_cut_model(name, flush, rule):
    """drs_stats_kernel + the cut of drs_select(_wave)_kernel for every (user, layer d >= 1), fed with the fp64 beam's state: factors
    exp(S - max S), exp(T - max T) and their products and sums in the case's precision T (flush=True: subnormal results become 0, as on
    a device that flushes them), maxima over 16-column blocks, tau = the beam-th largest block score (the kernels use a lower bound a
    few 2^-16 below: fewer misses, never more), thr = tau (1 - rel).

    rule "parent":  exact path iff a sum is 0 / non-finite or thr is under the score floor.
    rule "guarded": also iff a live path's largest product is below PMAX_MIN or thr / cp of a live path is below PROD_MIN.
    A layer that keeps the cut with fewer survivors than the beam, or more than the list holds, also goes to the exact path (as on the
    device), which is correct by construction.  Returns counts: layers, s_zero (layers with a zero sum), exact, missed (fp64 winners
    whose score is under thr in a layer that keeps the cut), miss_layers, worst (largest missed probability / beam-th probability),
    damaged_kept (layers that keep the cut although a live path's sum is off by more than rel, or a winner's product is below the
    smallest normal)."""
    c = build(name)
    dt, T = c["dtype"], NP_T[c["dtype"]]
    tiny, rel, K, beam = np.finfo(T).tiny, REL[dt], c["K"], c["beam"]
    fl = (lambda x: np.where(np.abs(x) < tiny, T(0), x)) if flush else (lambda x: x)
    rec = beam64(name)[3]
    ET = {}
    for key, tab in c["T"].items():
        tt = tab.astype(T)
        ET[key] = fl(np.exp(tt - tt.max(axis=1, keepdims=True)))
    res = dict(layers=0, s_zero=0, exact=0, missed=0, miss_layers=0, worst=0.0, damaged_kept=0)
    kpad = -K % 16
    with np.errstate(all="ignore"):
        for u in range(c["U"]):
            for d in range(1, c["D"]):
                r = rec[u][d]
                nodes, npth = r["nodes"], len(r["nodes"])
                sd = c["S"][d][u].astype(T)
                pr = np.repeat(fl(np.exp(sd - sd.max()))[None, :], npth, axis=0)
                for t in range(d):
                    pr = fl(pr * ET[(d, t)][nodes[:, t]])
                s = pr.sum(axis=1, dtype=T)
                cp = r["pprob"].astype(T) / s
                braw = np.pad(pr, ((0, 0), (0, kpad))).reshape(npth, -1, 16).max(axis=2)
                bsc = np.zeros(npth * 64, T)
                bsc[:braw.size] = fl(braw * cp[:, None]).reshape(-1)
                tau = np.sort(bsc)[::-1][min(npth * 64, beam) - 1]
                thr = T(tau * (T(1) - rel))
                res["layers"] += 1
                res["s_zero"] += int((s == 0).any())
                exact = bool((~(s > 0) | ~np.isfinite(s)).any()) or not (thr >= FLOOR[dt]) or not np.isfinite(thr)
                if rule == "guarded":
                    exact = exact or bool((braw.max(axis=1) < PMAX_MIN[dt]).any()) or not bool((thr >= PROD_MIN[dt] * cp).all())
                else:
                    assert rule == "parent"
                keep = None
                if not exact:
                    keep = fl(pr * cp[:, None]).reshape(-1) >= thr
                    exact = keep.sum() < len(r["win"]) or keep.sum() > nl_of(beam)
                if exact:
                    res["exact"] += 1
                    continue
                lg = c["S"][d][u][None, :] + sum(c["T"][(d, t)][nodes[:, t]] for t in range(d))
                mh, _ = _mhat_gap(c, u, d, nodes, lg)
                m = lg.max(axis=1)
                log_s_true = m + np.log(np.exp(lg - m[:, None]).sum(axis=1)) - mh
                win_q, win_k = r["win"] // K, r["win"] % K
                thin = (lg[win_q, win_k] - mh[win_q] < np.log(float(tiny)))[keep[r["win"]]]
                if (np.abs(np.log(s.astype(np.float64)) - log_s_true) > float(rel)).any() or thin.any():
                    res["damaged_kept"] += 1
                lost = r["win"][~keep[r["win"]]]
                if len(lost):
                    flat = r["cand"].reshape(-1)
                    res["missed"] += len(lost)
                    res["miss_layers"] += 1
                    res["worst"] = max(res["worst"], float(flat[lost].max() / flat[r["win"][-1]]))
    return res
