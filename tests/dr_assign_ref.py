"""TEST INFRASTRUCTURE — the greedy path assignment of the Deep-Retrieval M-step restated over the CSR arrays the device
entry points take, the random-path draw restated on Python integers, and the replay that judges a device trace.

assign_ref is oracle/dr_mstep_oracle.optimize with arrays for dicts (tests/test_dr_assign_host.py holds the two, and
dr_mstep.assign_paths, against each other).  It also records every decision: (iteration, hit index, round, chosen position, gain,
runner-up gain).

The tolerance of the replay.  Host and device evaluate
    g = nv * (log1p(prob + partial) - log1p(partial)) - penalty_factor * ((s + 1)^p / p - s^p / p)
on the SAME fp64 inputs (the replay carries `partial` forward from the device's own reported gains, `size` from its own choices), with
IEEE operations everywhere except the two log1p calls.  With eps = 2^-52 an ulp of x is at most eps |x|:
  * the device log1p is documented to 1 ulp (HIP math API, double precision log1p: 1 ULP): two calls, 2 ulp;
  * the formula has 8 rounded operations (prob + partial, the difference of the logarithms, the product with nv, two divisions by p, the
    difference of the two quotients, the product with penalty_factor, the final difference; the integer powers are exact while
    (s + 1)^p < 2^53): half an ulp each, 4 ulp;
  * the same again for the host side (glibc's log1p is documented to 1 ulp as well).
So k = 2 * (2 * 1 + 8 / 2) = 12, each ulp taken of a quantity no larger than A = nv (|log1p(prob + partial)| + |log1p(partial)|) + |penalty|,
which bounds every intermediate of the formula except the two quotients — and those are bit-equal on both sides (exact powers, one
correctly rounded division each).  tol = k * eps * A.  Nothing here was tuned on a device result."""
import math

import numpy as np

K_TOL = 12
EPS = 2.0 ** -52
MASK = (1 << 64) - 1
RETRY = 64


def penalty(s, pf, p):
    f = lambda x: math.pow(x, p) / p
    return pf * (f(s + 1) - f(s))


def gain(nv, prob, partial, s, pf, p):
    """the host route's gain (dr_mstep.assign_paths); ValueError from math.log1p where partial <= -1"""
    return nv * (math.log1p(prob + partial) - math.log1p(partial)) - penalty(s, pf, p)


def tol(nv, prob, partial, s, pf, p):
    a = nv * (abs(math.log1p(prob + partial)) + abs(math.log1p(partial))) + abs(penalty(s, pf, p))
    return K_TOL * EPS * a


def hit_items(case):
    return np.flatnonzero(np.asarray(case["occ"]) > 0)


def assign_ref(case):
    """-> dict(out [num_item, J] int64 (-1 in the rows of unhit items), sizes {code: size} of every code of the CSR, decisions
    [(t, g, j, pos, gain, runner_up | None)], sel [T, n_hit, J])"""
    off, codes, scores, occ = (np.asarray(case[k]) for k in ("off", "codes", "scores", "occ"))
    T, J, pf, p = case["T"], case["J"], case["pf"], case["p"]
    hit = hit_items(case)
    size = {int(c): 0 for c in codes.tolist()}
    out = np.full((len(occ), J), -1, np.int64)
    last = np.zeros((len(hit), J), np.int64)
    sel = np.zeros((T, len(hit), J), np.int32)
    decisions = []
    for t in range(1, T + 1):
        for g, v in enumerate(hit.tolist()):
            cc, ss = codes[off[v]:off[v + 1]].tolist(), scores[off[v]:off[v + 1]].tolist()
            nv = int(occ[v])
            chosen, partial = set(), 0.0
            for j in range(J - 1, -1, -1):
                if t > 1:
                    size[cc[last[g, j]]] -= 1
                best, best_g, second = None, None, None
                for pos, (c, prob) in enumerate(zip(cc, ss)):
                    if pos in chosen:
                        continue
                    gn = gain(nv, prob, partial, size[c], pf, p)
                    if best is None or gn > best_g:
                        if best is not None and (second is None or best_g > second):
                            second = best_g
                        best, best_g = pos, gn
                    elif second is None or gn > second:
                        second = gn
                if best is None:
                    raise ValueError("item %d has fewer candidate paths than paths per item" % v)
                size[cc[best]] += 1
                chosen.add(best)
                partial = partial + best_g
                last[g, j] = best
                sel[t - 1, g, j] = best
                decisions.append((t, g, j, best, best_g, second))
            out[v] = [cc[q] for q in last[g]]
    return dict(out=out, sizes=size, decisions=decisions, sel=sel)


def min_margin(case, want):
    """the smallest (winner - runner-up) / tol over the decisions of assign_ref's trajectory; tol: the largest over the item's candidates
    at that decision, with the largest size the run ever sees (the penalty grows with it)"""
    off, scores, occ = (np.asarray(case[k]) for k in ("off", "scores", "occ"))
    hit = hit_items(case)
    smax = max(want["sizes"].values()) + 1
    worst, partial = float("inf"), {}
    for t, g, j, pos, gn, second in want["decisions"]:
        v = int(hit[g])
        if j == case["J"] - 1:
            partial[g] = 0.0
        tl = max(tol(int(occ[v]), s, partial[g], smax, case["pf"], case["p"]) for s in scores[off[v]:off[v + 1]].tolist())
        if second is not None:
            worst = min(worst, (gn - second) / tl)
        partial[g] += gn
    return worst


def _splitmix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def random_node(seed, v, j, d, K):
    """node d of random path j of item v: the first of up to RETRY counter-based draws below the largest multiple of K, modulo K"""
    key = _splitmix(_splitmix((seed & MASK) ^ _splitmix(v)) ^ ((j << 8) | d))
    lim = (1 << 64) // K * K
    r = 0
    for ctr in range(RETRY):
        r = _splitmix(key ^ ((ctr * 0xD6E8FEB86659FD93) & MASK))
        if r < lim:
            break
    return r % K


def random_code(seed, v, j, K, D):
    code = 0
    for d in range(D):
        code = code * K + random_node(seed, v, j, d, K)
    return code


def replay(case, trace_sel, trace_gain):
    """Walks every decision of a device trace, `size` and `partial` carried forward from the device's own choices and reported gains.
    -> (final sizes {code: size}, out [num_item, J] as the choices imply, the number of decisions)"""
    off, codes, scores, occ = (np.asarray(case[k]) for k in ("off", "codes", "scores", "occ"))
    T, J, pf, p = case["T"], case["J"], case["pf"], case["p"]
    hit = hit_items(case)
    assert trace_sel.shape == (T, len(hit), J) and trace_gain.shape == (T, len(hit), J)
    size = {int(c): 0 for c in codes.tolist()}
    out = np.full((len(occ), J), -1, np.int64)
    n = 0
    for t in range(1, T + 1):
        for g, v in enumerate(hit.tolist()):
            cc, ss = codes[off[v]:off[v + 1]].tolist(), scores[off[v]:off[v + 1]].tolist()
            nv = int(occ[v])
            chosen, partial = set(), 0.0
            for j in range(J - 1, -1, -1):
                if t > 1:
                    size[cc[int(trace_sel[t - 2, g, j])]] -= 1
                pos, rep = int(trace_sel[t - 1, g, j]), float(trace_gain[t - 1, g, j])
                where = "iteration %d, item %d, round %d" % (t, v, j)
                assert 0 <= pos < len(cc) and pos not in chosen, where
                free = [q for q in range(len(cc)) if q not in chosen]
                gains = {q: gain(nv, ss[q], partial, size[cc[q]], pf, p) for q in free}
                tols = {q: tol(nv, ss[q], partial, size[cc[q]], pf, p) for q in free}
                assert abs(rep - gains[pos]) <= tols[pos], (where, rep, gains[pos], tols[pos])
                tl = max(tols.values())
                assert gains[pos] >= max(gains.values()) - 2 * tl, (where, gains[pos], max(gains.values()), tl)
                twins = [q for q in free if gains[q] == gains[pos] and ss[q] == ss[pos] and size[cc[q]] == size[cc[pos]]]
                assert pos == min(twins), (where, pos, twins)
                size[cc[pos]] += 1
                chosen.add(pos)
                partial = partial + rep
                n += 1
            out[v] = [cc[int(q)] for q in trace_sel[t - 1, g]]
    return size, out, n
