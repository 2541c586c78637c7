"""Deep-Retrieval M-step: `CoordinateDescent.optimize`
(deep-retrieval/src/main/scala/com/mass/dr/optim/CoordinateDescent.scala:29-83) over the device beam search.

The expensive part — one beam search with `beam = numCandidatePath` per training sample (:143-147, :181-186) — is ONE
batched `dm_dr_beam_search` call per chunk; per-item aggregation is a sort + segmented sum over 64-bit path codes, on the host
(`batch_path_scores`) or without the candidates leaving the device (`batch_path_scores_dev`, `optimize(path_scores="device")`); the
streaming mode's decayed running scores likewise (`streaming_path_scores` on the host, `streaming_path_scores_dev` /
`optimize(train_mode="streaming", path_scores="device_streaming")` on the device).  The greedy,
penalised path choice is inherently sequential over items (a shared path-size table), as in the reference: `assign_paths` is the host
loop, `assign_paths_dev` / `optimize(assign="device")` the same chain as one wave on the device (Engine.dr_mstep_assign_paths,
Engine.dr_mstep_optimize).
Orders the reference takes from hash maps are fixed here: ties between equal path scores resolve to the smaller path code
(ascending node tuple), items are visited in ascending id."""
import math

import numpy as np


def _codes(paths, K):
    c = np.zeros(paths.shape[:-1], np.int64)
    for d in range(paths.shape[-1]):
        c = c * K + paths[..., d]
    return c


def _decode(code, K, D):
    out = []
    for _ in range(D):
        out.append(int(code % K))
        code //= K
    return tuple(reversed(out))


def candidate_paths(engine, sequences, num_candidate_path, chunk=65536):
    """beamSearch(d.sequence, model, numCandidatePath) for every sample -> (path codes [N, C] int64 (-1 = none), probs [N, C])"""
    seqs = np.ascontiguousarray(sequences, np.int32)
    K = engine.dr_dims["K"]
    codes, probs = [], []
    for o in range(0, len(seqs), chunk):
        p, pr, cnt = engine.dr_beam_search(seqs[o:o + chunk], num_candidate_path)
        c = _codes(p.astype(np.int64), K)
        c[np.arange(p.shape[1])[None, :] >= cnt[:, None]] = -1
        codes.append(c)
        probs.append(pr)
    return np.concatenate(codes), np.concatenate(probs)


def batch_path_scores(engine, sequences, targets, num_candidate_path):
    """batchPathScore + aggregatePathScore (:117-163): {item: (codes [m] int64, scores [m] float64)}, scores descending."""
    codes, probs = candidate_paths(engine, sequences, num_candidate_path)
    tg = np.repeat(np.asarray(targets, np.int64), codes.shape[1])
    order_in = np.arange(codes.size)
    c, p = codes.ravel(), probs.ravel()
    keep = c >= 0
    tg, c, p, order_in = tg[keep], c[keep], p[keep], order_in[keep]
    o = np.lexsort((order_in, c, tg))                  # by item, then path, sums in sample order
    tg, c, p = tg[o], c[o], p[o]
    new = np.ones(len(c), bool)
    new[1:] = (tg[1:] != tg[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(new)
    # NOT the reference's left-to-right order: reduceat gives first + sum(rest) per segment, and numpy's add loop sums the rest with eight
    # accumulators once it has eight or more terms.  Two terms always agree with the reference; from three on the last bit can differ.
    # batch_path_scores_dev folds left to right, as the reference does
    sums = np.add.reduceat(p, starts) if len(starts) else p[:0]
    gi, gc = tg[starts], c[starts]
    out = {}
    bounds = np.flatnonzero(np.r_[True, gi[1:] != gi[:-1], True])
    for a, b in zip(bounds[:-1], bounds[1:]):
        s, cc = sums[a:b], gc[a:b]
        k = np.argsort(-s, kind="stable")[:num_candidate_path]     # ties: ascending path code
        out[int(gi[a])] = (cc[k], s[k])
    return out


def batch_path_scores_dev(engine, sequences, targets, num_candidate_path, with_occurrence=False):
    """batch_path_scores on the device (Engine.dr_mstep_path_scores): search, aggregation and the cut at C without the
    candidates leaving the device; every score is summed in sample order.  -> the dict batch_path_scores returns (and, with
    with_occurrence, {item: number of samples})."""
    off, codes, scores, occ = engine.dr_mstep_path_scores(sequences, targets, num_candidate_path)
    items = np.flatnonzero(off[1:] > off[:-1])
    out = {int(v): (codes[off[v]:off[v + 1]], scores[off[v]:off[v + 1]]) for v in items}
    if not with_occurrence:
        return out
    hit = np.flatnonzero(occ)
    return out, dict(zip(hit.tolist(), occ[hit].tolist()))


def streaming_path_scores(engine, sequences, targets, num_candidate_path, decay_factor=0.999, batch_size=8192):
    """streamingPathScore (:165-211): exponentially decayed running scores, merged sample by sample."""
    codes, probs = candidate_paths(engine, sequences, num_candidate_path)
    scores = {}
    for i, item in enumerate(np.asarray(targets).tolist()):
        m = codes[i] >= 0
        cand_c, cand_p = codes[i][m], probs[i][m]
        if item not in scores:
            scores[item] = (cand_c.copy(), cand_p.copy())
            continue
        oc, op = scores[item]
        min_score = op.min()
        union = np.union1d(oc, cand_c)                              # ascending path code
        so = dict(zip(oc.tolist(), op.tolist()))
        sc = dict(zip(cand_c.tolist(), cand_p.tolist()))
        new = np.array([decay_factor * so[u] + sc[u] if (u in so and u in sc)
                        else (decay_factor * min_score + sc[u] if u in sc else decay_factor * so[u]) for u in union.tolist()])
        k = np.argsort(-new, kind="stable")[:num_candidate_path]
        scores[item] = (union[k], new[k])
    return scores


def streaming_path_scores_dev(engine, sequences, targets, num_candidate_path, decay_factor=0.999, with_occurrence=False):
    """streaming_path_scores on the device (Engine.dr_mstep_streaming_path_scores): search, the per-item fold in ascending
    sample index and the cut at C without the candidates leaving the device.  -> the dict streaming_path_scores returns (and, with
    with_occurrence, {item: number of samples})."""
    off, codes, scores, occ = engine.dr_mstep_streaming_path_scores(sequences, targets, num_candidate_path, decay_factor)
    hit = np.flatnonzero(occ)
    out = {int(v): (codes[off[v]:off[v + 1]], scores[off[v]:off[v + 1]]) for v in hit}
    if not with_occurrence:
        return out
    return out, dict(zip(hit.tolist(), occ[hit].tolist()))


def penalty_func(path_size, poly_order):
    f = lambda s: math.pow(s, poly_order) / poly_order
    return f(path_size + 1) - f(path_size)


def assign_paths(item_path_scores, item_occurrence, all_items, num_iteration, num_path_per_item, K, D, seed=0,
                 penalty_factor=3e-6, penalty_poly_order=4):
    """The coordinate-descent loop of `optimize` (:48-82) -> {item: [J path tuples]}."""
    rng = np.random.default_rng(seed)
    mapping, path_size = {}, {}
    for t in range(1, num_iteration + 1):
        for v in all_items:
            v = int(v)
            if v not in item_occurrence:
                mapping[v] = [int(c) for c in _codes(rng.integers(0, K, size=(num_path_per_item, D)), K)]   # generateRandomPath
                continue
            cc, ss = item_path_scores[v]
            selected, partial = [], 0.0
            nv = item_occurrence[v]
            for j in range(num_path_per_item - 1, -1, -1):
                if t > 1:
                    last = mapping[v][j]
                    path_size[last] = path_size[last] - 1
                best, best_score = None, None
                for code, prob in zip(cc.tolist(), ss.tolist()):
                    if code in selected:
                        continue
                    penalty = penalty_factor * penalty_func(path_size.get(code, 0), penalty_poly_order)
                    g = nv * (math.log1p(prob + partial) - math.log1p(partial)) - penalty
                    if best is None or g > best_score:
                        best, best_score = code, g
                if best is None:
                    raise ValueError("item %d has fewer candidate paths than paths per item" % v)
                path_size[best] = path_size.get(best, 0) + 1
                selected = [best] + selected
                partial = partial + best_score        # the reference accumulates the gain here (CoordinateDescent.scala:76)
            mapping[v] = selected
    return {v: [_decode(c, K, D) for c in codes] for v, codes in mapping.items()}


def decode_codes(codes, K, D):
    """path codes [...] -> node ids [..., D] (code = sum_d node_d * K^(D-1-d)), vectorised"""
    c = np.array(codes, np.int64)
    out = np.empty(c.shape + (D,), np.int64)
    for d in range(D - 1, -1, -1):
        out[..., d] = c % K
        c //= K
    return out


def pack_csr(item_path_scores, item_occurrence, num_item):
    """the dicts of the host routes -> the CSR of the device routes: (item_off [num_item + 1], codes, scores, occurrence [num_item])"""
    cnt = np.zeros(num_item, np.int64)
    occ = np.zeros(num_item, np.int64)
    items = sorted(int(v) for v in item_path_scores)
    for v in items:
        cnt[v] = len(item_path_scores[v][0])
    for v, n in item_occurrence.items():
        occ[int(v)] = n
    off = np.zeros(num_item + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    codes = np.concatenate([np.asarray(item_path_scores[v][0], np.int64) for v in items]) if items else np.zeros(0, np.int64)
    scores = np.concatenate([np.asarray(item_path_scores[v][1], np.float64) for v in items]) if items else np.zeros(0, np.float64)
    return off, codes, scores, occ


def _as_mapping(out_codes, K, D, items=None):
    """[num_item, J] codes -> {item: [J path tuples]} for `items` (None: every item); the decode is one vectorised pass"""
    J = out_codes.shape[1]
    flat = list(map(tuple, decode_codes(out_codes, K, D).reshape(-1, D).tolist()))
    items = range(out_codes.shape[0]) if items is None else items
    return {int(v): flat[int(v) * J:(int(v) + 1) * J] for v in items}


def assign_paths_dev(engine, item_off, codes, scores, occurrence, num_iteration, num_path_per_item, K, D, seed=0, penalty_factor=3e-6,
                     penalty_poly_order=4, all_items=None, as_array=False):
    """assign_paths on the device (Engine.dr_mstep_assign_paths) over the CSR the device path-score routes return.  The hit
    items get what assign_paths gives them (up to the last bits of log1p where two gains nearly tie); the items that never occur draw
    from the library's own counter-based stream, not numpy's.  all_items (None: every item): an item outside it is not visited and its
    row is not handed out.  -> {item: [J path tuples]}, or with as_array=True the codes [num_item, J] int64."""
    occ = np.array(occurrence, np.int64)
    items = None
    if all_items is not None:
        items = np.unique(np.asarray(list(all_items), np.int64))
        if len(items) != len(occ):
            keep = np.zeros(len(occ), bool)
            keep[items] = True
            occ[~keep] = 0
        else:
            items = None
    out = engine.dr_mstep_assign_paths(item_off, codes, scores, occ, K, D, num_path_per_item, num_iteration, penalty_factor, penalty_poly_order, seed)
    return out if as_array else _as_mapping(out, K, D, items)


def optimize(engine, sequences, targets, all_items, num_candidate_path, num_path_per_item, num_iteration=3, train_mode="batch",
             decay_factor=0.999, batch_size=8192, seed=0, penalty_factor=3e-6, penalty_poly_order=4, path_scores="host", assign="host",
             as_array=False):
    """CoordinateDescent.optimize(model, trainMode) -> item -> paths (internal ids).  path_scores="device" (batch mode only) aggregates the
    candidates on the device (batch_path_scores_dev) and takes the item occurrences from the same call; path_scores="device_streaming"
    (streaming mode only) does the same for the decayed running scores (streaming_path_scores_dev).  assign="device" runs the greedy
    assignment on the device too (assign_paths_dev): with a device path_scores and all_items = every item it is ONE call
    (Engine.dr_mstep_optimize), nothing but the result leaves the device; as_array=True (assign="device" only) returns the codes
    [num_item, J] instead of the dict."""
    K, D = engine.dr_dims["K"], engine.dr_dims["D"]
    if path_scores not in ("host", "device", "device_streaming"):
        raise ValueError(path_scores)
    if assign not in ("host", "device"):
        raise ValueError(assign)
    if as_array and assign != "device":
        raise ValueError("as_array=True needs assign=\"device\"")
    if assign == "device":
        if path_scores == "device_streaming" and train_mode != "streaming":
            raise ValueError("path_scores=\"device_streaming\" serves train_mode=\"streaming\" only")
        if path_scores == "device" and train_mode != "batch":
            raise ValueError("path_scores=\"device\" serves train_mode=\"batch\" only (streaming: \"device_streaming\")")
        if train_mode not in ("batch", "streaming"):
            raise ValueError(train_mode)
        num_item = engine.dr_dims["num_item"]
        items = np.unique(np.asarray(list(all_items), np.int64))
        every = len(items) == num_item
        kw = dict(seed=seed, penalty_factor=penalty_factor, penalty_poly_order=penalty_poly_order)
        if path_scores != "host" and every:
            out = engine.dr_mstep_optimize(sequences, targets, num_candidate_path, num_path_per_item, num_iteration, train_mode, decay_factor, **kw)
            return out if as_array else _as_mapping(out, K, D)
        if path_scores == "host":
            sc = (batch_path_scores(engine, sequences, targets, num_candidate_path) if train_mode == "batch" else
                  streaming_path_scores(engine, sequences, targets, num_candidate_path, decay_factor, batch_size))
            tg, cnt = np.unique(np.asarray(targets), return_counts=True)
            csr = pack_csr(sc, dict(zip(tg.tolist(), cnt.tolist())), num_item)
        elif path_scores == "device":
            csr = engine.dr_mstep_path_scores(sequences, targets, num_candidate_path)
        else:
            csr = engine.dr_mstep_streaming_path_scores(sequences, targets, num_candidate_path, decay_factor)
        return assign_paths_dev(engine, *csr, num_iteration, num_path_per_item, K, D, all_items=None if every else items, as_array=as_array, **kw)
    if path_scores == "device_streaming":
        if train_mode != "streaming":
            raise ValueError("path_scores=\"device_streaming\" serves train_mode=\"streaming\" only")
        sc, occ = streaming_path_scores_dev(engine, sequences, targets, num_candidate_path, decay_factor, with_occurrence=True)
        return assign_paths(sc, occ, sorted(int(i) for i in all_items), num_iteration, num_path_per_item, K, D, seed,
                            penalty_factor, penalty_poly_order)
    if path_scores == "device":
        # two spellings, one per mode: tests/test_gpu_dr_mstep.py pins that "device" with train_mode="streaming" raises, so the streaming
        # route is "device_streaming"; folding the two into one is left to whoever edits that test
        if train_mode != "batch":
            raise ValueError("path_scores=\"device\" serves train_mode=\"batch\" only (streaming: \"device_streaming\")")
        sc, occ = batch_path_scores_dev(engine, sequences, targets, num_candidate_path, with_occurrence=True)
        return assign_paths(sc, occ, sorted(int(i) for i in all_items), num_iteration, num_path_per_item, K, D, seed,
                            penalty_factor, penalty_poly_order)
    if train_mode == "batch":
        sc = batch_path_scores(engine, sequences, targets, num_candidate_path)
    elif train_mode == "streaming":
        sc = streaming_path_scores(engine, sequences, targets, num_candidate_path, decay_factor, batch_size)
    else:
        raise ValueError(train_mode)
    tg, cnt = np.unique(np.asarray(targets), return_counts=True)          # computeItemOccurrence (:128-131)
    occ = dict(zip(tg.tolist(), cnt.tolist()))
    return assign_paths(sc, occ, sorted(int(i) for i in all_items), num_iteration, num_path_per_item, K, D, seed,
                        penalty_factor, penalty_poly_order)
