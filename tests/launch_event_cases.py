"""The calls whose event pairs tests/test_gpu_launch_events.py pins, shared with tests/golden/make_launch_event_counts.py: for one call
of the public Engine API, how many pairs of each EvKind (csrc/host_request.hip.inc) the library records.

Every case is (model, switches, before, call): `model` names one of the small engines of Models, `switches` is the environment the call
runs under (the library reads them per call), `before` (or None) prepares what the call needs — a gradient for an Adam step — and is not
counted.  measure() runs before + call once unmeasured, so that copies a handle builds lazily on first use are in place whatever ran
before, then counts the second call.  Shapes are small on purpose: one slab, one chunk, nothing that depends on the number of CUs."""
import os

import numpy as np

import deepfm_ref
from dismember_amd import synth
from helpers import random_din_weights, random_histories, synthetic_tree

KINDS = range(96)             # every number an EvKind has, and the gaps between them
DEPTH, ITEMS, NI = 8, 200, (1 << 9) - 1
U, L = 64, 10
DFM_TIMED = {"DM_DFM_TIME_LAUNCHES": "1"}
DR_TIMED = {"DM_DR_TIME_LAUNCHES": "1"}
DR = dict(E=16, L=4, K=7, D=3, num_item=200)


class Models:
    """the engines of the cases, built on first use and closed together"""

    def __init__(self):
        self._eng = {}
        self.tree = synthetic_tree(np.random.default_rng(21), DEPTH, ITEMS)
        self.seqs = random_histories(np.random.default_rng(22), self.tree["leaf_ids"], U, L)
        self.seqs20 = random_histories(np.random.default_rng(23), self.tree["leaf_ids"], U, 20)
        r = np.random.default_rng(24)
        self.codes = r.integers((1 << DEPTH) - 1, NI, (U, L)).astype(np.int32)       # leaf codes: OTM histories, scorer rows
        self.codes[0, 7:] = -1
        self.row_codes = r.integers(0, NI, U).astype(np.int32)
        self.labels = (r.random(U) < 0.5).astype(np.float32)
        # DeepFM training: 8 users of 8 rows (grouped), the same rows ragged (CSR: one user without rows)
        self.g_seq, self.g_codes, self.g_y = self.codes[:8], self.row_codes.reshape(8, 8), self.labels.reshape(8, 8)
        self.csr_off = np.array([0, 3, 3, 20, 21, 40, 41, 50, 64], np.int64)
        # OTM tree construction: 13 items in nodes of level 4, 0 .. 11 histories each, two levels down
        counts = np.array([(0, 1, 3, 4, 5, 11)[i % 6] for i in range(13)], np.int64)
        self.t_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.t_rows = r.integers(0, NI, (int(self.t_off[-1]), L)).astype(np.int32)
        self.t_node = r.integers(15, 31, 13).astype(np.int32)
        # Deep-Retrieval
        d = DR
        self.dr_seq = r.integers(0, d["num_item"], (U, d["L"])).astype(np.int32)
        self.dr_seq[r.random((U, d["L"])) < 0.2] = -1
        self.dr_paths = r.integers(0, d["K"], (U, d["D"])).astype(np.int32)
        self.dr_targets = r.integers(0, d["num_item"], U).astype(np.int32)

    def get(self, name):
        if name not in self._eng:
            self._eng[name] = getattr(self, "_" + name)()
        return self._eng[name]

    def close(self):
        for e in self._eng.values():
            e.close()
        self._eng = {}

    def _tree_engine(self):
        from dismember_amd import Engine
        eng, t = Engine(0), self.tree
        eng.load_tree(t["codes"], t["ids"], t["is_leaf"], int(t["max_level"]))
        eng.load_id_maps(t["leaf_ids"], t["leaf_codes"])
        return eng

    def _din(self):
        eng = self._tree_engine()
        eng.load_weights_din(random_din_weights(np.random.default_rng(30), 32, NI), 32, NI)
        return eng

    def _din64(self):
        from dismember_amd import Engine
        eng = Engine(0)
        eng.load_weights_din(random_din_weights(np.random.default_rng(31), 32, NI, dtype=np.float64, std=0.2, bias_std=0.1), 32, NI)
        eng.train_init(lr=1e-3)
        return eng

    def _dfm(self):
        eng = self._tree_engine()
        eng.load_weights_deepfm(deepfm_ref.random_deepfm_weights(np.random.default_rng(32), 16, L, NI), 16, L, NI)
        return eng

    def _dfm_train(self):
        eng = self._dfm()
        eng.deepfm_train_init()
        return eng

    def _dr_model(self, train):
        from dismember_amd import Engine
        d, rng = DR, np.random.default_rng(33)
        w = synth.make_dr_model(d["num_item"], d["K"], d["D"], d["L"], d["E"], rng)
        eng = Engine(0)
        eng.dr_load_model(w, d["E"], d["L"], d["K"], d["D"], d["num_item"], dtype=np.float32)
        eng.dr_load_path_items(*synth.dr_path_items(synth.make_dr_paths(d["num_item"], d["K"], d["D"], 2, rng)))
        if train:
            eng.dr_train_init()
            eng.dr_rerank_train_init(8)
        return eng

    def _dr(self):
        return self._dr_model(False)

    def _dr_sliced(self):
        """the column-sliced search on this small batch: DM_DR_SLICED_MIN_USERS is read when the model is loaded"""
        os.environ["DM_DR_SLICED_MIN_USERS"] = "1"
        try:
            return self._dr_model(False)
        finally:
            os.environ.pop("DM_DR_SLICED_MIN_USERS", None)

    def _dr_train(self):
        return self._dr_model(True)


def _f32_search(e, m, users=U):
    e.set_scorer_mode("f32")
    try:
        e.tdm_beam_search(m.seqs[:users], 16, 10)
    finally:
        e.set_scorer_mode("auto")


def _umask(seq):
    um = np.zeros(len(seq), np.uint32)
    for j in range(seq.shape[1]):
        um |= (seq[:, j] == -1).astype(np.uint32) << np.uint32(j)
    return um


_dfm_rows = lambda e, m: e.deepfm_train_forward_backward(m.row_codes, m.codes, m.labels)
_dfm_grouped = lambda e, m: e.deepfm_train_forward_backward_grouped(m.g_seq, m.g_codes, m.g_y)
_dfm_csr = lambda e, m: e.deepfm_train_forward_backward_csr(m.g_seq, m.csr_off, m.row_codes, m.labels)
_dr_step = lambda e, m: e.dr_train_forward_backward(m.dr_seq, m.dr_paths)
_dr_rerank = lambda e, m: e.dr_rerank_forward_backward(m.dr_seq, m.dr_targets)

# name: (model, switches, before, call)
CASES = {
    "din-tdm-auto": ("din", {}, None, lambda e, m: e.tdm_beam_search(m.seqs, 16, 10)),
    "din-tdm-f32": ("din", {}, None, _f32_search),
    "din-tdm-single-user": ("din", {}, None, lambda e, m: e.tdm_beam_search(m.seqs[:1], 16, 10)),      # the one-wave kernel: staged, with its pairs
    "din-tdm-single-user-direct": ("din", {}, None, lambda e, m: _f32_search(e, m, 1)),      # the single-request path: one launch and no pair
    "din-forward": ("din", {}, None, lambda e, m: e.din_forward(m.row_codes[1:], m.codes[1:])),      # (row 0 holds padding)
    "din-otm": ("din", {}, None, lambda e, m: e.otm_beam_search(m.codes, 12, DEPTH)),
    "din-bruteforce": ("din", {}, None, lambda e, m: e.tdm_bruteforce_topk(m.seqs, 10)),
    "din-tdm-long-pipeline": ("din", {"DM_LONG_PIPELINE": "1"}, None, lambda e, m: e.tdm_beam_search(m.seqs20, 16, 10)),
    "din64-train-grouped": ("din64", {}, None,
                            lambda e, m: e.train_forward_backward_grouped(m.g_seq, _umask(m.g_seq), m.g_codes, m.g_y)),
    "dfm-forward": ("dfm", {}, None, lambda e, m: e.deepfm_forward(m.row_codes, m.codes)),
    "dfm-tdm": ("dfm", {}, None, lambda e, m: e.tdm_beam_search(m.seqs, 16, 10, use_mask=False)),
    "dfm-pairs-forward": ("dfm", {}, None, lambda e, m: e.deepfm_pairs_forward(m.row_codes, m.codes[:16], seq_div=4)),
    "dfm-otm": ("dfm", {}, None, lambda e, m: e.otm_beam_search(m.codes, 12, DEPTH)),
    "dfm-otm-child-weights": ("dfm", {}, None, lambda e, m: e.deepfm_otm_child_weights(m.t_off, m.t_rows, m.t_node, 4, 6)),
}
for _tag, _env in (("", {}), ("-timed", DFM_TIMED)):
    CASES.update({
        "dfm-train-rows" + _tag: ("dfm_train", _env, None, _dfm_rows),
        "dfm-train-grouped" + _tag: ("dfm_train", _env, None, _dfm_grouped),
        "dfm-train-csr" + _tag: ("dfm_train", _env, None, _dfm_csr),
        "dfm-adam" + _tag: ("dfm_train", _env, _dfm_rows, lambda e, m: e.deepfm_adam_step(1.0)),
    })
for _tag, _env in (("", {}), ("-timed", DR_TIMED)):
    CASES.update({
        "dr-beam" + _tag: ("dr", _env, None, lambda e, m: e.dr_beam_search(m.dr_seq, 5)),
        "dr-beam-sliced" + _tag: ("dr_sliced", _env, None, lambda e, m: e.dr_beam_search(m.dr_seq, 5)),
        "dr-recommend" + _tag: ("dr", _env, None, lambda e, m: e.dr_recommend(m.dr_seq, 5, 10)),
        "dr-mstep" + _tag: ("dr", _env, None, lambda e, m: e.dr_mstep_path_scores(m.dr_seq, m.dr_targets, 5)),
        "dr-train" + _tag: ("dr_train", _env, None, _dr_step),
        "dr-rerank-train" + _tag: ("dr_train", _env, None, _dr_rerank),
        "dr-adam" + _tag: ("dr_train", _env, _dr_step, lambda e, m: e.dr_adam_step(1.0)),
        "dr-rerank-adam" + _tag: ("dr_train", _env, _dr_rerank, lambda e, m: e.dr_rerank_adam_step(1.0)),
    })
SWITCHES = ("DM_LONG_PIPELINE", "DM_DFM_TIME_LAUNCHES", "DM_DR_TIME_LAUNCHES")


def measure(models, name, setenv, delenv):
    """{"total": pairs of the call, "<kind>": pairs of that kind, for the kinds that have any}; setenv(name, value) / delenv(name) set and
    unset a switch (monkeypatch's, or os.environ's)"""
    model, env, before, call = CASES[name]
    eng = models.get(model)
    for s in SWITCHES:
        if s in env:
            setenv(s, env[s])
        else:
            delenv(s)
    for counted in (False, True):
        if before is not None:
            before(eng, models)
        eng.timing_reset()
        call(eng, models)
    out = {"total": eng.timing_get()[0]}
    for k in KINDS:
        n = eng.timing_get_kind(k)[0]
        if n:
            out[str(k)] = n
    return out
