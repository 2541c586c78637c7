"""Deep-Retrieval E-step over the device training steps: `LocalOptimizer.optimize`
(deep-retrieval/src/main/scala/com/mass/dr/optim/LocalOptimizer.scala:58-133).  The layer model: expand every sample by the J paths of
its target item (dataset/MiniBatch.scala:18-50, transformLayerData), one forward/backward, one Adam step.  With `rerank=True` the rerank
model follows on the same batch, as the reference trains both on every mini-batch: sampled softmax over the target and `num_sampled`
negatives, its own two Adam updates (scalann nn/SampledSoftmaxLoss.scala).

One E-step / M-step round on an engine that holds a Deep-Retrieval model (`Engine.dr_load_model`):

    from dismember_amd import dr_mstep
    from dismember_amd.dr_train import DRTrainer

    trainer = DRTrainer(engine, item_paths, lr=1e-3)            # item_paths [num_item, J, D]
    for seqs, targets in batches:                                # E-step: fit the layer model to the current paths
        trainer.step(seqs, targets)
    print(trainer.losses[-1])                                    # per-layer cross-entropy of the last batch
    new_paths = dr_mstep.optimize(engine, all_seqs, all_targets, range(num_item),      # M-step: re-assign the paths from a
                                  num_candidate_path=20, num_path_per_item=J,          # beam search over the TRAINED weights;
                                  path_scores="device")                                # the candidates never leave the device
    trainer.set_item_paths(np.array([new_paths[i] for i in range(num_item)]))

The streaming M-step (`cd.train_mode streaming`, configs/c5_dr_10m.conf) has its own device route: `train_mode="streaming",
decay_factor=0.999, path_scores="device_streaming"` folds every item's decayed running scores on the device.

The first search after a step rebuilds the search's derived copies of the weights; steps in between do not.

Data-parallel: every rank holds a replica and passes the SAME global batch to `step`; the trainer slices it as
LocalOptimizer.trainLayerBatch does, exchanges the layer model's gradients (`Engine.dr_train_sync_gradients`) and steps with 1 / P:

    trainer = DRTrainer(engine, item_paths, lr=1e-3, comm=Comm.from_env())
    trainer.step(seqs, targets)                                  # the mean loss over the workers, the same on every rank

The sample-grouped layer step takes every sample once with its J paths instead of the expanded batch: the same
gradient re-associated, each history product computed once per sample (opt-in, also by DM_DR_TRAIN_GROUPED=1).  The evaluation losses:

    trainer = DRTrainer(engine, item_paths, lr=1e-3, grouped=True)
    trainer.evaluate_layer(eval_seqs, eval_targets)              # Evaluator.evaluateLayerModel: per-layer cross-entropy [D]
    evaluation.evaluate_dr(engine, eval_seqs, labels, users, consumed, topk, beam, loss_fn=trainer.eval_loss_fn(eval_seqs, eval_targets))

Both halves, served end to end:

    trainer = DRTrainer(engine, item_paths, lr=1e-3, rerank=True, num_sampled=20, seed=1)
    for seqs, targets in batches:
        layer_loss, rerank_loss = trainer.step(seqs, targets)
    print(trainer.evaluate_rerank(eval_seqs, eval_targets))      # Evaluator.evaluateReRankModel: the full softmax
    engine.dr_recommend(user_seqs, beam, topk)                   # reads the trained rerank arrays in place
"""
import os

import numpy as np


def param_sections(E, L, K, D, num_item):
    """name -> (start, stop) in the trainable vector [layer_emb ; W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}]"""
    out, o = {}, 0
    for name, n in [("emb", (num_item + K * (D - 1)) * E)] + [x for d in range(D) for x in (("W%d" % d, K * (L + d) * E), ("b%d" % d, K))]:
        out[name] = (o, o + n)
        o += n
    return out


def split_params(vec, E, L, K, D, num_item):
    """the trainable vector -> dict(layer_emb, layer_w [D], layer_b [D]) as dr_load_model takes them"""
    sec = param_sections(E, L, K, D, num_item)
    v = lambda n: vec[slice(*sec[n])]
    return dict(layer_emb=v("emb").reshape(-1, E), layer_w=[v("W%d" % d).reshape(K, (L + d) * E) for d in range(D)],
                layer_b=[v("b%d" % d) for d in range(D)])


def pack_params(weights, dtype=np.float64):
    return np.concatenate([np.asarray(weights["layer_emb"], dtype).ravel()] +
                          [np.asarray(a, dtype).ravel() for w, b in zip(weights["layer_w"], weights["layer_b"]) for a in (w, b)])


def expand_batch(seqs, targets, item_paths):
    """transformLayerData: one row per (sample, path of its target item) -> (seq_ids [B*J, L], paths [B*J, D])"""
    seqs = np.ascontiguousarray(seqs, np.int32)
    tg = np.asarray(targets, np.int64)
    J = item_paths.shape[1]
    return np.repeat(seqs, J, axis=0), np.ascontiguousarray(item_paths[tg].reshape(len(tg) * J, -1), np.int32)


def layer_slices(B, W):
    """LocalOptimizer.trainLayerBatch (LocalOptimizer.scala:135-166): how a mini-batch of B samples is split over W workers ->
    ([(offset, length)] per worker, P = the workers that get a sample: W, or B when B < W)"""
    task, extra = B // W, B % W
    return [(i * task + min(i, extra), task + (1 if i < extra else 0)) for i in range(W)], (extra if task == 0 else W)


def init_rerank_weights(num_item, L, E, rng, dtype=np.float64):
    """The five rerank arrays as the reference's modules initialise them: Embedding and Linear weights and softmaxWeights N(0, 0.05)
    (scalann nn/Embedding.scala:20, nn/Linear.scala:12, RerankModel.scala:15), the Linear bias and softmaxBiases zero (Linear.scala:13,
    RerankModel.scala:16).  rng: a numpy Generator."""
    n = lambda *shape: (rng.standard_normal(shape) * 0.05).astype(dtype)
    return dict(rerank_emb=n(num_item, E), rerank_w=n(E, L * E), rerank_b=np.zeros(E, dtype),
                softmax_w=n(num_item, E), softmax_b=np.zeros(num_item, dtype))


def init_layer_weights(num_item, L, K, D, E, rng, dtype=np.float64):
    """The layer model's arrays as LayerModel.scala:22-39 initialises them: the shared embedding table [(num_item + K (D - 1)) x E] and
    every Linear weight [K x (L + d) E] N(0, 0.05) (scalann nn/EmbeddingShare.scala:21, nn/Linear.scala:12), the Linear biases zero
    (Linear.scala:13).  rng: a numpy Generator."""
    n = lambda *shape: (rng.standard_normal(shape) * 0.05).astype(dtype)
    return dict(layer_emb=n(num_item + K * (D - 1), E), layer_w=[n(K, (L + d) * E) for d in range(D)], layer_b=[np.zeros(K, dtype) for _ in range(D)])


def split_rerank(graph, softmax, E, L, num_item):
    """the two trainable vectors [rerank_emb ; rerank_w ; rerank_b] and [softmax_w ; softmax_b] -> the five arrays of dr_load_model"""
    a, b = num_item * E, num_item * E + E * L * E
    return dict(rerank_emb=graph[:a].reshape(num_item, E), rerank_w=graph[a:b].reshape(E, L * E), rerank_b=graph[b:],
                softmax_w=softmax[:a].reshape(num_item, E), softmax_b=softmax[a:])


def pack_rerank(weights, dtype=np.float64):
    f = lambda k: np.asarray(weights[k], dtype).ravel()
    return np.concatenate([f("rerank_emb"), f("rerank_w"), f("rerank_b")]), np.concatenate([f("softmax_w"), f("softmax_b")])


class DRTrainer:
    """Trains the Deep-Retrieval model `engine` holds.  item_paths [num_item, J, D] int: the current item -> paths mapping
    (MappingOp.itemPathMapping).  `losses` collects the per-layer loss [D] of every step.

    rerank=True also trains the rerank model (the engine's model must hold the five rerank arrays): num_sampled negatives per row drawn
    on the device from `seed`; accumulate=True is the reference's never-cleared softmax-table gradient, False clears it per
    batch; rerank_epochs: the reference's reRankStoppingEpoch — the rerank step runs while `epoch` (1-based, advanced by next_epoch())
    is <= rerank_epochs (None: always).  `rerank_losses` collects its loss per step (NaN once stopped).  The rerank optimizer takes the
    layer optimizer's options (one learning rate in the reference's conf); its softmax tables take the criterion's own (eps 1e-7, no decay).

    comm (a dismember_amd.comm.Comm, None: one worker): data-parallel training of the LAYER model.  Every rank passes the same global
    (seqs, targets) to step(); rank i trains its slice (layer_slices), the gradients are exchanged (Engine.dr_train_sync_gradients: the
    rank-ordered sum, so the replicas stay bit-identical) and the Adam step divides by P, the number of ranks that had a sample.  step()
    returns the mean of those ranks' losses (LocalOptimizer.scala:164-165).  The RERANK model is not split: as in the reference every
    step trains it on the whole batch, here on every rank with the same seed — deterministic step and sampler keep those replicas
    identical too, and this half does not get faster with more ranks.  All ranks must pass the same seed (ValueError otherwise).
    sync_s / sync_calls: wall time spent in the exchange and the number of exchanges.

    grouped (None: DM_DR_TRAIN_GROUPED=1 in the environment, otherwise False): the layer step takes every sample once with its J paths
    (Engine.dr_train_forward_backward_grouped) instead of the batch expanded by np.repeat: the same gradient re-associated,
    each history product computed once per sample.  Losses, the exchange and 1 / P are as in the row step."""

    def __init__(self, engine, item_paths, lr=1e-3, lr_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8, rerank=False, num_sampled=None, seed=0,
                 accumulate=True, rerank_epochs=None, comm=None, grouped=None, resident=False):
        self.engine = engine
        self.comm = comm
        self.resident = bool(resident)
        self.grouped = os.environ.get("DM_DR_TRAIN_GROUPED") == "1" if grouped is None else bool(grouped)
        self.sync_s, self.sync_calls = 0.0, 0
        self.set_item_paths(item_paths)
        self.losses = []
        self.rerank = bool(rerank)
        self.rerank_losses = []
        self.rerank_epochs = rerank_epochs
        self.epoch = 1
        engine.dr_train_init(lr=lr, lr_decay=lr_decay, beta1=beta1, beta2=beta2, eps=eps)
        if self.rerank:
            if num_sampled is None:
                raise ValueError("rerank=True needs num_sampled")
            if comm is not None:          # (a collective: every rank raises, or none)
                # the sampler's seed is 64 bits wide and the allreduce carries doubles: compare the two 32-bit halves, each exact
                halves = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], np.float64)
                hi, lo = comm.allreduce(halves, "max"), -comm.allreduce(-halves, "max")
                if not np.array_equal(hi, lo):
                    raise ValueError("DRTrainer: every rank must pass the same seed with rerank=True (the rerank replicas draw the same negatives)")
            engine.dr_rerank_train_init(num_sampled, seed=seed, accumulate=accumulate, lr=lr, lr_decay=lr_decay, beta1=beta1, beta2=beta2, eps=eps)
        if comm is not None:
            engine.attach_comm(comm)

    def set_item_paths(self, item_paths):
        p = np.ascontiguousarray(item_paths, np.int32)
        d = self.engine.dr_dims
        if p.ndim != 3 or p.shape[0] != d["num_item"] or p.shape[2] != d["D"]:
            raise ValueError("item_paths must be [num_item, J, D]")
        self.item_paths = p
        if self.resident:
            self.engine.dr_set_item_paths(p)

    def load_set(self, seqs, targets):
        """resident=True: the training set goes to the device once (Engine.dr_train_set_load); step_range() trains on ranges of it"""
        self._need_resident("load_set")
        self.engine.dr_train_set_load(seqs, targets)
        self.set_size = len(np.asarray(targets).reshape(-1))

    def shuffle(self, seed):
        """the order of the trainer's current epoch (Engine.dr_train_set_shuffle(seed, epoch))"""
        self._need_resident("shuffle")
        self.engine.dr_train_set_shuffle(seed, self.epoch)

    def _need_resident(self, what):
        if not self.resident:
            raise ValueError("DRTrainer.%s needs resident=True" % what)

    def step_range(self, offset, length):
        """step() on samples order[offset : offset + length] of the resident set: nothing but the range goes to the device.  With a
        communicator the range is sliced by layer_slices, exchanged and stepped with 1 / P as step() does with its batch."""
        self._need_resident("step_range")
        return self._step(length, lambda lo, n: self.engine.dr_train_set_forward_backward(offset + lo, n, grouped=self.grouped),
                          lambda: self.engine.dr_train_set_rerank_forward_backward(offset, length), "step_range")

    def step(self, seqs, targets):
        """one batch: expand by the targets' paths, forward/backward, Adam -> per-layer losses [D]; with rerank=True the rerank step
        follows on the unexpanded batch -> (per-layer losses [D], sampled-softmax loss)"""
        if self.comm is not None:
            seqs, targets = np.asarray(seqs), np.asarray(targets)
        return self._step(len(targets), lambda lo, n: self._forward_backward(seqs[lo:lo + n], targets[lo:lo + n]),
                          lambda: self.engine.dr_rerank_forward_backward(seqs, targets), "step")

    def _step(self, B, layer_fb, rerank_fb, who):
        """what step() and step_range() share.  layer_fb(lo, n): the layer model's forward/backward on samples [lo, lo + n) of the B
        of this step; rerank_fb(): the rerank model's on all of them.  One worker: the whole batch and Adam.  With a communicator,
        trainLayerBatch + syncGradients: this rank's slice, the exchange, Adam with 1 / P -> the mean loss of the P working ranks."""
        if self.comm is None:
            loss = layer_fb(0, B)
            self.engine.dr_adam_step(1.0)
        else:
            import time
            slices, P = layer_slices(B, self.comm.world)
            if P == 0:
                raise ValueError("DRTrainer.%s: empty batch" % who)
            lo, n = slices[self.comm.rank]
            loss = np.zeros(self.engine.dr_dims["D"], np.float64)
            if n > 0:                     # (a rank past P runs no step: it enters the exchange with no rows and a zero dense part)
                loss = layer_fb(lo, n)
            t0 = time.perf_counter()
            self.engine.dr_train_sync_gradients()
            self.sync_s += time.perf_counter() - t0; self.sync_calls += 1
            self.engine.dr_adam_step(1.0 / P)
            loss = self.comm.allreduce(loss) / P
        self.losses.append(loss)
        if not self.rerank:
            return loss
        rr = float("nan")
        if self.rerank_epochs is None or self.epoch <= self.rerank_epochs:
            rr = rerank_fb()
            self.engine.dr_rerank_adam_step(1.0)
        self.rerank_losses.append(rr)
        return loss, rr

    def _forward_backward(self, seqs, targets):
        """the layer model's forward/backward on (seqs, targets): grouped, every sample once with the [J, D] paths of its target; otherwise
        the batch expanded to one row per path"""
        if self.grouped:
            return self.engine.dr_train_forward_backward_grouped(seqs, self.item_paths[np.asarray(targets, np.int64)])
        return self.engine.dr_train_forward_backward(*expand_batch(seqs, targets, self.item_paths))

    def mstep(self, seqs, targets, num_candidate_path, num_iteration=3, assign="host", **kw):
        """the M-step of one E/M round: dr_mstep.optimize over every item with the trained weights (the number of paths per item stays),
        and the new mapping becomes the trainer's.  assign="device" runs the greedy assignment on the device as well;
        kw: optimize's other arguments (train_mode, path_scores, decay_factor, seed, penalty_factor, penalty_poly_order).
        -> the new item_paths [num_item, J, D]

        resident=True: Engine.dr_train_set_mstep over the RESIDENT set in storage order, both halves on the device.  seqs and targets
        must then be None (the set is the one load_set uploaded), assign is not looked at, and kw may hold train_mode, decay_factor,
        seed, penalty_factor and penalty_poly_order only (path_scores has no meaning there): anything else is a ValueError."""
        from dismember_amd import dr_mstep
        d = self.engine.dr_dims
        if self.resident:
            if seqs is not None or targets is not None:
                raise ValueError("DRTrainer.mstep with resident=True runs over the set load_set uploaded: pass seqs=None, targets=None")
            extra = set(kw) - {"train_mode", "decay_factor", "seed", "penalty_factor", "penalty_poly_order"}
            if extra:
                raise ValueError("DRTrainer.mstep with resident=True does not take %s" % ", ".join(sorted(extra)))
            return self._mstep_resident(num_candidate_path, num_iteration, **kw)
        m = dr_mstep.optimize(self.engine, seqs, targets, range(d["num_item"]), num_candidate_path, self.item_paths.shape[1], num_iteration,
                              assign=assign, **kw)
        self.set_item_paths(np.array([m[i] for i in range(d["num_item"])], np.int32))
        return self.item_paths

    def _mstep_resident(self, num_candidate_path, num_iteration, train_mode="batch", decay_factor=0.999, penalty_factor=3e-6, penalty_poly_order=4, seed=0):
        """Engine.dr_train_set_mstep over the resident set (storage order): table and CSR follow on the device, the host copy from its codes"""
        d = self.engine.dr_dims
        codes = self.engine.dr_train_set_mstep(num_candidate_path, num_iteration, train_mode, decay_factor, penalty_factor, penalty_poly_order, seed)
        p = np.empty(codes.shape + (d["D"],), np.int32)
        for k in range(d["D"] - 1, -1, -1):
            p[..., k] = codes % d["K"]
            codes = codes // d["K"]
        self.item_paths = p
        return self.item_paths

    def next_epoch(self):
        self.epoch += 1

    def evaluate_rerank(self, seqs, targets):
        """Evaluator.evaluateReRankModel: the full-softmax loss of the rerank model on (seqs, targets)"""
        return self.engine.dr_rerank_full_loss(seqs, targets)

    def evaluate_layer(self, seqs, targets):
        """Evaluator.evaluateLayerModel: the per-layer cross-entropy [D] of (seqs, targets) under the current item -> paths mapping"""
        return self.engine.dr_layer_loss(seqs, self.item_paths[np.asarray(targets, np.int64)])

    def eval_loss_fn(self, eval_seqs, eval_targets):
        """-> the loss_fn(off, n) evaluation.evaluate_dr takes: (layer losses [D], rerank loss) of eval samples [off, off + n); the rerank
        loss is the full softmax's when the trainer trains the rerank model, otherwise 0"""
        seqs, targets = np.asarray(eval_seqs), np.asarray(eval_targets)

        def loss_fn(off, n):
            s, t = seqs[off:off + n], targets[off:off + n]
            return self.evaluate_layer(s, t).tolist(), (self.evaluate_rerank(s, t) if self.rerank else 0.0)
        return loss_fn

    def rerank_weights(self):
        """the five rerank arrays as dr_load_model takes them"""
        d = self.engine.dr_dims
        return split_rerank(self.engine.dr_rerank_download("graph"), self.engine.dr_rerank_download("softmax"), d["E"], d["L"], d["num_item"])

    def weights(self):
        d = self.engine.dr_dims
        return split_params(self.engine.dr_train_download("weights"), d["E"], d["L"], d["K"], d["D"], d["num_item"])

    def close(self):
        self.engine.dr_train_free()
        if self.rerank:
            self.engine.dr_rerank_train_free()
