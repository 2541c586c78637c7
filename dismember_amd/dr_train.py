"""Deep-Retrieval E-step over the device training step: `LocalOptimizer.optimize`'s layer-model half
(deep-retrieval/src/main/scala/com/mass/dr/optim/LocalOptimizer.scala:58-116) — expand every sample by the J paths of its target
item (dataset/MiniBatch.scala:18-50, transformLayerData), one forward/backward, one Adam step.  The rerank model is not trained here.

One E-step / M-step round on an engine that holds a Deep-Retrieval model (`Engine.dr_load_model`):

    from dismember_amd import dr_mstep
    from dismember_amd.dr_train import DRTrainer

    trainer = DRTrainer(engine, item_paths, lr=1e-3)            # item_paths [num_item, J, D]
    for seqs, targets in batches:                                # E-step: fit the layer model to the current paths
        trainer.step(seqs, targets)
    print(trainer.losses[-1])                                    # per-layer cross-entropy of the last batch
    new_paths = dr_mstep.optimize(engine, all_seqs, all_targets, range(num_item),      # M-step: re-assign the paths from a
                                  num_candidate_path=20, num_path_per_item=J)          # beam search over the TRAINED weights
    trainer.set_item_paths(np.array([new_paths[i] for i in range(num_item)]))

The first search after a step rebuilds the search's derived copies of the weights; steps in between do not.
"""
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


class DRTrainer:
    """Trains the layer model of the Deep-Retrieval model `engine` holds.  item_paths [num_item, J, D] int: the current item -> paths
    mapping (MappingOp.itemPathMapping).  `losses` collects the per-layer loss [D] of every step."""

    def __init__(self, engine, item_paths, lr=1e-3, lr_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
        self.engine = engine
        self.set_item_paths(item_paths)
        self.losses = []
        engine.dr_train_init(lr=lr, lr_decay=lr_decay, beta1=beta1, beta2=beta2, eps=eps)

    def set_item_paths(self, item_paths):
        p = np.ascontiguousarray(item_paths, np.int32)
        d = self.engine.dr_dims
        if p.ndim != 3 or p.shape[0] != d["num_item"] or p.shape[2] != d["D"]:
            raise ValueError("item_paths must be [num_item, J, D]")
        self.item_paths = p

    def step(self, seqs, targets):
        """one batch: expand by the targets' paths, forward/backward, Adam -> per-layer losses [D]"""
        seq, paths = expand_batch(seqs, targets, self.item_paths)
        loss = self.engine.dr_train_forward_backward(seq, paths)
        self.engine.dr_adam_step(1.0)
        self.losses.append(loss)
        return loss

    def weights(self):
        d = self.engine.dr_dims
        return split_params(self.engine.dr_train_download("weights"), d["E"], d["L"], d["K"], d["D"], d["num_item"])

    def close(self):
        self.engine.dr_train_free()
