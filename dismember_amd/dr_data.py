"""The Deep-Retrieval data set: `LocalDataSet` (deep-retrieval/src/main/scala/com/mass/dr/dataset/LocalDataSet.scala) restated.

    ds = DRDataSet(sample, num_layer, num_node, num_path_per_item, train_batch_size, eval_batch_size, seq_len, min_seq_len, split_ratio,
                   initialize_mapping=True, rng=np.random.default_rng(0))
    ds.item_id_map          original item id -> internal id (itemIdMapping)
    ds.item_paths           [num_item, J, D] (itemPathMapping: drawn like MappingOp.initItemPathMapping, or read from the mapping file)
    ds.train_seqs / ds.train_targets, ds.eval_seqs / ds.eval_labels / ds.eval_users, ds.user_consumed

`sample` is what tasks._read_interactions returns (user, item, timestamp columns in file order).  Per user (generateData, :81-124): the
items in a STABLE sort by timestamp (sortBy), distinct keeping the first occurrence, mapped to internal ids; then
    n <= min_seq_len        consumed only
    n == min_seq_len + 1    one training sample: the padded first n - 1 items -> the last
    longer                  splitPoint = ceil((n - min_seq_len) split_ratio); sliding windows of seq_len + 1 over the padded items up to
                            splitPoint + seq_len are the training samples; the rest are the eval labels, minus the items consumed in
                            the training part; a user whose labels all vanish has no eval sample; consumed = the training part.
The reference walks the users in the order of a hash map's groupBy, which no file pins down: here they are visited in ascending user
id.  The padding id is -1.  An eval sample's target (for the eval losses) is its first label (DRSample.scala).
"""
import math

import numpy as np

PADDING = -1


def user_items(sample):
    """user -> the user's original item ids, stable-sorted by timestamp, distinct keeping the first; users ascending"""
    by_user = {}
    for u, i, t in zip(sample["user"], sample["item"], sample["timestamp"]):
        by_user.setdefault(int(u), []).append((int(t), int(i)))
    out = {}
    for u in sorted(by_user):
        seen, items = set(), []
        for _, i in sorted(by_user[u], key=lambda x: x[0]):      # (sorted is stable, as sortBy is)
            if i not in seen:
                seen.add(i); items.append(i)
        out[u] = items
    return out


def first_appearance_mapping(sample):
    """initData.map(_.item).distinct.zipWithIndex: original id -> internal id in first-appearance order"""
    m = {}
    for i in sample["item"]:
        m.setdefault(int(i), len(m))
    return m


def generate_data(sample, item_id_map, seq_len, min_seq_len, split_ratio):
    """-> (user_consumed {user: [internal ids]}, train [(seq, target)], eval [(seq, labels, user)])"""
    if not (seq_len > 0 and min_seq_len > 0 and seq_len >= min_seq_len):
        raise ValueError("requirement failed: seqLen > 0 && minSeqLen > 0 && seqLen >= minSeqLen")
    consumed, train, evals = {}, [], []
    pad = [PADDING] * (seq_len - min_seq_len)
    for user, orig in user_items(sample).items():
        items = [item_id_map[i] for i in orig]
        n = len(items)
        if n <= min_seq_len:
            consumed[user] = items
        elif n == min_seq_len + 1:
            consumed[user] = items
            train.append((pad + items[:-1], items[-1]))
        else:
            full = pad + items
            split = int(math.ceil((n - min_seq_len) * split_ratio))
            part = full[:split + seq_len]
            for a in range(0, len(part) - seq_len):
                w = part[a:a + seq_len + 1]
                train.append((w[:-1], w[-1]))
            consumed[user] = items[:split + min_seq_len]
            cset = set(consumed[user])
            labels = [x for x in full[split + seq_len:] if x not in cset]
            if labels:
                evals.append((part[-seq_len:], labels, user))
    return consumed, train, evals


class DRDataSet:
    def __init__(self, sample, num_layer, num_node, num_path_per_item, train_batch_size, eval_batch_size, seq_len, min_seq_len, split_ratio,
                 initialize_mapping=True, mapping_path=None, rng=None):
        self.num_layer, self.num_node, self.num_path_per_item = num_layer, num_node, num_path_per_item
        self.seq_len, self.train_batch_size, self.eval_batch_size = seq_len, train_batch_size, eval_batch_size
        if initialize_mapping:
            self.item_id_map = first_appearance_mapping(sample)
            rng = rng or np.random.default_rng(0)
            # MappingOp.initItemPathMapping (MappingOp.scala:30-43): num_path_per_item paths of num_layer uniform nodes per item
            self.item_paths = rng.integers(0, num_node, size=(len(self.item_id_map), num_path_per_item, num_layer), dtype=np.int32)
        else:
            from . import dr_io
            m = dr_io.read_mapping(mapping_path)
            self.item_id_map = dict(zip(m["items"].tolist(), m["ids"].tolist()))
            self.item_paths = np.zeros((len(self.item_id_map),) + m["paths"].shape[1:], np.int32)
            self.item_paths[m["ids"]] = m["paths"]
        self.num_item = len(self.item_id_map)
        self.id_item_map = {v: k for k, v in self.item_id_map.items()}
        self.user_consumed, train, evals = generate_data(sample, self.item_id_map, seq_len, min_seq_len, split_ratio)
        self.train_seqs = np.array([t[0] for t in train], np.int32).reshape(-1, seq_len)
        self.train_targets = np.array([t[1] for t in train], np.int32)
        self.eval_seqs = np.array([e[0] for e in evals], np.int32).reshape(-1, seq_len)
        self.eval_labels = [e[1] for e in evals]
        self.eval_users = np.array([e[2] for e in evals], np.int64)
        self.eval_targets = np.array([e[1][0] for e in evals], np.int32)
        # iteratorMiniBatch (:55-79): a batch is that many TARGETS, each expanded by its paths
        self.num_targets_per_batch = max(1, train_batch_size // num_path_per_item)
        self.num_eval_targets_per_batch = max(1, eval_batch_size // num_path_per_item)

    @property
    def train_size(self):
        return len(self.train_targets)
