"""TDMClusterTree: re-cluster the items by their learnt embeddings into a new tree, on the device.

    python -m dismember_amd.cluster --tdmConfFile configs/c1_tdm_movielens.conf [--quiet]

  RecursiveCluster  <- tdm/src/main/scala/com/mass/tdm/cluster/RecursiveCluster.scala:18-60 (run), :141-198 (cluster / balanceTree)
  read_embeddings   <- RecursiveCluster.readFile: `id, v, v, ...` lines
  write_embeddings  <- Serialization.saveEmbeddings (tdm/.../utils/Serialization.scala:15-58), DecimalFormat("###.############")
  tdm_cluster_tree  <- examples/.../tdm/TDMClusterTree.scala: the `cluster` block of the conf file

The recursion itself — 2-means per node with `cluster_num` restarts, the balanced split by distance to centroid 0, down to single
items — is one library call (dm_cluster_tree / dm_cluster_tree_model, dismember_amd/csrc/cluster.hip.inc).  `cluster_num` is a
RESTART count (smile's PartitionClustering.run), as in the reference; its conf files' `cluster_iter` line is read by nobody there
and by nobody here.  Only `cluster_type kmeans` is built: `spectral` (smile + ARPACK) raises ValueError.
"""
import sys
import time
from decimal import Decimal

import numpy as np

from . import conf as C
from . import tree_io


def _fmt(v):
    """DecimalFormat("###.############") of one float: up to 12 fraction digits (half-even), no exponent, no grouping."""
    s = format(Decimal(float(v)).quantize(Decimal("1e-12")), "f")
    s = s.rstrip("0").rstrip(".")
    if s in ("-0", "", "-"):
        s = "-0" if s.startswith("-") else "0"
    return s


def write_embeddings(path, ids, embeddings):
    ids = np.asarray(ids).ravel()
    emb = np.asarray(embeddings)
    order = np.argsort(ids, kind="stable")
    with open(path, "w") as f:
        for i in order.tolist():
            f.write("%d" % int(ids[i]))
            f.write("".join(", " + _fmt(x) for x in emb[i].tolist()))
            f.write("\n")


def read_embeddings(path):
    """-> (ids int32 [n], embeddings float32 [n, E])."""
    ids, rows = [], []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            parts = line.split(",")
            ids.append(int(parts[0].strip()))
            rows.append([float(x) for x in parts[1:]])
    return np.asarray(ids, np.int32), np.asarray(rows, np.float64).astype(np.float32)


class RecursiveCluster:
    def __init__(self, engine, ids, embeddings=None, cluster_iter_num=10, cluster_type="kmeans", seed=2024, max_iter=100, tol=1e-4):
        """embeddings=None: the rows of the engine's loaded model at the items' current leaf codes."""
        if cluster_type not in ("kmeans", "spectral"):
            raise ValueError("clusterType must be one of ('kmeans', 'spectral')")
        if cluster_type == "spectral":
            raise ValueError("cluster_type spectral is not built (smile + ARPACK in the reference); use kmeans")
        self.engine = engine
        self.ids = np.asarray(ids, np.int32).ravel()
        self.embeddings = None if embeddings is None else np.ascontiguousarray(embeddings, np.float32)
        if self.embeddings is not None and self.embeddings.shape[0] != self.ids.size:
            raise ValueError("ids and embeddings differ in length")
        self.restarts, self.seed, self.max_iter, self.tol = int(cluster_iter_num), int(seed), int(max_iter), float(tol)
        self.stats = None

    def run(self, output_tree_path=None):
        """-> (ids, codes); writes the tree file (TreeBuilder.build: leaves flattened to the last level, no stat) when a path is given."""
        if self.embeddings is None:
            codes, self.stats, _ = self.engine.cluster_tree(item_ids=self.ids, restarts=self.restarts, max_iter=self.max_iter, tol=self.tol, seed=self.seed)
        else:
            codes, self.stats, _ = self.engine.cluster_tree(embeddings=self.embeddings, restarts=self.restarts, max_iter=self.max_iter, tol=self.tol,
                                                            seed=self.seed)
        if output_tree_path:
            tree_io.write_tree_file(output_tree_path, self.ids, codes)
        return self.ids, codes


def tdm_cluster_tree(conf_path, quiet=True, engine=None, seed=2024):
    """-> dict(ids, codes, seconds, stats, params)."""
    from .engine import Engine
    p = C.task_params("TDMClusterTree", conf_path)
    if not quiet:
        print("\n".join("%s: %s" % kv for kv in sorted(p.items())))
    ids, emb = read_embeddings(p["embed_path"])
    eng = engine or Engine(0)
    t0 = time.perf_counter()
    model = RecursiveCluster(eng, ids, emb, cluster_iter_num=p["cluster_num"], cluster_type=p["cluster_type"], seed=seed)
    ids, codes = model.run(p["tree_protobuf_path"])
    dt = time.perf_counter() - t0
    if not quiet:
        print("cluster tree: %d items, %.4fs" % (ids.size, dt))
    return dict(ids=ids, codes=codes, seconds=dt, stats=model.stats, params=p)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    path = None
    for i, a in enumerate(argv):
        if a == "--tdmConfFile" and i + 1 < len(argv):
            path = argv[i + 1]
        elif a.startswith("--tdmConfFile="):
            path = a.split("=", 1)[1]
    if path is None:
        print("usage: python -m dismember_amd.cluster --tdmConfFile <file> [--quiet]", file=sys.stderr)
        return 2
    tdm_cluster_tree(path, quiet="--quiet" in argv)
    return 0


if __name__ == "__main__":
    sys.exit(main())
