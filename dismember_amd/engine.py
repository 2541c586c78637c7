"""Thin object wrapper over the C ABI: one Engine == one dm_handle_t (device + stream)."""
import ctypes as C
import os

import numpy as np

from . import _native as N


class DismemberError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("dismember_hip error %d: %s" % (code, msg))
        self.code = code


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t):
    return a.ctypes.data_as(t)


class Engine:
    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        rc = N.lib().dm_create(device_id, C.byref(self._h))
        if rc != 0:
            raise DismemberError(rc, (N.lib().dm_last_error(None) or b"").decode())
        self.E = None
        self.dtype = None

    def clone(self):
        """dm_clone: a second engine on the same device that reads this engine's tree, weights and derived copies (no copy is made)
        through its own stream and request buffers — the reference's cloneModule() workers (LocalOptimizer.scala:28-44).  Loading and
        training go through the owner; close the clones first."""
        c = Engine.__new__(Engine)
        c._h = C.c_void_p()
        self._chk(N.lib().dm_clone(self._h, C.byref(c._h)))
        c.E, c.dtype = self.E, self.dtype
        c._owner = self                      # keeps the owner alive for as long as the clone exists
        return c

    def close(self):
        if getattr(self, "_h", None):
            rc = N.lib().dm_destroy(self._h)
            if rc != 0:
                raise DismemberError(rc, (N.lib().dm_last_error(self._h) or b"").decode())
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise DismemberError(rc, (N.lib().dm_last_error(self._h) or b"").decode())

    # ---- loading
    def load_tree(self, codes, node_ids, is_leaf, max_level):
        codes, node_ids = _i32(codes), _i32(node_ids)
        is_leaf = np.ascontiguousarray(is_leaf, dtype=np.uint8)
        self.max_level = int(max_level)
        self._chk(N.lib().dm_load_tree_tdm(self._h, _p(codes, N.i32p), _p(node_ids, N.i32p), _p(is_leaf, N.u8p),
                                           codes.size, int(max_level)))

    def load_tree_file(self, path):
        """TDM.loadTree / TDMOp.initTree(treePbPath) (tdm/.../model/TDM.scala:50-52; DistTree.loadData, tdm/.../tree/DistTree.scala:40-87):
        a reference tree file -> device index + id maps + node probabilities, parsed inside the library (dm_load_tree_file)."""
        self._chk(N.lib().dm_load_tree_file(self._h, os.fsencode(path)))
        with open(path, "rb") as f:                    # max_level for the Python-side bookkeeping: the tree_meta record closes the file
            data = f.read()
        from . import tree_io
        self.max_level = tree_io.read_max_level(data)

    def load_id_maps(self, leaf_item_ids, leaf_codes):
        a, b = _i32(leaf_item_ids), _i32(leaf_codes)
        self._chk(N.lib().dm_load_id_maps(self._h, _p(a, N.i32p), _p(b, N.i32p), a.size))

    def load_weights_din(self, compact, E, num_index):
        w = np.ascontiguousarray(compact)
        if w.dtype == np.float32:
            dt = 0
        elif w.dtype == np.float64:
            dt = 1
        else:
            raise TypeError("weights must be float32 or float64")
        self._chk(N.lib().dm_load_weights_din(self._h, dt, int(E), int(num_index), w.ctypes.data_as(C.c_void_p), w.size))
        self.E, self.dtype, self.num_index = int(E), w.dtype, int(num_index)

    def load_weights_deepfm(self, compact, E, L, num_index):
        """dm_load_weights_deepfm: the reference's DeepFM graph (tdm/.../model/DeepFM.scala:11-45), float32 only, compact vector
        [emb num_index x E ; l1.W T x (T E) ; l1.b T ; l2.W 1 x T ; l2.b 1] with T = L + 1.  L is part of the model."""
        w = np.ascontiguousarray(compact)
        if w.dtype == np.float32:
            dt = 0
        elif w.dtype == np.float64:
            dt = 1                                     # (refused by the library: DM_ERR_UNSUPPORTED)
        else:
            raise TypeError("weights must be float32")
        self._chk(N.lib().dm_load_weights_deepfm(self._h, dt, int(E), int(L), int(num_index), w.ctypes.data_as(C.c_void_p), w.size))
        self.E, self.dtype, self.num_index = int(E), w.dtype, int(num_index)

    def scorer_kind(self):
        """(kind, seq_len) of the loaded scorer (dm_get_scorer_kind): ("din", 0) or ("deepfm", L)."""
        k, sl = C.c_int(0), C.c_int(0)
        self._chk(N.lib().dm_get_scorer_kind(self._h, C.byref(k), C.byref(sl)))
        return ("deepfm" if k.value == 1 else "din"), sl.value

    @property
    def scorer(self):
        return self.scorer_kind()[0]

    def load_weights_din_synthetic(self, E, num_index, seed, small=None, tree_depth=None, rho=0.0, std=0.05):
        """Build the compact DIN vector on the device (N(0, 0.05) table; `small` = host array holding
        [att.W ; l1.W ; l1.b ; l2.W ; l2.b], defaults to the reference init) and load it without a host copy."""
        n = num_index * E + 3 * E * E + 2 * E + 1
        d = self.dev_alloc(n * 4)
        if tree_depth is not None and rho > 0.0:
            assert num_index == (1 << (tree_depth + 1)) - 1
            self._chk(N.lib().dm_fill_tree_normal(self._h, d, int(E), int(tree_depth), float(rho), float(std), int(seed)))
        else:
            self._chk(N.lib().dm_fill_normal(self._h, d, num_index * E, 0.0, float(std), int(seed)))
        if small is None:
            rng = np.random.default_rng(int(seed))
            small = np.zeros(3 * E * E + 2 * E + 1, np.float32)
            small[:3 * E * E] = rng.standard_normal(3 * E * E, dtype=np.float32) * 0.05
            small[3 * E * E + E:3 * E * E + 2 * E] = rng.standard_normal(E, dtype=np.float32) * 0.05
        small = np.ascontiguousarray(small, dtype=np.float32)
        assert small.size == 3 * E * E + 2 * E + 1
        self._chk(N.lib().dm_memcpy_h2d(self._h, C.c_void_p(d.value + num_index * E * 4),
                                        small.ctypes.data_as(C.c_void_p), small.nbytes))
        self._chk(N.lib().dm_load_weights_din_dev(self._h, int(E), int(num_index), d, n))
        self.E, self.dtype, self.num_index = int(E), np.dtype(np.float32), int(num_index)
        self._synth_ptr, self._synth_n = d, n
        return d

    def load_weights_din_synthetic_f64(self, E, num_index, seed, small=None):
        """The fp64 counterpart (the reference's OTM model type): the table holds the f32 draws widened to double
        (dm_fill_normal_f64), the small matrices come from `small` (defaults to the reference init) as doubles."""
        n = num_index * E + 3 * E * E + 2 * E + 1
        d = self.dev_alloc(n * 8)
        self._chk(N.lib().dm_fill_normal_f64(self._h, d, num_index * E, 0.0, 0.05, int(seed)))
        if small is None:
            rng = np.random.default_rng(int(seed))
            small = np.zeros(3 * E * E + 2 * E + 1, np.float32)
            small[:3 * E * E] = rng.standard_normal(3 * E * E, dtype=np.float32) * 0.05
            small[3 * E * E + E:3 * E * E + 2 * E] = rng.standard_normal(E, dtype=np.float32) * 0.05
        small = np.ascontiguousarray(small, dtype=np.float64)
        assert small.size == 3 * E * E + 2 * E + 1
        self._chk(N.lib().dm_memcpy_h2d(self._h, C.c_void_p(d.value + num_index * E * 8),
                                        small.ctypes.data_as(C.c_void_p), small.nbytes))
        self._chk(N.lib().dm_load_weights_din_dev_f64(self._h, int(E), int(num_index), d, n))
        self.E, self.dtype, self.num_index = int(E), np.dtype(np.float64), int(num_index)
        self._synth_ptr, self._synth_n = d, n
        return d

    def save_model(self, path):
        """TDM.saveModel (T/model/TDM.scala:32-41): weights + index in one flat file (dm_save_model)."""
        self._chk(N.lib().dm_save_model(self._h, os.fsencode(path)))

    @staticmethod
    def checkpoint_leaf_ids(path):
        """(item ids, leaf codes) of a dm_save_model checkpoint (layout: csrc/checkpoint.hip.inc); empty when it holds no id map."""
        import struct
        with open(path, "rb") as f:
            hd = f.read(72)
            _, _, _, _, has_tree, has_ids, _, _ = struct.unpack("<8i", hd[8:40])
            _, _, n_nodes, n_leaf = struct.unpack("<4q", hd[40:72])
            if not has_ids:
                return np.zeros(0, np.int32), np.zeros(0, np.int32)
            if has_tree:
                f.seek(72 + 8 * n_nodes + (n_nodes + 7) // 8 * 8)
            both = np.frombuffer(f.read(8 * n_leaf), dtype="<i4")
        return both[:n_leaf].astype(np.int32), both[n_leaf:].astype(np.int32)

    # ---- TDMClusterTree (csrc/cluster.hip.inc)
    def leaf_embeddings(self, item_ids):
        """dm_get_leaf_embeddings: the loaded table's rows at the items' current leaf codes, [n, E] float32."""
        ids = _i32(item_ids).ravel()
        if self.E is None:
            raise DismemberError(-3, "leaf_embeddings: no weights loaded through this Engine")
        out = np.empty((ids.size, int(self.E)), np.float32)
        self._chk(N.lib().dm_get_leaf_embeddings(self._h, _p(ids, N.i32p), ids.size, _p(out, N.f32p)))
        return out

    def cluster_tree(self, embeddings=None, item_ids=None, restarts=10, max_iter=100, tol=1e-4, seed=0, trace=False):
        """dm_cluster_tree (embeddings: [n, E] float32 on the host) or dm_cluster_tree_model (item_ids: the rows of the loaded
        table at the items' leaf codes, gathered on the device) -> (codes [n] before flattenLeaves, stats dict, trace dict | None).
        max_level = ceil(log2 n); the trace arrays are indexed as include/dismember_hip.h says."""
        if (embeddings is None) == (item_ids is None):
            raise ValueError("cluster_tree: give either embeddings or item_ids")
        if embeddings is not None:
            x = np.ascontiguousarray(embeddings, dtype=np.float32)
            if x.ndim != 2:
                raise ValueError("cluster_tree: embeddings must be [n, E]")
            n, E = x.shape
        else:
            ids = _i32(item_ids).ravel()
            n, E = ids.size, int(self.E or 0)
        codes = np.empty(max(n, 1), np.int32)
        stats = N.ClusterStats()
        tr, bufs = None, None
        if trace:
            max_level = max(0, int(n - 1).bit_length()) if n > 1 else 0
            nodes = (1 << max_level) - 1
            bufs = dict(centroid0=np.full((max(nodes, 1), max(E, 1)), np.nan, np.float32), seeds=np.full((max(nodes, 1), 2), -1, np.int32),
                        iters=np.zeros(max(nodes, 1), np.int32), distortion=np.full(max(nodes, 1), np.nan, np.float64),
                        dist=np.full((max(max_level, 1), max(n, 1)), np.nan, np.float32), perm=np.zeros(max(n, 1), np.int32))
            tr = N.ClusterTrace(nodes, max_level, _p(bufs["centroid0"], N.f32p), _p(bufs["seeds"], N.i32p), _p(bufs["iters"], N.i32p),
                                bufs["distortion"].ctypes.data_as(C.POINTER(C.c_double)), _p(bufs["dist"], N.f32p), _p(bufs["perm"], N.i32p))
        trp = C.byref(tr) if tr is not None else None
        if embeddings is not None:
            rc = N.lib().dm_cluster_tree(self._h, _p(x, N.f32p), n, E, int(restarts), int(max_iter), float(tol), int(seed) & (2 ** 64 - 1),
                                         _p(codes, N.i32p), trp, C.byref(stats))
        else:
            rc = N.lib().dm_cluster_tree_model(self._h, _p(ids, N.i32p), n, int(restarts), int(max_iter), float(tol), int(seed) & (2 ** 64 - 1),
                                               _p(codes, N.i32p), trp, C.byref(stats))
        self._chk(rc)
        st = {k: getattr(stats, k) for k, _ in N.ClusterStats._fields_}
        if bufs is not None:
            bufs.update(max_level=max_level, centroid0=bufs["centroid0"][:nodes], seeds=bufs["seeds"][:nodes], iters=bufs["iters"][:nodes],
                        distortion=bufs["distortion"][:nodes], dist=bufs["dist"][:max_level], perm=bufs["perm"][:n])
        return codes[:n], st, bufs

    def load_model(self, path):
        """TDM.loadModel: replaces the handle's tree, id maps and weights with the checkpoint's."""
        self._chk(N.lib().dm_load_model(self._h, os.fsencode(path)))
        import struct
        with open(path, "rb") as f:
            hd = f.read(8 + 8 * 4 + 4 * 8)
        _, dtype, E, max_level, has_tree, _, _, _ = struct.unpack("<8i", hd[8:40])
        num_index, = struct.unpack("<q", hd[40:48])
        self.E, self.dtype, self.num_index = int(E), np.dtype(np.float64 if dtype == 1 else np.float32), int(num_index)
        if has_tree:
            self.max_level = int(max_level)

    def download_weights(self):
        """Host copy of the compact vector built by load_weights_din_synthetic (for the CPU oracle)."""
        out = np.empty(self._synth_n, self.dtype)
        self.d2h(out, self._synth_ptr)
        return out

    # ---- operator level
    def id_to_code(self, item_ids):
        ids = _i32(item_ids)
        codes = np.empty_like(ids)
        mask = np.empty_like(ids)
        nm = C.c_int(0)
        self._chk(N.lib().dm_tdm_id_to_code(self._h, _p(ids, N.i32p), ids.size, _p(codes, N.i32p), _p(mask, N.i32p),
                                            C.byref(nm)))
        return codes, mask[:nm.value].copy()

    def din_forward(self, codes, seqs, pad_flat_idx=None, L=None):
        codes = _i32(codes).ravel()
        seqs = _i32(seqs)
        B = codes.size
        if L is None:
            L = seqs.shape[-1] if seqs.ndim == 2 else seqs.size // max(B, 1)
        seqs = seqs.ravel()
        pad = _i32([] if pad_flat_idx is None else pad_flat_idx).ravel()
        out = np.empty(B, dtype=self.dtype)
        self._chk(N.lib().dm_din_forward(self._h, _p(codes, N.i32p), _p(seqs, N.i32p), _p(pad, N.i32p), pad.size, B, L,
                                         out.ctypes.data_as(C.c_void_p)))
        return out

    def deepfm_forward(self, codes, seqs):
        """dm_deepfm_forward: logits [B] float32 of the DeepFM graph for rows (code, history codes [L]); -1 = a zero row.  There is no
        mask argument: the graph has none."""
        codes = _i32(codes).ravel()
        seqs = _i32(seqs)
        B = codes.size
        L = seqs.shape[-1] if seqs.ndim == 2 else seqs.size // max(B, 1)
        seqs = seqs.ravel()
        out = np.empty(B, dtype=np.float32)
        self._chk(N.lib().dm_deepfm_forward(self._h, _p(codes, N.i32p), _p(seqs, N.i32p), B, int(L), _p(out, N.f32p)))
        return out

    def deepfm_pairs_forward(self, codes, seqs, seq_div=1):
        """dm_deepfm_pairs_forward: logits [P] float32 of P (node code, history) pairs; pair i is scored against history i // seq_div
        of seqs [ceil(P / seq_div), L] (codes, -1 = a zero row).  The scorer of JTM tree learning with a DeepFM model."""
        codes = _i32(codes).ravel()
        seqs = _i32(seqs)
        P, seq_div = codes.size, int(seq_div)
        H = -(-P // max(seq_div, 1))
        L = seqs.shape[-1] if seqs.ndim == 2 else seqs.size // max(H, 1)
        if seq_div >= 1 and seqs.size != H * L:
            raise ValueError("deepfm_pairs_forward: %d pairs at seq_div %d need %d histories, got %d values of L = %d" % (P, seq_div, H, seqs.size, L))
        seqs = seqs.ravel()
        out = np.empty(P, dtype=np.float32)
        self._chk(N.lib().dm_deepfm_pairs_forward(self._h, _p(codes, N.i32p), _p(seqs, N.i32p), P, int(L), seq_div, _p(out, N.f32p)))
        return out

    # ---- OTM tree construction with a DeepFM model (csrc/dfm_otm_tree.hip.inc)
    @staticmethod
    def _otm_tree_rows(row_off, row_codes):
        off = np.ascontiguousarray(row_off, np.int64).ravel()
        rows = _i32(row_codes)
        n = off.size - 1
        R = int(off[-1]) if off.size else 0
        if n < 0:
            raise ValueError("row_off needs n_items + 1 entries")
        L = rows.shape[-1] if rows.ndim == 2 else rows.size // max(R, 1)
        rows = rows.ravel()
        if rows.size < R * L:
            raise ValueError("row_off ends at row %d but row_codes holds %d values of L = %d" % (R, rows.size, L))
        return off, rows, n, int(L)

    def deepfm_otm_child_weights(self, row_off, row_codes, item_node, old_level, level, L=None, use_mask=False):
        """dm_deepfm_otm_child_weights: weights [n_items, 2^(level - old_level)] float64 of TreeConstruction.aggregateWeights with the
        DeepFM graph; item i owns the histories row_off[i] .. row_off[i + 1] of row_codes [rows, L] (NODE codes, -1 = padding) and sits
        in node item_node[i] of old_level."""
        off, rows, n, Lr = self._otm_tree_rows(row_off, row_codes)
        node = _i32(item_node).ravel()
        if node.size != n:
            raise ValueError("item_node holds %d entries for %d items" % (node.size, n))
        w = np.empty((max(n, 1), 1 << max(0, min(int(level) - int(old_level), 8))), np.float64)
        self._chk(N.lib().dm_deepfm_otm_child_weights(self._h, _p(off, N.i64p), _p(rows, N.i32p), _p(node, N.i32p), n, int(Lr if L is None else L),
                                                      int(old_level), int(level), int(use_mask), w.ctypes.data_as(C.POINTER(C.c_double))))
        return w[:n]

    def deepfm_otm_tree_prepare(self, row_off, row_codes, L=None):
        """dm_deepfm_otm_tree_prepare: the histories of a catalogue go up once and their per-history part of the score stays on the
        device for deepfm_otm_tree_weights; a second prepare replaces the first."""
        off, rows, n, Lr = self._otm_tree_rows(row_off, row_codes)
        self._chk(N.lib().dm_deepfm_otm_tree_prepare(self._h, _p(off, N.i64p), _p(rows, N.i32p), n, int(Lr if L is None else L)))

    def deepfm_otm_tree_weights(self, item_node, old_level, level):
        """dm_deepfm_otm_tree_weights: one gap step on the prepared catalogue; the bytes of deepfm_otm_child_weights."""
        node = _i32(item_node).ravel()
        n = node.size
        w = np.empty((max(n, 1), 1 << max(0, min(int(level) - int(old_level), 8))), np.float64)
        self._chk(N.lib().dm_deepfm_otm_tree_weights(self._h, _p(node, N.i32p), n, int(old_level), int(level), w.ctypes.data_as(C.POINTER(C.c_double))))
        return w[:n]

    def deepfm_otm_tree_release(self):
        self._chk(N.lib().dm_deepfm_otm_tree_release(self._h))

    # ---- beam search
    @staticmethod
    def _csr(consumed, U):
        if consumed is None:
            return None, None
        off = np.zeros(U + 1, np.int64)
        for u in range(U):
            off[u + 1] = off[u] + len(consumed[u])
        ids = _i32(np.concatenate([_i32(c) for c in consumed]) if off[U] > 0 else np.zeros(1, np.int32))
        return off, ids

    def tdm_beam_search(self, seq_item_ids, beam, topk, use_mask=True, consumed=None, widen_consumed=False, out=None):
        """out: optional (ids [U, topk] int32, scores [U, topk] float32, counts [U] int32) to fill — a serving loop reuses its result
        buffers (fresh 200 MB arrays page-fault on every call, inside the download)."""
        seq = _i32(seq_item_ids)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, L = seq.shape
        opts = N.SearchOpts(int(beam), int(topk), int(bool(use_mask)), int(bool(widen_consumed)))
        off, cids = self._csr(consumed, U)
        if out is not None:
            ids, sc, cnt = out
            assert ids.shape == (U, topk) and ids.dtype == np.int32 and sc.shape == (U, topk) and sc.dtype == np.float32
            assert cnt.shape == (U,) and cnt.dtype == np.int32 and ids.flags.c_contiguous and sc.flags.c_contiguous
        else:
            ids = np.empty((U, topk), np.int32)
            sc = np.empty((U, topk), np.float32)
            cnt = np.empty(U, np.int32)
        self._chk(N.lib().dm_tdm_beam_search(self._h, _p(seq, N.i32p), U, L, C.byref(opts),
                                             None if off is None else _p(off, N.i64p),
                                             None if cids is None else _p(cids, N.i32p), _p(ids, N.i32p),
                                             _p(sc, N.f32p), _p(cnt, N.i32p)))
        return ids, sc, cnt

    def tdm_beam_search_trace(self, seq_item_ids, beam, topk, use_mask=True, max_levels=None):
        seq = _i32(seq_item_ids)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, L = seq.shape
        if max_levels is None:
            max_levels = self.max_level + 2
        cap = max(32, ((2 * beam + 15) // 16) * 16)
        opts = N.SearchOpts(int(beam), int(topk), int(bool(use_mask)), 0)
        ids = np.empty((U, topk), np.int32)
        sc = np.empty((U, topk), np.float32)
        cnt = np.empty(U, np.int32)
        tc = np.zeros((U, max_levels, cap), np.int32)
        ts = np.zeros((U, max_levels, cap), np.float32)
        tn = np.zeros((U, max_levels), np.int32)
        self._chk(N.lib().dm_tdm_beam_search_trace(self._h, _p(seq, N.i32p), U, L, C.byref(opts), _p(ids, N.i32p),
                                                   _p(sc, N.f32p), _p(cnt, N.i32p), max_levels, _p(tc, N.i32p),
                                                   _p(ts, N.f32p), _p(tn, N.i32p)))
        return ids, sc, cnt, tc, ts, tn

    def otm_beam_search(self, seq_codes, beam, leaf_level, out=None):
        seq = _i32(seq_codes)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, L = seq.shape
        if out is not None:
            ids, sc, cnt = out
            assert ids.shape == (U, 2 * beam) and ids.dtype == np.int32 and sc.shape == (U, 2 * beam) and sc.dtype == np.float32
            assert cnt.shape == (U,) and cnt.dtype == np.int32 and ids.flags.c_contiguous and sc.flags.c_contiguous
        else:
            ids = np.empty((U, 2 * beam), np.int32)
            sc = np.empty((U, 2 * beam), np.float32)
            cnt = np.empty(U, np.int32)
        fn = N.lib().dm_deepfm_otm_beam_search if self.scorer == "deepfm" else N.lib().dm_otm_beam_search      # (the DeepFM twin: DESIGN.md §15)
        self._chk(fn(self._h, _p(seq, N.i32p), U, L, int(beam), int(leaf_level), _p(ids, N.i32p), _p(sc, N.f32p), _p(cnt, N.i32p)))
        return ids, sc, cnt

    def otm_beam_search_f64(self, seq_codes, beam, leaf_level, trace_levels=None):
        """CandidateSearcher.beamSearch in the reference's own arithmetic (DIN[Double]); f64 weights required.  With
        trace_levels: also every level's candidates (OTMTree.beamSearchNodes): (ids, scores, counts, tc, ts, tn)."""
        seq = _i32(seq_codes)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, L = seq.shape
        f64p = C.POINTER(C.c_double)
        ids = np.empty((U, 2 * beam), np.int32)
        sc = np.empty((U, 2 * beam), np.float64)
        cnt = np.empty(U, np.int32)
        if trace_levels is None:
            self._chk(N.lib().dm_otm_beam_search_f64(self._h, _p(seq, N.i32p), U, L, int(beam), int(leaf_level), _p(ids, N.i32p),
                                                     sc.ctypes.data_as(f64p), _p(cnt, N.i32p)))
            return ids, sc, cnt
        cap = max(32, ((2 * beam + 15) // 16) * 16)
        tc = np.zeros((U, trace_levels, cap), np.int32)
        ts = np.zeros((U, trace_levels, cap), np.float64)
        tn = np.zeros((U, trace_levels), np.int32)
        self._chk(N.lib().dm_otm_beam_search_trace_f64(self._h, _p(seq, N.i32p), U, L, int(beam), int(leaf_level), _p(ids, N.i32p),
                                                       sc.ctypes.data_as(f64p), _p(cnt, N.i32p), int(trace_levels),
                                                       _p(tc, N.i32p), ts.ctypes.data_as(f64p), _p(tn, N.i32p)))
        return ids, sc, cnt, tc, ts, tn

    def otm_beam_search_trace(self, seq_codes, beam, leaf_level, trace_levels):
        """dm_otm_beam_search_trace (float scores; arithmetic per the scorer mode; a DeepFM model: dm_deepfm_otm_beam_search_trace):
        (ids, scores, counts, tc, ts, tn)."""
        seq = _i32(seq_codes)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, L = seq.shape
        cap = max(32, ((2 * beam + 15) // 16) * 16)
        ids = np.empty((U, 2 * beam), np.int32); sc = np.empty((U, 2 * beam), np.float32); cnt = np.empty(U, np.int32)
        tc = np.zeros((U, trace_levels, cap), np.int32); ts = np.zeros((U, trace_levels, cap), np.float32)
        tn = np.zeros((U, trace_levels), np.int32)
        fn = N.lib().dm_deepfm_otm_beam_search_trace if self.scorer == "deepfm" else N.lib().dm_otm_beam_search_trace
        self._chk(fn(self._h, _p(seq, N.i32p), U, L, int(beam), int(leaf_level), _p(ids, N.i32p), _p(sc, N.f32p), _p(cnt, N.i32p),
                     int(trace_levels), _p(tc, N.i32p), _p(ts, N.f32p), _p(tn, N.i32p)))
        return ids, sc, cnt, tc, ts, tn

    def tdm_bruteforce_topk(self, seq_item_ids, topk, use_mask=True):
        seq = _i32(seq_item_ids)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, L = seq.shape
        ids = np.empty((U, topk), np.int32)
        sc = np.empty((U, topk), np.float32)
        cnt = np.empty(U, np.int32)
        self._chk(N.lib().dm_tdm_bruteforce_topk(self._h, _p(seq, N.i32p), U, L, int(topk), int(bool(use_mask)),
                                                 _p(ids, N.i32p), _p(sc, N.f32p), _p(cnt, N.i32p)))
        return ids, sc, cnt

    # ---- training (row A12)
    def train_init(self, lr=1e-3, lr_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
        o = N.AdamOpts(lr, lr_decay, beta1, beta2, eps)
        self._chk(N.lib().dm_train_init(self._h, C.byref(o)))

    def train_forward_backward(self, codes, seqs, pad_flat_idx, labels):
        codes = _i32(codes).ravel()
        seqs = _i32(seqs)
        B = codes.size
        L = seqs.shape[-1] if seqs.ndim == 2 else seqs.size // B
        seqs = seqs.ravel()
        pad = _i32([] if pad_flat_idx is None else pad_flat_idx).ravel()
        lab = np.ascontiguousarray(labels, np.float32).ravel()
        loss = C.c_float(0)
        self._chk(N.lib().dm_train_forward_backward(self._h, _p(codes, N.i32p), _p(seqs, N.i32p), _p(pad, N.i32p), pad.size,
                                                    _p(lab, N.f32p), B, L, C.byref(loss)))
        return self.train_last_loss() if self.dtype == np.float64 else loss.value

    def train_last_loss(self):
        """The loss of the last forward/backward in the model's precision (dm_train_last_loss)."""
        v = C.c_double(0)
        self._chk(N.lib().dm_train_last_loss(self._h, C.byref(v)))
        return v.value

    def train_sync_stats(self):
        o = (C.c_uint64 * 8)()
        self._chk(N.lib().dm_train_sync_stats(self._h, o))
        return {"nranks": int(o[0]), "transport": "rccl" if o[1] == 1 else "host", "rows_mine": int(o[2]), "rows_total": int(o[3]),
                "bytes_sent": int(o[4]), "bytes_recv": int(o[5]), "host_syncs": int(o[6])}

    def set_node_probs(self, codes, probs):
        """Node.probality per tree node (needed by sample_with_probability)."""
        c = _i32(codes); pr = np.ascontiguousarray(probs, np.float32)
        self._chk(N.lib().dm_tdm_set_node_probs(self._h, _p(c, N.i32p), _p(pr, N.f32p), c.size))

    def make_train_batch(self, seq_item_ids, target_item_ids, neg_counts, start_level=1, seed=0, use_mask=True, with_prob=False,
                         tolerance=20):
        """NegativeSampler.sample + MiniBatch.convert (sampled on the device): (codes [R], seqs [R, L], rowmask [R], labels [R])."""
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), int(bool(use_mask)), int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_tdm_make_train_batch(self._h, _p(seq, N.i32p), _p(tgt, N.i32p), T, L, _p(neg, N.i32p), neg.size,
                                                  C.byref(o), None, None, None, None, 0, C.byref(n)))
        R = n.value
        codes = np.empty(max(R, 1), np.int32); seqs = np.empty((max(R, 1), L), np.int32)
        mask = np.empty(max(R, 1), np.uint32); lab = np.empty(max(R, 1), np.float32)
        self._chk(N.lib().dm_tdm_make_train_batch(self._h, _p(seq, N.i32p), _p(tgt, N.i32p), T, L, _p(neg, N.i32p), neg.size,
                                                  C.byref(o), _p(codes, N.i32p), _p(seqs, N.i32p),
                                                  mask.ctypes.data_as(C.POINTER(C.c_uint32)), _p(lab, N.f32p), R, C.byref(n)))
        R = n.value
        return codes[:R], seqs[:R], mask[:R], lab[:R]

    def train_step_sampled(self, seq_item_ids, target_item_ids, neg_counts, start_level=1, seed=0, use_mask=True, with_prob=False,
                           tolerance=20, grouped=False):
        """convertBatch + trainBatch with the rows resident in HBM: targets and histories are uploaded (40 B per target),
        dm_tdm_sample_train_batch_dev expands them on the device straight into the buffers of
        dm_train_forward_backward_dev.  Returns the mean BCE loss of the expanded rows.
        grouped (f32 models, L <= 16): dm_tdm_sample_train_batch_csr_dev into the buffers of dm_train_forward_backward_csr_dev instead
         — the same rows from the same seed, every target's history and mask written and read once; no [R][L] row
        histories are carved."""
        if grouped:
            return self._train_step_sampled_csr(seq_item_ids, target_item_ids, neg_counts, start_level, seed, use_mask, with_prob, tolerance)
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), int(bool(use_mask)), int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_tdm_sample_train_batch_dev(self._h, None, None, T, L, _p(neg, N.i32p), neg.size, C.byref(o), None, None,
                                                        None, None, 0, C.byref(n)))
        R = max(n.value, 1)
        al = lambda v: (v + 255) & ~255
        need = al(T * L * 4) + al(T * 4) + 2 * al(R * 4) + al(R * L * 4) + al(R * 4)     # the six sub-buffers as carved below
        if getattr(self, "_samp_bytes", 0) < need:
            if getattr(self, "_samp_buf", None):
                self.dev_free(self._samp_buf)
            self._samp_buf, self._samp_bytes = self.dev_alloc(need + need // 2), need + need // 2
        base = self._samp_buf.value
        d_seq = C.c_void_p(base); base += al(T * L * 4)
        d_tgt = C.c_void_p(base); base += al(T * 4)
        d_codes = C.c_void_p(base); base += al(R * 4)
        d_seqs = C.c_void_p(base); base += al(R * L * 4)
        d_mask = C.c_void_p(base); base += al(R * 4)
        d_lab = C.c_void_p(base)
        self.h2d(d_seq, seq); self.h2d(d_tgt, tgt)
        self._chk(N.lib().dm_tdm_sample_train_batch_dev(self._h, d_seq, d_tgt, T, L, _p(neg, N.i32p), neg.size, C.byref(o), d_codes,
                                                        d_seqs, d_mask, d_lab, R, C.byref(n)))
        if n.value == 0:
            return 0.0
        loss = C.c_float(0)
        self._chk(N.lib().dm_train_forward_backward_dev(self._h, d_codes, d_seqs, d_mask, d_lab, n.value, L, C.byref(loss)))
        return loss.value

    def _sample_csr_carve(self, T, L, R):
        """the sampler's CSR buffers inside the engine's grow-only sampling buffer: ids, targets, codes, seq codes, masks, offsets, labels"""
        al = lambda v: (v + 255) & ~255
        need = 2 * al(T * L * 4) + 2 * al(T * 4) + 2 * al(R * 4) + al((T + 1) * 8)        # the seven sub-buffers as carved below: no [R][L]
        if getattr(self, "_samp_bytes", 0) < need:
            if getattr(self, "_samp_buf", None):
                self.dev_free(self._samp_buf)
            self._samp_buf, self._samp_bytes = self.dev_alloc(need + need // 2), need + need // 2
        base = self._samp_buf.value
        out = []
        for nbytes in (T * L * 4, T * 4, R * 4, T * L * 4, T * 4, (T + 1) * 8, R * 4):
            out.append(C.c_void_p(base)); base += al(nbytes)
        return out

    def _sample_csr_dev(self, seq_item_ids, target_item_ids, neg_counts, start_level, seed, use_mask, with_prob, tolerance):
        """dm_tdm_sample_train_batch_csr_dev into the sampling buffer -> (T, L, R, d_codes, d_sc, d_um, d_off, d_lab)"""
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), int(bool(use_mask)), int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_tdm_sample_train_batch_csr_dev(self._h, None, None, T, L, _p(neg, N.i32p), neg.size, C.byref(o), None, None, None,
                                                            None, None, 0, C.byref(n)))
        R = max(n.value, 1)
        d_seq, d_tgt, d_codes, d_sc, d_um, d_off, d_lab = self._sample_csr_carve(T, L, R)
        if T:
            self.h2d(d_seq, seq); self.h2d(d_tgt, tgt)
        self._chk(N.lib().dm_tdm_sample_train_batch_csr_dev(self._h, d_seq, d_tgt, T, L, _p(neg, N.i32p), neg.size, C.byref(o), d_codes, d_sc,
                                                            d_um, d_off, d_lab, R, C.byref(n)))
        return T, L, n.value, d_codes, d_sc, d_um, d_off, d_lab

    def _train_step_sampled_csr(self, seq_item_ids, target_item_ids, neg_counts, start_level, seed, use_mask, with_prob, tolerance):
        T, L, R, d_codes, d_sc, d_um, d_off, d_lab = self._sample_csr_dev(seq_item_ids, target_item_ids, neg_counts, start_level, seed,
                                                                           use_mask, with_prob, tolerance)
        if R == 0:
            return 0.0
        return self.train_forward_backward_csr_dev(d_sc, d_um, d_off, d_codes, d_lab, T, R, L)

    def sample_train_batch_csr(self, seq_item_ids, target_item_ids, neg_counts, start_level=1, seed=0, use_mask=True, with_prob=False,
                               tolerance=20):
        """dm_tdm_sample_train_batch_csr_dev, downloaded (for the tests): (codes [R], labels [R], seq_codes [T, L], user_mask [T],
        row_off [T + 1])."""
        T, L, R, d_codes, d_sc, d_um, d_off, d_lab = self._sample_csr_dev(seq_item_ids, target_item_ids, neg_counts, start_level, seed,
                                                                           use_mask, with_prob, tolerance)
        codes = np.empty(R, np.int32); lab = np.empty(R, np.float32); sc = np.empty((T, L), np.int32)
        um = np.empty(T, np.uint32); off = np.empty(T + 1, np.int64)
        if R:
            self.d2h(codes, d_codes); self.d2h(lab, d_lab)
        self.d2h(off, d_off)
        if T:
            self.d2h(sc, d_sc); self.d2h(um, d_um)
        return codes, lab, sc, um, off

    def train_forward_backward_csr(self, seq_codes, user_mask, row_off, codes, labels):
        """One forward/backward of an f32 DIN model over a ragged user-grouped batch (dm_train_forward_backward_csr_dev):
        seq_codes [U][L], user_mask [U] (bit j: position j masked) or None, row_off [U + 1] (int64), codes / labels [B] — rows
        row_off[u] .. row_off[u + 1] are user u's and share its history and mask; a user may have none.  ADDS to the gradient, like
        train_forward_backward.  Checks the offsets here (ValueError), uploads and calls the device entry, which checks them again on
        the device (ids are not range-checked: one outside [0, num_index) reads as -1); -> the mean loss."""
        seq = _i32(seq_codes)
        U, L = seq.shape if seq.ndim == 2 else (0, 1)
        off = np.ascontiguousarray(row_off, np.int64).ravel()
        codes = _i32(codes).ravel()
        B = codes.size
        lab = np.ascontiguousarray(labels, np.float32).ravel()
        um = None if user_mask is None else np.ascontiguousarray(user_mask, np.uint32).ravel()
        if off.size != U + 1 or lab.size != B or (um is not None and um.size != U):
            raise ValueError("train_forward_backward_csr: row_off must hold U + 1 offsets, user_mask U words and labels one value per row")
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != B:
            bad = 0 if off[0] != 0 else int(np.flatnonzero(np.diff(off) < 0)[0]) if (np.diff(off) < 0).any() else U
            raise ValueError("train_forward_backward_csr: row_off must start at 0, never decrease and end at B = %d "
                             "(first offending user %d)" % (B, bad))
        al = lambda v: (v + 255) & ~255
        buf = self.dev_alloc(al(U * L * 4) + al(U * 4) + al((U + 1) * 8) + 2 * al(B * 4) + 256)
        try:
            d_seq = C.c_void_p(buf.value)
            d_um = C.c_void_p(d_seq.value + al(U * L * 4))
            d_off = C.c_void_p(d_um.value + al(U * 4))
            d_codes = C.c_void_p(d_off.value + al((U + 1) * 8))
            d_lab = C.c_void_p(d_codes.value + al(B * 4))
            if U:
                self.h2d(d_seq, seq); self.h2d(d_off, off)
                if um is not None:
                    self.h2d(d_um, um)
            if B:
                self.h2d(d_codes, codes); self.h2d(d_lab, lab)
            return self.train_forward_backward_csr_dev(d_seq, d_um if um is not None else None, d_off, d_codes, d_lab, U, B, L)
        finally:
            self.dev_free(buf)

    def train_forward_backward_csr_dev(self, d_seq_codes, d_user_mask, d_row_off, d_codes, d_labels, U, B, L):
        """the same on device arrays: d_seq_codes [U][L], d_user_mask [U] or None, d_row_off [U + 1] int64, d_codes / d_labels [B] -> the mean loss"""
        loss = C.c_float(0)
        self._chk(N.lib().dm_train_forward_backward_csr_dev(self._h, d_seq_codes, d_user_mask, d_row_off, d_codes, d_labels, int(U), int(B), int(L),
                                                            C.byref(loss)))
        return loss.value

    def train_forward_backward_grouped(self, seq_codes, user_mask, codes, labels):
        """One forward/backward over a user-grouped batch (dm_train_forward_backward_grouped_dev): seq_codes [U][L], user_mask [U]
        (bit j: position j masked) or None, codes / labels [U][n] — every user's n candidate rows share the user's history, as
        MiniBatch.batchTransform / transformWithMask build them.  Returns the mean BCE loss (model precision)."""
        seq = _i32(seq_codes)
        U, L = seq.shape
        codes = _i32(codes).reshape(U, -1)
        n = codes.shape[1]
        lab = np.ascontiguousarray(labels, np.float32).reshape(U, n)
        al = lambda v: (v + 255) & ~255
        need = al(U * L * 4) + al(U * 4) + 2 * al(U * n * 4)
        buf = self.dev_alloc(need)
        try:
            base = buf.value
            d_seq = C.c_void_p(base); base += al(U * L * 4)
            d_um = C.c_void_p(base); base += al(U * 4)
            d_codes = C.c_void_p(base); base += al(U * n * 4)
            d_lab = C.c_void_p(base)
            self.h2d(d_seq, seq); self.h2d(d_codes, codes); self.h2d(d_lab, lab)
            if user_mask is not None:
                self.h2d(d_um, np.ascontiguousarray(user_mask, np.uint32).ravel())
            loss = C.c_float(0)
            self._chk(N.lib().dm_train_forward_backward_grouped_dev(self._h, d_seq, d_um if user_mask is not None else None, d_codes, d_lab,
                                                                    U, n, L, C.byref(loss)))
            self.synchronize()
        finally:
            self.dev_free(buf)
        return self.train_last_loss() if self.dtype == np.float64 else loss.value

    @staticmethod
    def rowmask_to_flat(mask, L):
        """Row bit masks -> the flat index list Module.forward takes (Mask.scala:27-32)."""
        i, j = np.nonzero((mask[:, None] >> np.arange(L, dtype=np.uint32)[None, :]) & 1)
        return (i * L + j).astype(np.int32)

    # ---- multi-GPU exchange (comm.py)
    def attach_comm(self, comm):
        """comm: dismember_amd.comm.Comm, a raw dm_comm_t (comm.make_clique) or None."""
        self._comm = comm
        self._chk(N.lib().dm_comm_attach(self._h, None if comm is None else getattr(comm, "_c", comm)))

    def train_sync_gradients(self):
        """LocalOptimizer.syncGradients over the attached communicator (collective: every rank calls it)."""
        self._chk(N.lib().dm_train_sync_gradients(self._h))

    def comm_all_gather_dev(self, arr):
        """Var-size all-gather of DEVICE buffers over the attached communicator (dm_comm_all_gather_dev): uploads `arr`,
        gathers on the handle's stream (RCCL broadcasts, or host staging on the host transport), returns the concatenation."""
        a = np.ascontiguousarray(arr)
        if hasattr(self._comm, "world"):
            world = self._comm.world
        else:                                          # a raw dm_comm_t (comm.make_clique): ask the library
            r_, w_, t_ = C.c_int(0), C.c_int(1), C.c_int(0)
            self._chk(N.lib().dm_comm_rank(self._comm, C.byref(r_), C.byref(w_), C.byref(t_)))
            world = w_.value
        sizes = (C.c_uint64 * world)()
        d_send = self.dev_alloc(max(a.nbytes, 16))
        self.h2d(d_send, a)
        self._chk(N.lib().dm_comm_all_gather_dev(self._h, d_send, a.nbytes, None, 0, sizes))
        total = int(sum(sizes))
        d_recv = self.dev_alloc(max(total, 16))
        self._chk(N.lib().dm_comm_all_gather_dev(self._h, d_send, a.nbytes, d_recv, total, sizes))
        out = np.empty(total // a.itemsize, a.dtype)
        self.d2h(out, d_recv)
        self.dev_free(d_send); self.dev_free(d_recv)
        return out.reshape((-1,) + a.shape[1:])

    def adam_step(self, grad_scale=1.0):
        self._chk(N.lib().dm_adam_step(self._h, float(grad_scale)))

    def adam_last_step_rows(self):
        """(rows visited by the last Adam step, True when it took the active-rows path)."""
        r, a = C.c_uint64(0), C.c_int(0)
        self._chk(N.lib().dm_adam_last_step_rows(self._h, C.byref(r), C.byref(a)))
        return int(r.value), bool(a.value)

    def train_download(self, what="weights"):
        n = self.num_index * self.E + 3 * self.E * self.E + 2 * self.E + 1
        out = np.empty(n, self.dtype)          # the loaded dtype: fp64 models train in fp64
        self._chk(N.lib().dm_train_download(self._h, {"weights": 0, "grad": 1, "s": 2, "r": 3}[what], out.ctypes.data_as(C.c_void_p), n))
        return out

    # ---- Deep-Retrieval (row A13)
    def dr_load_model(self, weights, E, L, K, D, num_item, dtype=np.float64):
        """weights: dict with layer_emb, layer_w [D], layer_b [D] and optionally rerank_emb, rerank_w, rerank_b,
        softmax_w, softmax_b (numpy arrays; converted to `dtype`, which is also the arithmetic type)."""
        dt = np.dtype(dtype)
        f = lambda a: np.ascontiguousarray(a, dtype=dt)
        keep = dict(layer_emb=f(weights["layer_emb"]), layer_w=[f(w) for w in weights["layer_w"]],
                    layer_b=[f(b) for b in weights["layer_b"]])
        assert keep["layer_emb"].size == (num_item + K * (D - 1)) * E
        for d in range(D):
            assert keep["layer_w"][d].size == K * (L + d) * E and keep["layer_b"][d].size == K
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        m = N.DrModel()
        m.dtype = 0 if dt == np.float32 else 1
        m.on_device = 0
        m.embed, m.seq_len, m.num_node, m.num_layer, m.num_item = E, L, K, D, num_item
        m.layer_emb = vp(keep["layer_emb"])
        wp = (C.c_void_p * D)(*[vp(w) for w in keep["layer_w"]])
        bp = (C.c_void_p * D)(*[vp(b) for b in keep["layer_b"]])
        m.layer_w, m.layer_b = wp, bp
        if weights.get("rerank_emb") is not None:
            for k in ("rerank_emb", "rerank_w", "rerank_b", "softmax_w", "softmax_b"):
                keep[k] = f(weights[k])
                setattr(m, k, vp(keep[k]))
        self._chk(N.lib().dm_dr_load_model(self._h, C.byref(m)))
        self.dr_dims = dict(E=E, L=L, K=K, D=D, num_item=num_item, dtype=dt)

    def dr_load_model_dev(self, ptrs, E, L, K, D, num_item, dtype=np.float32):
        """like dr_load_model but every entry of `ptrs` is a device pointer (c_void_p); layer_w / layer_b are lists."""
        dt = np.dtype(dtype)
        m = N.DrModel()
        m.dtype = 0 if dt == np.float32 else 1
        m.on_device = 1
        m.embed, m.seq_len, m.num_node, m.num_layer, m.num_item = E, L, K, D, num_item
        m.layer_emb = ptrs["layer_emb"]
        wp = (C.c_void_p * D)(*ptrs["layer_w"])
        bp = (C.c_void_p * D)(*ptrs["layer_b"])
        m.layer_w, m.layer_b = wp, bp
        if ptrs.get("rerank_emb") is not None:
            for k in ("rerank_emb", "rerank_w", "rerank_b", "softmax_w", "softmax_b"):
                setattr(m, k, ptrs[k])
        self._chk(N.lib().dm_dr_load_model(self._h, C.byref(m)))
        self.dr_dims = dict(E=E, L=L, K=K, D=D, num_item=num_item, dtype=dt)

    def dr_load_model_synthetic(self, E, L, K, D, num_item, seed, scale=0.05, rerank=True, dtype=np.float32):
        """Random-init Deep-Retrieval model generated ON THE DEVICE (N(0, scale) matrices, zero biases — the reference's
        init, RerankModel.scala:15-16) and loaded without a host copy (bench only).  dtype float64 (the reference's
        arithmetic type) holds the same draws as float32, widened."""
        dt = np.dtype(dtype)
        fill = lambda n, sd, std: self._fill_new(n, sd, std, dt)
        ptrs = dict(layer_emb=fill((num_item + K * (D - 1)) * E, seed + 1, scale),
                    layer_w=[fill(K * (L + d) * E, seed + 10 + d, scale) for d in range(D)],
                    layer_b=[fill(K, seed + 20 + d, 0.0) for d in range(D)])
        if rerank:
            ptrs.update(rerank_emb=fill(num_item * E, seed + 2, scale), rerank_w=fill(E * L * E, seed + 3, scale),
                        rerank_b=fill(E, seed + 4, 0.0), softmax_w=fill(num_item * E, seed + 5, scale),
                        softmax_b=fill(num_item, seed + 6, 0.0))
        self.dr_load_model_dev(ptrs, E, L, K, D, num_item, dtype=dt)
        self.synchronize()
        for k, v in ptrs.items():
            for q in (v if isinstance(v, list) else [v]):
                self.dev_free(q)

    def _fill_new(self, n, seed, std, dtype=np.float32):
        dt = np.dtype(dtype)
        d = self.dev_alloc(int(n) * dt.itemsize)
        fn = N.lib().dm_fill_normal if dt == np.float32 else N.lib().dm_fill_normal_f64
        self._chk(fn(self._h, d, int(n), 0.0, float(std), int(seed)))
        return d

    def dr_load_path_items(self, path_nodes, item_off, items):
        pn = _i32(path_nodes).reshape(-1, self.dr_dims["D"])
        off = np.ascontiguousarray(item_off, dtype=np.int64)
        it = _i32(items)
        assert off.size == len(pn) + 1
        self._chk(N.lib().dm_dr_load_path_items(self._h, _p(pn, N.i32p), len(pn), _p(off, N.i64p), _p(it, N.i32p)))

    def dr_beam_search(self, seq_ids, beam):
        seq = _i32(seq_ids)
        if seq.ndim == 1:
            seq = seq[None, :]
        U, D = seq.shape[0], self.dr_dims["D"]
        assert seq.shape[1] == self.dr_dims["L"]
        paths = np.empty((U, beam, D), np.int32)
        probs = np.empty((U, beam), np.float64)
        cnt = np.empty(U, np.int32)
        self._chk(N.lib().dm_dr_beam_search(self._h, _p(seq, N.i32p), U, int(beam), _p(paths, N.i32p),
                                            probs.ctypes.data_as(C.POINTER(C.c_double)), _p(cnt, N.i32p)))
        return paths, probs, cnt

    def dr_recommend(self, seq_ids, beam, topk):
        seq = _i32(seq_ids)
        if seq.ndim == 1:
            seq = seq[None, :]
        U = seq.shape[0]
        assert seq.shape[1] == self.dr_dims["L"]
        ids = np.empty((U, topk), np.int32)
        sc = np.empty((U, topk), np.float64)
        cnt = np.empty(U, np.int32)
        self._chk(N.lib().dm_dr_recommend(self._h, _p(seq, N.i32p), U, int(beam), int(topk), _p(ids, N.i32p),
                                          sc.ctypes.data_as(C.POINTER(C.c_double)), _p(cnt, N.i32p)))
        return ids, sc, cnt

    def dr_search_counters(self, reset=True):
        """(exact_layers, wave_fallbacks, reasons[8]) since the last reset: user-layers of the Deep-Retrieval beam search that took the
        exact radix-select path (either route, layer 0 included), user-layers the sliced route's one-wave cut handed to the block
        kernel, and that count by reason (one byte each, so it wraps at 256): [1] sum zero / non-finite, [2] score floor, [3] too many
        blocks, [4] too few survivors, [5] too many survivors, [6] products in the underflow range."""
        slow = C.c_ulonglong(0)
        two = (C.c_ulonglong * 2)()
        lib = N.lib()
        lib.dm_debug_dr_slow_layers.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
        lib.dm_debug_dr_wave_fallbacks.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
        self._chk(lib.dm_debug_dr_slow_layers(self._h, C.byref(slow), int(bool(reset))))
        self._chk(lib.dm_debug_dr_wave_fallbacks(self._h, two, int(bool(reset))))
        return int(slow.value), int(two[0]), [(int(two[1]) >> (8 * i)) & 0xFF for i in range(8)]

    def dr_beam_search_dev(self, d_seq, U, beam, d_paths, d_probs, d_counts):
        self._chk(N.lib().dm_dr_beam_search_dev(self._h, d_seq, U, int(beam), d_paths, d_probs, d_counts))

    def dr_recommend_dev(self, d_seq, U, beam, topk, d_ids, d_scores, d_counts):
        self._chk(N.lib().dm_dr_recommend_dev(self._h, d_seq, U, int(beam), int(topk), d_ids, d_scores, d_counts))

    # ---- Deep-Retrieval M-step: per-item path scores
    def dr_mstep_path_scores(self, seqs, targets, num_candidate_path, trace=False, cap=None):
        """dm_dr_mstep_path_scores: seqs [N, L] internal ids (-1 = padding), targets [N] -> (item_off [num_item + 1], codes [total] int64,
        scores [total] float64, occurrence [num_item]); item v's candidates are codes / scores [item_off[v], item_off[v + 1]), at most
        num_candidate_path, descending by score, ties in ascending path code.  trace=True appends the beams the call aggregated:
        (paths [N, C, D], probs [N, C], counts [N]).  cap: capacity of codes / scores (default: min(N, num_item) * C, always enough)."""
        d = self.dr_dims
        seq = _i32(seqs).reshape(-1, d["L"])
        tg = _i32(targets).reshape(-1)
        assert len(seq) == len(tg)
        n, c = len(seq), int(num_candidate_path)
        if cap is None:
            cap = min(n, d["num_item"]) * max(c, 0)
        f64p = C.POINTER(C.c_double)
        off = np.empty(d["num_item"] + 1, np.int64)
        occ = np.empty(d["num_item"], np.int64)
        codes = np.empty(max(cap, 1), np.int64)
        scores = np.empty(max(cap, 1), np.float64)
        total = np.zeros(1, np.int64)
        tr = None
        if trace:
            tr = (np.empty((n, max(c, 0), d["D"]), np.int32), np.empty((n, max(c, 0)), np.float64), np.empty(n, np.int32))
        self._chk(N.lib().dm_dr_mstep_path_scores(self._h, _p(seq, N.i32p), _p(tg, N.i32p), n, c, int(cap), _p(off, N.i64p), _p(codes, N.i64p),
                                                  _p(scores, f64p), _p(occ, N.i64p), _p(total, N.i64p),
                                                  _p(tr[0], N.i32p) if trace else None, _p(tr[1], f64p) if trace else None,
                                                  _p(tr[2], N.i32p) if trace else None))
        t = int(total[0])
        out = (off, codes[:t].copy(), scores[:t].copy(), occ)
        return out + tr if trace else out

    def dr_mstep_path_scores_dev(self, d_seq, d_targets, n, num_candidate_path, cap, d_item_off, d_codes, d_scores, d_occurrence=None,
                                 d_trace=(None, None, None)):
        """the same on device arrays (ids not range-checked) -> total"""
        total = np.zeros(1, np.int64)
        self._chk(N.lib().dm_dr_mstep_path_scores_dev(self._h, d_seq, d_targets, int(n), int(num_candidate_path), int(cap), d_item_off, d_codes,
                                                      d_scores, d_occurrence, _p(total, N.i64p), d_trace[0], d_trace[1], d_trace[2]))
        return int(total[0])

    # ---- Deep-Retrieval M-step, streaming mode: decayed running path scores
    def dr_mstep_streaming_path_scores(self, seqs, targets, num_candidate_path, decay_factor=0.999, trace=False, cap=None):
        """dm_dr_mstep_streaming_path_scores: the arguments and the result of dr_mstep_path_scores; item v's entries are its running list
        after its last sample (streamingPathScore, folded in ascending sample index): descending by score, ties in ascending path code —
        except for an item with one sample, which keeps that sample's beam as it is."""
        d = self.dr_dims
        seq = _i32(seqs).reshape(-1, d["L"])
        tg = _i32(targets).reshape(-1)
        assert len(seq) == len(tg)
        n, c = len(seq), int(num_candidate_path)
        if cap is None:
            cap = min(n, d["num_item"]) * max(c, 0)
        f64p = C.POINTER(C.c_double)
        off = np.empty(d["num_item"] + 1, np.int64)
        occ = np.empty(d["num_item"], np.int64)
        codes = np.empty(max(cap, 1), np.int64)
        scores = np.empty(max(cap, 1), np.float64)
        total = np.zeros(1, np.int64)
        tr = None
        if trace:
            tr = (np.empty((n, max(c, 0), d["D"]), np.int32), np.empty((n, max(c, 0)), np.float64), np.empty(n, np.int32))
        self._chk(N.lib().dm_dr_mstep_streaming_path_scores(self._h, _p(seq, N.i32p), _p(tg, N.i32p), n, c, float(decay_factor), int(cap), _p(off, N.i64p),
                                                            _p(codes, N.i64p), _p(scores, f64p), _p(occ, N.i64p), _p(total, N.i64p),
                                                            _p(tr[0], N.i32p) if trace else None, _p(tr[1], f64p) if trace else None,
                                                            _p(tr[2], N.i32p) if trace else None))
        t = int(total[0])
        out = (off, codes[:t].copy(), scores[:t].copy(), occ)
        return out + tr if trace else out

    def dr_mstep_streaming_path_scores_dev(self, d_seq, d_targets, n, num_candidate_path, cap, d_item_off, d_codes, d_scores, d_occurrence=None,
                                           d_trace=(None, None, None), decay_factor=0.999):
        """the same on device arrays (ids not range-checked) -> total"""
        total = np.zeros(1, np.int64)
        self._chk(N.lib().dm_dr_mstep_streaming_path_scores_dev(self._h, d_seq, d_targets, int(n), int(num_candidate_path), float(decay_factor), int(cap),
                                                                d_item_off, d_codes, d_scores, d_occurrence, _p(total, N.i64p), d_trace[0], d_trace[1],
                                                                d_trace[2]))
        return int(total[0])

    # ---- Deep-Retrieval M-step: the greedy penalised path assignment
    def dr_mstep_assign_paths(self, item_off, codes, scores, occurrence, num_node, num_layer, num_path_per_item, num_iteration=3, penalty_factor=3e-6,
                              penalty_poly_order=4, seed=0, with_paths=False, trace=False):
        """dm_dr_mstep_assign_paths on the CSR dr_mstep_path_scores returns (needs no model) -> out_codes [num_item, J] int64: the J path
        codes of every item (an item with occurrence 0: random paths from `seed`).  with_paths=True appends (path_codes [P] ascending,
        path_sizes [P] int32): the distinct codes of the CSR and their final sizes; trace=True appends (trace_sel [T, n_hit, J] int32,
        trace_gain [T, n_hit, J]): the chosen candidate position and the computed gain of every decision, hit items in ascending id."""
        off = np.ascontiguousarray(item_off, np.int64).reshape(-1)
        cd = np.ascontiguousarray(codes, np.int64).reshape(-1)
        sc = np.ascontiguousarray(scores, np.float64).reshape(-1)
        oc = np.ascontiguousarray(occurrence, np.int64).reshape(-1)
        ni, total, j, t = len(oc), len(cd), int(num_path_per_item), int(num_iteration)
        assert len(off) == ni + 1 and len(sc) == total
        f64p = C.POINTER(C.c_double)
        out = np.empty((ni, max(j, 0)), np.int64)
        pc = ps = npaths = ts = tg = None
        if with_paths:
            pc, ps, npaths = np.empty(max(total, 1), np.int64), np.empty(max(total, 1), np.int32), np.zeros(1, np.int64)
        if trace:
            nh = int((oc > 0).sum())
            ts, tg = np.zeros((max(t, 0), nh, max(j, 0)), np.int32), np.zeros((max(t, 0), nh, max(j, 0)), np.float64)
        opt = lambda a, ty: _p(a, ty) if a is not None else None
        self._chk(N.lib().dm_dr_mstep_assign_paths(self._h, _p(off, N.i64p), _p(cd, N.i64p), _p(sc, f64p), _p(oc, N.i64p), ni, total, int(num_node), int(num_layer),
                                                   j, t, float(penalty_factor), int(penalty_poly_order), int(seed), _p(out, N.i64p), opt(pc, N.i64p), opt(ps, N.i32p),
                                                   opt(npaths, N.i64p), opt(ts, N.i32p), opt(tg, f64p)))
        res = (out,)
        if with_paths:
            res += (pc[:int(npaths[0])].copy(), ps[:int(npaths[0])].copy())
        if trace:
            res += (ts, tg)
        return res[0] if len(res) == 1 else res

    def dr_mstep_assign_paths_dev(self, d_item_off, d_codes, d_scores, d_occurrence, num_item, total, num_node, num_layer, num_path_per_item, d_out_codes,
                                  num_iteration=3, penalty_factor=3e-6, penalty_poly_order=4, seed=0, d_paths=(None, None), d_trace=(None, None)):
        """the same on device arrays -> the number of distinct paths (None without d_paths = (d_path_codes, d_path_sizes))"""
        npaths = np.zeros(1, np.int64)
        self._chk(N.lib().dm_dr_mstep_assign_paths_dev(self._h, d_item_off, d_codes, d_scores, d_occurrence, int(num_item), int(total), int(num_node), int(num_layer),
                                                       int(num_path_per_item), int(num_iteration), float(penalty_factor), int(penalty_poly_order), int(seed),
                                                       d_out_codes, d_paths[0], d_paths[1], _p(npaths, N.i64p) if d_paths[0] is not None else None,
                                                       d_trace[0], d_trace[1]))
        return int(npaths[0]) if d_paths[0] is not None else None

    def dr_mstep_optimize(self, seqs, targets, num_candidate_path, num_path_per_item, num_iteration=3, train_mode="batch", decay_factor=0.999,
                          penalty_factor=3e-6, penalty_poly_order=4, seed=0):
        """dm_dr_mstep_optimize: the path scores of dr_mstep_path_scores (train_mode "batch") or dr_mstep_streaming_path_scores ("streaming")
        and the assignment on them in one call, nothing but the result leaves the device -> out_codes [num_item, J] int64"""
        if train_mode not in ("batch", "streaming"):
            raise ValueError(train_mode)
        d = self.dr_dims
        seq = _i32(seqs).reshape(-1, d["L"])
        tg = _i32(targets).reshape(-1)
        assert len(seq) == len(tg)
        out = np.empty((d["num_item"], max(int(num_path_per_item), 0)), np.int64)
        self._chk(N.lib().dm_dr_mstep_optimize(self._h, _p(seq, N.i32p), _p(tg, N.i32p), len(seq), int(num_candidate_path), int(train_mode == "streaming"),
                                               float(decay_factor), int(num_path_per_item), int(num_iteration), float(penalty_factor), int(penalty_poly_order),
                                               int(seed), _p(out, N.i64p)))
        return out

    # ---- Deep-Retrieval: the mapping and the training set resident on the device
    def dr_set_item_paths(self, item_paths):
        """item_paths [num_item, J, D] nodes: the table stays on the device and the path -> items CSR is built from it there - what
        dr_load_path_items(*synth.dr_path_items(item_paths)) leaves behind, without the host inversion"""
        d = self.dr_dims
        p = _i32(item_paths)
        if p.ndim != 3 or p.shape[0] != d["num_item"] or p.shape[2] != d["D"]:
            raise ValueError("item_paths must be [num_item, J, D]")
        self._chk(N.lib().dm_dr_set_item_paths(self._h, _p(p, N.i32p), p.shape[1]))

    def dr_train_set_size(self):
        """-> (samples of the resident set, paths per item of the resident table), 0 for what the handle does not hold: the extents of
        the downloads below, asked of the library rather than remembered here"""
        n, j = C.c_int64(0), C.c_int32(0)
        self._chk(N.lib().dm_dr_train_set_size(self._h, C.byref(n), C.byref(j)))
        return int(n.value), int(j.value)

    def dr_path_items_download(self):
        """the path -> items CSR after either loader -> (codes [P] int64 ascending, item_off [P + 1] int64, items [n] int32)"""
        n_paths, n_items = C.c_int64(0), C.c_int64(0)
        self._chk(N.lib().dm_dr_path_items_size(self._h, C.byref(n_paths), C.byref(n_items)))
        codes, off, items = np.empty(n_paths.value, np.int64), np.empty(n_paths.value + 1, np.int64), np.empty(n_items.value, np.int32)
        self._chk(N.lib().dm_dr_path_items_download(self._h, _p(codes, N.i64p), _p(off, N.i64p), _p(items, N.i32p)))
        return codes, off, items

    def dr_item_paths_download(self):
        """the resident item -> paths table [num_item, J, D]"""
        d = self.dr_dims
        out = np.empty((d["num_item"], max(self.dr_train_set_size()[1], 1), d["D"]), np.int32)      # (no table: one row, and the library refuses)
        self._chk(N.lib().dm_dr_item_paths_download(self._h, _p(out, N.i32p), out.size))
        return out

    def dr_train_set_load(self, seqs, targets):
        """seqs [N, L] internal ids (-1 = padding), targets [N]: uploaded once; the order is the identity until dr_train_set_shuffle"""
        seq = _i32(seqs).reshape(-1, self.dr_dims["L"])
        tg = _i32(targets).reshape(-1)
        assert len(seq) == len(tg)
        self._chk(N.lib().dm_dr_train_set_load(self._h, _p(seq, N.i32p), _p(tg, N.i32p), len(tg)))

    def dr_train_set_free(self):
        self._chk(N.lib().dm_dr_train_set_free(self._h))

    def dr_train_set_shuffle(self, seed, epoch):
        """the order of an epoch: sample indices sorted (stable) by splitmix(splitmix(seed ^ splitmix(epoch)) + i)"""
        self._chk(N.lib().dm_dr_train_set_shuffle(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch)))

    def dr_train_set_order(self):
        out = np.empty(max(self.dr_train_set_size()[0], 1), np.int32)                              # (no set: the library refuses)
        self._chk(N.lib().dm_dr_train_set_order_download(self._h, _p(out, N.i32p)))
        return out

    def dr_train_set_forward_backward(self, offset, length, grouped=False):
        """the layer step (grouped: the sample-grouped one) on samples order[offset : offset + length] of the resident set, gathered on
        the device with their targets' paths -> per-layer losses [D]; dr_adam_step / dr_train_sync_gradients follow"""
        loss = np.empty(self.dr_dims["D"], np.float64)
        self._chk(N.lib().dm_dr_train_set_forward_backward(self._h, int(offset), int(length), int(bool(grouped)), loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def dr_train_set_rerank_forward_backward(self, offset, length):
        """the rerank step on the same range, negatives drawn on the device -> the sampled-softmax loss"""
        loss = C.c_double(0.0)
        self._chk(N.lib().dm_dr_train_set_rerank_forward_backward(self._h, int(offset), int(length), C.byref(loss)))
        return float(loss.value)

    def dr_train_set_mstep(self, num_candidate_path, num_iteration=3, train_mode="batch", decay_factor=0.999, penalty_factor=3e-6, penalty_poly_order=4, seed=0):
        """dr_mstep_optimize over the resident set in storage order, J the resident table's; the table and the CSR follow the new codes
        on the device -> out_codes [num_item, J] int64"""
        if train_mode not in ("batch", "streaming"):
            raise ValueError(train_mode)
        out = np.empty((self.dr_dims["num_item"], self.dr_train_set_size()[1]), np.int64)
        self._chk(N.lib().dm_dr_train_set_mstep(self._h, int(num_candidate_path), int(train_mode == "streaming"), float(decay_factor), int(num_iteration),
                                                float(penalty_factor), int(penalty_poly_order), int(seed), _p(out, N.i64p)))
        return out

    # ---- Deep-Retrieval E-step: the layer model's training step
    def dr_train_init(self, lr=1e-3, lr_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
        o = N.AdamOpts(lr, lr_decay, beta1, beta2, eps)
        self._chk(N.lib().dm_dr_train_init(self._h, C.byref(o)))

    def dr_train_free(self):
        self._chk(N.lib().dm_dr_train_free(self._h))

    def dr_train_forward_backward(self, seq_ids, paths):
        """seq_ids [B, L] internal ids (-1 = padding), paths [B, D] nodes: one row per (sample, path of its target item).
        Replaces the gradient with this batch's; -> per-layer losses [D] (float64)."""
        d = self.dr_dims
        seq = _i32(seq_ids).reshape(-1, d["L"])
        pa = _i32(paths).reshape(-1, d["D"])
        assert len(seq) == len(pa)
        loss = np.empty(d["D"], np.float64)
        self._chk(N.lib().dm_dr_train_forward_backward(self._h, _p(seq, N.i32p), _p(pa, N.i32p), len(seq),
                                                       loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def dr_train_forward_backward_dev(self, d_seq, d_paths, B):
        """the same on device arrays (not range-checked) -> per-layer losses [D]"""
        loss = np.empty(self.dr_dims["D"], np.float64)
        self._chk(N.lib().dm_dr_train_forward_backward_dev(self._h, d_seq, d_paths, int(B), loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def _dr_grouped_args(self, seq_ids, paths):
        d = self.dr_dims
        seq = _i32(seq_ids).reshape(-1, d["L"])
        pa = _i32(paths)
        if pa.ndim != 3 or pa.shape[0] != len(seq) or pa.shape[2] != d["D"]:
            raise ValueError("paths must be [S, J, D] with one entry per row of seq_ids")
        return seq, pa, np.empty(d["D"], np.float64)

    def dr_train_forward_backward_grouped(self, seq_ids, paths):
        """seq_ids [S, L] internal ids (-1 = padding), paths [S, J, D] nodes: every sample once, with the J paths of its target item
        (DESIGN.md §24).  The gradient of dr_train_forward_backward on the expanded batch (np.repeat(seq_ids, J), paths.reshape(-1, D)),
        each history product computed once per sample; -> per-layer losses [D] (float64), the mean over the S J rows."""
        seq, pa, loss = self._dr_grouped_args(seq_ids, paths)
        self._chk(N.lib().dm_dr_train_forward_backward_grouped(self._h, _p(seq, N.i32p), _p(pa, N.i32p), len(seq), pa.shape[1],
                                                               loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def dr_train_forward_backward_grouped_dev(self, d_seq, d_paths, S, J):
        """the same on device arrays [S, L] and [S, J, D] (not range-checked) -> per-layer losses [D]"""
        loss = np.empty(self.dr_dims["D"], np.float64)
        self._chk(N.lib().dm_dr_train_forward_backward_grouped_dev(self._h, d_seq, d_paths, int(S), int(J), loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def dr_layer_loss(self, seq_ids, paths):
        """Evaluator.evaluateLayerModel: the per-layer cross-entropy [D] of seq_ids [S, L] with paths [S, J, D], the mean over the S J
        rows.  Forward only; needs no dr_train_init and leaves gradient and optimizer state alone."""
        seq, pa, loss = self._dr_grouped_args(seq_ids, paths)
        self._chk(N.lib().dm_dr_layer_loss(self._h, _p(seq, N.i32p), _p(pa, N.i32p), len(seq), pa.shape[1], loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def dr_adam_step(self, grad_scale=1.0):
        self._chk(N.lib().dm_dr_adam_step(self._h, float(grad_scale)))

    def dr_train_sync_gradients(self):
        """LocalOptimizer.syncGradients for the Deep-Retrieval layer model over the attached communicator (dm_dr_train_sync_gradients,
        DESIGN.md §22; collective: every rank calls it, a rank that ran no step included).  Afterwards every replica's gradient is the
        rank-ordered sum, in the model's dtype, of the ranks' gradients; dr_adam_step(1 / P) follows.  train_sync_stats() says what it moved."""
        self._chk(N.lib().dm_dr_train_sync_gradients(self._h))

    def dr_train_param_count(self):
        n = C.c_int64(0)
        self._chk(N.lib().dm_dr_train_param_count(self._h, C.byref(n)))
        return int(n.value)

    def dr_train_download(self, what="weights"):
        """The trainable vector [layer_emb ; W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}] ("weights"), its gradient ("grad") or an Adam
        moment ("s", "r"), in the model's dtype."""
        n = self.dr_train_param_count()
        out = np.empty(n, self.dr_dims["dtype"])
        self._chk(N.lib().dm_dr_train_download(self._h, {"weights": 0, "grad": 1, "s": 2, "r": 3}[what], out.ctypes.data_as(C.c_void_p), n))
        return out

    # ---- DeepFM: the training step
    def deepfm_train_init(self, lr=1e-3, lr_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
        o = N.AdamOpts(lr, lr_decay, beta1, beta2, eps)
        self._chk(N.lib().dm_deepfm_train_init(self._h, C.byref(o)))

    def deepfm_train_free(self):
        self._chk(N.lib().dm_deepfm_train_free(self._h))

    def deepfm_train_forward_backward(self, codes, seqs, labels):
        """codes [B], seqs [B, L] node codes (-1 = a zero row), labels [B].  Replaces the gradient with this batch's; -> the mean
        BCE-with-logits loss (float64)."""
        codes = _i32(codes).ravel()
        B = codes.size
        seqs = _i32(seqs).reshape(B, -1) if B else _i32(seqs).reshape(0, 1)
        lab = np.ascontiguousarray(labels, np.float32).ravel()
        assert lab.size == B
        loss = C.c_double(0)
        self._chk(N.lib().dm_deepfm_train_forward_backward(self._h, _p(codes, N.i32p), _p(seqs, N.i32p), _p(lab, N.f32p), B,
                                                           seqs.shape[1], C.byref(loss)))
        return loss.value

    def deepfm_train_forward_backward_dev(self, d_codes, d_seqs, d_labels, B, L):
        """the same on device arrays (not range-checked) -> the mean loss"""
        loss = C.c_double(0)
        self._chk(N.lib().dm_deepfm_train_forward_backward_dev(self._h, d_codes, d_seqs, d_labels, int(B), int(L), C.byref(loss)))
        return loss.value

    def deepfm_train_forward_backward_grouped(self, seq_codes, codes, labels):
        """The same step on a user-grouped batch (dm_deepfm_train_forward_backward_grouped_dev): seq_codes [U][L],
        codes / labels [U][R] — a user's R candidate rows share the user's history, which is read once.  Uploads and calls the device
        entry (ids are not range-checked: one outside [0, num_index) reads as -1); -> the mean loss (float64)."""
        seq = _i32(seq_codes)
        U, L = seq.shape if seq.ndim == 2 else (0, 1)
        codes = _i32(codes).reshape(U, -1) if U else _i32(codes).reshape(0, 1)
        R = codes.shape[1]
        lab = np.ascontiguousarray(labels, np.float32).reshape(U, R)
        al = lambda v: (v + 255) & ~255
        buf = self.dev_alloc(al(U * L * 4) + 2 * al(U * R * 4) + 256)
        try:
            d_seq = C.c_void_p(buf.value)
            d_codes = C.c_void_p(buf.value + al(U * L * 4))
            d_lab = C.c_void_p(d_codes.value + al(U * R * 4))
            if U and R:
                self.h2d(d_seq, seq); self.h2d(d_codes, codes); self.h2d(d_lab, lab)
            return self.deepfm_train_forward_backward_grouped_dev(d_seq, d_codes, d_lab, U, R, L)
        finally:
            self.dev_free(buf)

    def deepfm_train_forward_backward_grouped_dev(self, d_seq_codes, d_codes, d_labels, U, R, L):
        """the same on device arrays: d_seq_codes [U][L], d_codes / d_labels [U * R] user-major -> the mean loss"""
        loss = C.c_double(0)
        self._chk(N.lib().dm_deepfm_train_forward_backward_grouped_dev(self._h, d_seq_codes, d_codes, d_labels, int(U), int(R), int(L),
                                                                       C.byref(loss)))
        return loss.value

    def deepfm_train_forward_backward_csr(self, seq_codes, row_off, codes, labels):
        """The same step on a ragged user-grouped batch (dm_deepfm_train_forward_backward_csr_dev): seq_codes [U][L],
        row_off [U + 1] (int64), codes / labels [B] — rows row_off[u] .. row_off[u + 1] are user u's and share its history; a user may
        have none.  Checks the offsets here (ValueError), uploads and calls the device entry, which checks them again on the device
        (ids are not range-checked: one outside [0, num_index) reads as -1); -> the mean loss (float64)."""
        seq = _i32(seq_codes)
        U, L = seq.shape if seq.ndim == 2 else (0, 1)
        off = np.ascontiguousarray(row_off, np.int64).ravel()
        codes = _i32(codes).ravel()
        B = codes.size
        lab = np.ascontiguousarray(labels, np.float32).ravel()
        if off.size != U + 1 or lab.size != B:
            raise ValueError("deepfm_train_forward_backward_csr: row_off must hold U + 1 offsets and labels one value per row")
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != B:
            bad = 0 if off[0] != 0 else int(np.flatnonzero(np.diff(off) < 0)[0]) if (np.diff(off) < 0).any() else U
            raise ValueError("deepfm_train_forward_backward_csr: row_off must start at 0, never decrease and end at B = %d "
                             "(first offending user %d)" % (B, bad))
        al = lambda v: (v + 255) & ~255
        buf = self.dev_alloc(al(U * L * 4) + al((U + 1) * 8) + 2 * al(B * 4) + 256)
        try:
            d_seq = C.c_void_p(buf.value)
            d_off = C.c_void_p(buf.value + al(U * L * 4))
            d_codes = C.c_void_p(d_off.value + al((U + 1) * 8))
            d_lab = C.c_void_p(d_codes.value + al(B * 4))
            if U:
                self.h2d(d_seq, seq); self.h2d(d_off, off)
            if B:
                self.h2d(d_codes, codes); self.h2d(d_lab, lab)
            return self.deepfm_train_forward_backward_csr_dev(d_seq, d_off, d_codes, d_lab, U, B, L)
        finally:
            self.dev_free(buf)

    def deepfm_train_forward_backward_csr_dev(self, d_seq_codes, d_row_off, d_codes, d_labels, U, B, L):
        """the same on device arrays: d_seq_codes [U][L], d_row_off [U + 1] int64, d_codes / d_labels [B] -> the mean loss"""
        loss = C.c_double(0)
        self._chk(N.lib().dm_deepfm_train_forward_backward_csr_dev(self._h, d_seq_codes, d_row_off, d_codes, d_labels, int(U), int(B), int(L),
                                                                   C.byref(loss)))
        return loss.value

    def deepfm_sample_train_batch_csr(self, seq_item_ids, target_item_ids, neg_counts, start_level=1, seed=0, with_prob=False, tolerance=20):
        """dm_deepfm_sample_train_batch_csr_dev, downloaded (for the tests): (codes [R], labels [R], seq_codes [T, L], row_off [T + 1])."""
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), 0, int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_deepfm_sample_train_batch_csr_dev(self._h, None, None, T, L, _p(neg, N.i32p), neg.size, C.byref(o), None, None,
                                                               None, None, 0, C.byref(n)))
        R = max(n.value, 1)
        al = lambda v: (v + 255) & ~255
        buf = self.dev_alloc(2 * al(T * L * 4) + al(T * 4) + 2 * al(R * 4) + al((T + 1) * 8) + 256)
        try:
            base = buf.value
            d_seq = C.c_void_p(base); base += al(T * L * 4)
            d_tgt = C.c_void_p(base); base += al(T * 4)
            d_codes = C.c_void_p(base); base += al(R * 4)
            d_sc = C.c_void_p(base); base += al(T * L * 4)
            d_off = C.c_void_p(base); base += al((T + 1) * 8)
            d_lab = C.c_void_p(base)
            if T:
                self.h2d(d_seq, seq); self.h2d(d_tgt, tgt)
            self._chk(N.lib().dm_deepfm_sample_train_batch_csr_dev(self._h, d_seq, d_tgt, T, L, _p(neg, N.i32p), neg.size, C.byref(o), d_codes,
                                                                   d_sc, d_off, d_lab, R, C.byref(n)))
            R = n.value
            codes = np.empty(R, np.int32); lab = np.empty(R, np.float32); sc = np.empty((T, L), np.int32); off = np.empty(T + 1, np.int64)
            if R:
                self.d2h(codes, d_codes); self.d2h(lab, d_lab)
            self.d2h(off, d_off)
            if T:
                self.d2h(sc, d_sc)
            return codes, lab, sc, off
        finally:
            self.dev_free(buf)

    def deepfm_make_train_batch(self, seq_item_ids, target_item_ids, neg_counts, start_level=1, seed=0, with_prob=False, tolerance=20):
        """make_train_batch for a DeepFM model (no mask): (codes [R], seqs [R, L], labels [R])."""
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), 0, int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_deepfm_make_train_batch(self._h, _p(seq, N.i32p), _p(tgt, N.i32p), T, L, _p(neg, N.i32p), neg.size,
                                                     C.byref(o), None, None, None, 0, C.byref(n)))
        R = n.value
        codes = np.empty(max(R, 1), np.int32); seqs = np.empty((max(R, 1), L), np.int32); lab = np.empty(max(R, 1), np.float32)
        self._chk(N.lib().dm_deepfm_make_train_batch(self._h, _p(seq, N.i32p), _p(tgt, N.i32p), T, L, _p(neg, N.i32p), neg.size,
                                                     C.byref(o), _p(codes, N.i32p), _p(seqs, N.i32p), _p(lab, N.f32p), R, C.byref(n)))
        R = n.value
        return codes[:R], seqs[:R], lab[:R]

    def deepfm_train_step_sampled(self, seq_item_ids, target_item_ids, neg_counts, start_level=1, seed=0, with_prob=False, tolerance=20,
                                  return_rows=False, grouped=False):
        """train_step_sampled for a DeepFM model: dm_deepfm_sample_train_batch_dev expands the targets on the device straight into
        the buffers of dm_deepfm_train_forward_backward_dev.  Returns the mean BCE loss of the expanded rows (with return_rows: and
        the rows (codes, seqs, labels), downloaded).
        grouped: dm_deepfm_sample_train_batch_csr_dev into the buffers of dm_deepfm_train_forward_backward_csr_dev instead (DESIGN.md
        §17) — the same rows from the same seed, every target's history written and read once; the [R][L] row histories are never
        carved (return_rows then gives (codes, seq_codes [T, L], labels, row_off [T + 1]))."""
        if grouped:
            return self._deepfm_train_step_sampled_csr(seq_item_ids, target_item_ids, neg_counts, start_level, seed, with_prob, tolerance,
                                                       return_rows)
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), 0, int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_deepfm_sample_train_batch_dev(self._h, None, None, T, L, _p(neg, N.i32p), neg.size, C.byref(o), None, None,
                                                           None, 0, C.byref(n)))
        R = max(n.value, 1)
        al = lambda v: (v + 255) & ~255
        need = al(T * L * 4) + al(T * 4) + al(R * 4) + al(R * L * 4) + al(R * 4)        # the five sub-buffers as carved below
        if getattr(self, "_samp_bytes", 0) < need:
            if getattr(self, "_samp_buf", None):
                self.dev_free(self._samp_buf)
            self._samp_buf, self._samp_bytes = self.dev_alloc(need + need // 2), need + need // 2
        base = self._samp_buf.value
        d_seq = C.c_void_p(base); base += al(T * L * 4)
        d_tgt = C.c_void_p(base); base += al(T * 4)
        d_codes = C.c_void_p(base); base += al(R * 4)
        d_seqs = C.c_void_p(base); base += al(R * L * 4)
        d_lab = C.c_void_p(base)
        self.h2d(d_seq, seq); self.h2d(d_tgt, tgt)
        self._chk(N.lib().dm_deepfm_sample_train_batch_dev(self._h, d_seq, d_tgt, T, L, _p(neg, N.i32p), neg.size, C.byref(o), d_codes,
                                                           d_seqs, d_lab, R, C.byref(n)))
        R = n.value
        loss = C.c_double(0)
        if R:
            self._chk(N.lib().dm_deepfm_train_forward_backward_dev(self._h, d_codes, d_seqs, d_lab, R, L, C.byref(loss)))
        if not return_rows:
            return loss.value
        codes = np.empty(R, np.int32); seqs = np.empty((R, L), np.int32); lab = np.empty(R, np.float32)
        if R:
            self.d2h(codes, d_codes); self.d2h(seqs, d_seqs); self.d2h(lab, d_lab)
        return loss.value, (codes, seqs, lab)

    def _deepfm_train_step_sampled_csr(self, seq_item_ids, target_item_ids, neg_counts, start_level, seed, with_prob, tolerance, return_rows):
        seq = _i32(seq_item_ids)
        tgt = _i32(target_item_ids).ravel()
        T, L = seq.shape
        neg = _i32(neg_counts)
        o = N.SampleOpts(int(start_level), int(bool(with_prob)), int(tolerance), 0, int(seed))
        n = C.c_int64(0)
        self._chk(N.lib().dm_deepfm_sample_train_batch_csr_dev(self._h, None, None, T, L, _p(neg, N.i32p), neg.size, C.byref(o), None, None,
                                                               None, None, 0, C.byref(n)))
        R = max(n.value, 1)
        al = lambda v: (v + 255) & ~255
        need = 2 * al(T * L * 4) + al(T * 4) + 2 * al(R * 4) + al((T + 1) * 8)          # the six sub-buffers as carved below: no [R][L]
        if getattr(self, "_samp_bytes", 0) < need:
            if getattr(self, "_samp_buf", None):
                self.dev_free(self._samp_buf)
            self._samp_buf, self._samp_bytes = self.dev_alloc(need + need // 2), need + need // 2
        base = self._samp_buf.value
        d_seq = C.c_void_p(base); base += al(T * L * 4)
        d_tgt = C.c_void_p(base); base += al(T * 4)
        d_codes = C.c_void_p(base); base += al(R * 4)
        d_sc = C.c_void_p(base); base += al(T * L * 4)
        d_off = C.c_void_p(base); base += al((T + 1) * 8)
        d_lab = C.c_void_p(base)
        self.h2d(d_seq, seq); self.h2d(d_tgt, tgt)
        self._chk(N.lib().dm_deepfm_sample_train_batch_csr_dev(self._h, d_seq, d_tgt, T, L, _p(neg, N.i32p), neg.size, C.byref(o), d_codes,
                                                               d_sc, d_off, d_lab, R, C.byref(n)))
        R = n.value
        loss = C.c_double(0)
        if R:
            self._chk(N.lib().dm_deepfm_train_forward_backward_csr_dev(self._h, d_sc, d_off, d_codes, d_lab, T, R, L, C.byref(loss)))
        if not return_rows:
            return loss.value
        codes = np.empty(R, np.int32); lab = np.empty(R, np.float32); sc = np.empty((T, L), np.int32); off = np.empty(T + 1, np.int64)
        if R:
            self.d2h(codes, d_codes); self.d2h(lab, d_lab)
        self.d2h(sc, d_sc); self.d2h(off, d_off)
        return loss.value, (codes, sc, lab, off)

    def deepfm_adam_step(self, grad_scale=1.0):
        self._chk(N.lib().dm_deepfm_adam_step(self._h, float(grad_scale)))

    def deepfm_train_sync_gradients(self):
        """LocalOptimizer.syncGradients for a DeepFM model over the attached communicator (dm_deepfm_train_sync_gradients, DESIGN.md
        §19; collective: every rank calls it, a rank whose batch was empty included).  Afterwards every replica's gradient is the
        rank-ordered fp32 sum of the ranks' gradients; deepfm_adam_step(1 / world) follows.  train_sync_stats() says what it moved."""
        self._chk(N.lib().dm_deepfm_train_sync_gradients(self._h))

    def deepfm_train_param_count(self):
        n = C.c_int64(0)
        self._chk(N.lib().dm_deepfm_train_param_count(self._h, C.byref(n)))
        return int(n.value)

    def deepfm_train_download(self, what="weights"):
        """The trained vector [emb ; l1.W ; l1.b ; l2.W ; l2.b] ("weights"), its gradient ("grad") or an Adam moment ("s", "r"), in
        the model's own (unpadded) layout, float32."""
        n = self.deepfm_train_param_count()
        out = np.empty(n, np.float32)
        self._chk(N.lib().dm_deepfm_train_download(self._h, {"weights": 0, "grad": 1, "s": 2, "r": 3}[what], _p(out, N.f32p), n))
        return out

    # ---- Deep-Retrieval E-step: the rerank model's training step
    def dr_rerank_train_init(self, num_sampled, seed=0, accumulate=True, lr=1e-3, lr_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8, softmax=None):
        """graph optimizer from the keywords; softmax: None (the reference's criterion optimizer: lr, 0.9, 0.999, eps 1e-7, no decay) or a
        dict(lr, lr_decay, beta1, beta2, eps)"""
        g = N.AdamOpts(lr, lr_decay, beta1, beta2, eps)
        sm = None if softmax is None else C.byref(N.AdamOpts(softmax["lr"], softmax.get("lr_decay", 0.0), softmax.get("beta1", 0.9),
                                                            softmax.get("beta2", 0.999), softmax.get("eps", 1e-7)))
        self._chk(N.lib().dm_dr_rerank_train_init(self._h, C.byref(g), sm, int(num_sampled), int(seed), 1 if accumulate else 0))
        self._dr_num_sampled = int(num_sampled)

    def dr_rerank_train_free(self):
        self._chk(N.lib().dm_dr_rerank_train_free(self._h))

    def dr_rerank_forward_backward(self, seq_ids, targets, negatives=None):
        """seq_ids [B, L] internal ids (-1 = padding), targets [B], negatives [B, num_sampled] or None (the device draws them).
        Replaces the graph's gradient, adds to (accumulate) or replaces the softmax tables'; -> the sampled-softmax loss (float)."""
        seq = _i32(seq_ids).reshape(-1, self.dr_dims["L"])
        tg = _i32(targets).reshape(-1)
        assert len(seq) == len(tg)
        neg = None
        if negatives is not None:
            neg = _i32(negatives).reshape(len(tg), self._dr_num_sampled)
        loss = C.c_double(0.0)
        self._chk(N.lib().dm_dr_rerank_forward_backward(self._h, _p(seq, N.i32p), _p(tg, N.i32p), None if neg is None else _p(neg, N.i32p),
                                                        len(seq), C.byref(loss)))
        return float(loss.value)

    def dr_rerank_forward_backward_dev(self, d_seq, d_targets, d_negatives, B):
        """the same on device arrays (not range-checked); d_negatives may be None"""
        loss = C.c_double(0.0)
        self._chk(N.lib().dm_dr_rerank_forward_backward_dev(self._h, d_seq, d_targets, d_negatives, int(B), C.byref(loss)))
        return float(loss.value)

    def dr_rerank_sample(self, targets, step):
        """the negatives the device draws for `targets` at forward/backward call number `step` (0-based) -> [B, num_sampled]"""
        tg = _i32(targets).reshape(-1)
        out = np.empty((len(tg), self._dr_num_sampled), np.int32)
        self._chk(N.lib().dm_dr_rerank_sample(self._h, _p(tg, N.i32p), len(tg), int(step), _p(out, N.i32p)))
        return out

    def dr_rerank_adam_step(self, grad_scale=1.0):
        self._chk(N.lib().dm_dr_rerank_adam_step(self._h, float(grad_scale)))

    def dr_rerank_sizes(self):
        """lengths of the two trainable vectors: {"graph": [rerank_emb ; rerank_w ; rerank_b], "softmax": [softmax_w ; softmax_b]}"""
        d = self.dr_dims
        return {"graph": d["num_item"] * d["E"] + d["E"] * d["L"] * d["E"] + d["E"], "softmax": d["num_item"] * d["E"] + d["num_item"]}

    def dr_rerank_download(self, vec="graph", what="weights"):
        """one of the two trainable vectors ("graph", "softmax"): its weights, gradient ("grad") or an Adam moment ("s", "r")"""
        n = self.dr_rerank_sizes()[vec]
        out = np.empty(n, self.dr_dims["dtype"])
        self._chk(N.lib().dm_dr_rerank_download(self._h, {"graph": 0, "softmax": 1}[vec], {"weights": 0, "grad": 1, "s": 2, "r": 3}[what],
                                                out.ctypes.data_as(C.c_void_p), n))
        return out

    def dr_rerank_full_loss(self, seq_ids, targets):
        """Evaluator.evaluateReRankModel: -mean log softmax over ALL items at the target"""
        seq = _i32(seq_ids).reshape(-1, self.dr_dims["L"])
        tg = _i32(targets).reshape(-1)
        assert len(seq) == len(tg)
        out = C.c_double(0.0)
        self._chk(N.lib().dm_dr_rerank_full_loss(self._h, _p(seq, N.i32p), _p(tg, N.i32p), len(seq), C.byref(out)))
        return float(out.value)

    # ---- device-resident path (bench)
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(N.lib().dm_dev_alloc(self._h, nbytes, C.byref(p)))
        return p

    def dev_free(self, p):
        self._chk(N.lib().dm_dev_free(self._h, p))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(N.lib().dm_memcpy_h2d(self._h, dptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def d2h(self, arr, dptr):
        self._chk(N.lib().dm_memcpy_d2h(self._h, arr.ctypes.data_as(C.c_void_p), dptr, arr.nbytes))

    def tdm_beam_search_dev(self, d_seq, U, L, beam, topk, d_ids, d_scores, d_counts, use_mask=True):
        opts = N.SearchOpts(int(beam), int(topk), int(bool(use_mask)), 0)
        self._chk(N.lib().dm_tdm_beam_search_dev(self._h, d_seq, U, L, C.byref(opts), None, None, d_ids, d_scores,
                                                 d_counts))

    def otm_beam_search_dev(self, d_seq, U, L, beam, leaf_level, d_ids, d_scores, d_counts):
        fn = N.lib().dm_deepfm_otm_beam_search_dev if self.scorer == "deepfm" else N.lib().dm_otm_beam_search_dev
        self._chk(fn(self._h, d_seq, U, L, int(beam), int(leaf_level), d_ids, d_scores, d_counts))

    def synchronize(self):
        self._chk(N.lib().dm_synchronize(self._h))

    _SCORER = {"f32": 0, "split_f16": 1, "auto": 2, "f64": 3}

    def set_scorer_mode(self, mode):
        """Arithmetic of the beam-search scorer: "f32" (fp32-input MFMA), "split_f16" (fp16 hi/lo operand split on the
        fp16 matrix pipe, fp32 accumulation) or "auto" (default: split_f16 where E allows); include/dismember_hip.h."""
        self._chk(N.lib().dm_set_scorer_mode(self._h, int(self._SCORER.get(mode, mode))))

    def scorer_mode(self):
        m, eff, se, sw = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(N.lib().dm_get_scorer_mode(self._h, C.byref(m), C.byref(eff), C.byref(se), C.byref(sw)))
        names = {v: k for k, v in self._SCORER.items()}
        return {"mode": names[eff.value], "setting": names[m.value], "shift_emb": se.value, "shift_w": sw.value}

    def timing_reset(self):
        self._chk(N.lib().dm_kernel_timing_reset(self._h))

    def timing_get(self):
        n, ms = C.c_int(0), C.c_double(0)
        self._chk(N.lib().dm_kernel_timing_get(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def timing_get_kind(self, kind):
        """launches and summed milliseconds of one kind of launch, as the library's EvKind names them (csrc/host_request.hip.inc):
        0 = a search's main kernel, a whole Deep-Retrieval search and every launch without a kind of its own; 1 = the second pass over
        the users the one-wave beam kernel deferred; under DM_DR_TIME_LAUNCHES=1 the sliced Deep-Retrieval search's launches, per
        layer d: 11 = layer 0, 10 + 2d = statistics, 11 + 2d = cut, 21 + 2d = the block version's second pass; 30 = general rows
        (din_forward); 40 / 41 = DeepFM user / level launches, 42 / 43 = the DeepFM pair scorer's per-history set-up / per-pair launches
        (JTM tree learning), 42 also the fused OTM beam search of a DeepFM model, 44 / 45 the unit scores / segment sums of OTM tree construction with a DeepFM
        model, and 40 .. 44 the launches of the grouped fp64 training step; under
        DM_DR_TIME_LAUNCHES=1 the Deep-Retrieval training step: 50 = forward GEMMs, 51 = softmax + cross-entropy, 52 = dX products,
        53 = dW / db products and slab sums, 54 = embedding gradient (pairs, sort, segment sums), 55 = Adam; and the M-step's path scores:
        80 = pairs of a chunk, 81 = the (item, path) sort, 82 = segment heads, 83 = segment sums, 84 = sort by score, 85 = sort by item,
        86 = the cut at C, 87 = codes / scores / offsets, 88 = occurrences; under DM_DFM_TIME_LAUNCHES=1 the DeepFM training step
        (70 .. 76) and its gradient exchange across ranks: 77 = this rank's unique rows and block, 78 = the rank-ordered sums after
        the all-gather; under DM_TRAIN_TIME_LAUNCHES=1 the ragged user-grouped DIN training step: 56 = per-user set-up, 57 = rows kernel,
        58 = per-user backward, 59 = dense gradients (column sums, three products and their slab sums), 68 = table gradient"""
        n, ms = C.c_int(0), C.c_double(0)
        self._chk(N.lib().dm_kernel_timing_get_kind(self._h, int(kind), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def last_beam_kernel(self):
        return (N.lib().dm_last_beam_kernel(self._h) or b"").decode()

    def g_table_state(self):
        """dm_debug_g_table: whether the last search on the one-wave-per-SIMD kernel read the per-row setup table (DM_G_TABLE),
        whether the owner's table is current, and its size in bytes."""
        used, cur, nbytes = C.c_int(0), C.c_int(0), C.c_ulonglong(0)
        fn = N.lib().dm_debug_g_table
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
        self._chk(fn(self._h, C.byref(used), C.byref(cur), C.byref(nbytes)))
        return {"used_last": bool(used.value), "current": bool(cur.value), "bytes": nbytes.value}

    def last_scored_rows(self):
        r = C.c_int64(0)
        self._chk(N.lib().dm_last_scored_rows(self._h, C.byref(r)))
        return r.value
