/*
 * dismember_hip.h — C ABI of libdismember_hip.so, the MI355X (gfx950) native
 * implementation of dismember's tree beam-search retrieval hot path.
 *
 * This is the drop-in boundary: every entry point names the
 * reference interface it replaces.  The reference has no FFI of its own for
 * this path (it is pure Scala calling MKL through BigDL's JNI); these are the
 * functions a JNI shim binds so that the Scala facades
 *   TDM.recommend            tdm/src/main/scala/com/mass/tdm/model/TDM.scala:17-22
 *   Recommender.recommendItems  tdm/.../model/Recommender.scala:18-37
 *   OTM.recommend            otm/src/main/scala/com/mass/otm/model/OTM.scala:14-22
 *   Module.forward           scalann/.../nn/abstractnn/AbstractModule.scala:19-41
 * keep their signatures.
 *
 * Conventions
 *   - every function returns 0 (DM_OK) or a negative dm_status; the message of
 *     the last failure on a handle is dm_last_error(h).  No exception crosses
 *     the boundary.
 *   - plain pointers and sizes only.  Host pointers are caller-owned and only
 *     read/written during the call.  Device memory is owned by the handle.
 *   - one handle per (device, stream); a handle is thread-compatible (one host
 *     thread at a time), like one cloned Module in the reference
 *     (tdm/.../optim/LocalOptimizer.scala:28-44).
 *   - there is NO CPU fallback: without a usable HIP device dm_create fails.
 *   - T/ = tdm/src/main/scala/com/mass/tdm/, O/ = otm/src/main/scala/com/mass/otm/,
 *     S/ = scalann/src/main/scala/com/mass/scalann/ in the citations below.
 */
#ifndef DISMEMBER_HIP_H
#define DISMEMBER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dm_ctx *dm_handle_t;

typedef enum {
  DM_OK = 0,
  DM_ERR_INVALID = -1,     /* bad argument (the reference's `require` failures) */
  DM_ERR_HIP = -2,         /* HIP runtime error */
  DM_ERR_STATE = -3,       /* tree / weights not loaded yet */
  DM_ERR_INDEX = -4,       /* embedding index out of range (LookupTable.scala:47-53 throws) */
  DM_ERR_UNSUPPORTED = -5  /* shape outside what the kernels are built for */
} dm_status;

typedef enum { DM_F32 = 0, DM_F64 = 1 } dm_dtype;

/* ---- lifetime ---------------------------------------------------------- */
int dm_version(void);
int dm_device_count(int *count);
int dm_create(int device_id, dm_handle_t *out);
int dm_destroy(dm_handle_t h);
/* A second handle on the same device that READS the tree, the id maps, the weights and every derived copy (fragment orders, split
 * planes, the pre-split table) of `h` — the same device memory, nothing is copied — through its own stream, request arenas and
 * workspace: the reference's `cloneModule()` workers share one weight storage (tdm/.../optim/LocalOptimizer.scala:28-44, pinned by
 * otm/src/test/scala/CloneModelSpec.scala:20-36).  One host thread per handle, as everywhere; searches through `h` and its clones run
 * concurrently.  Loading and training go through the owning handle only (DM_ERR_STATE on a clone); a clone sees the new weights at its
 * next call.  Weight updates must not overlap a clone's search in flight (the reference's workers meet at a barrier before the update,
 * LocalOptimizer.scala:73-80).  Destroy the clones before the owner (dm_destroy(owner) fails with DM_ERR_STATE while clones exist).
 * A clone of a clone shares the same owner.  The Deep-Retrieval model is per handle (not shared). */
int dm_clone(dm_handle_t h, dm_handle_t *clone);

const char *dm_last_error(dm_handle_t h); /* h may be NULL: last create-time error */
int dm_synchronize(dm_handle_t h);        /* hipStreamSynchronize on the handle's stream */

/* ---- index structures (replaces TDMOp.tree, T/operator/TDMOp.scala:18-19,61-82) ---- */

/* codeNodeMap (T/tree/DistTree.scala:40-87): one entry per tree node.
 * codes[i] = heap code, node_ids[i] = Node.id, is_leaf[i] = Node.is_leaf. */
int dm_load_tree_tdm(dm_handle_t h, const int32_t *codes, const int32_t *node_ids, const uint8_t *is_leaf,
                     int64_t n_nodes, int max_level);
/* idCodeMap + nonLeafOffset + maxCode (DistTree.loadItems, T/tree/DistTree.scala:26-38) */
int dm_load_id_maps(dm_handle_t h, const int32_t *leaf_item_ids, const int32_t *leaf_codes, int64_t n);
/* TDM.loadTree / TDMOp.initTree(treePbPath) (T/model/TDM.scala:50-52, T/operator/TDMOp.scala:61-82): the reference's own tree file —
 * [int32 BE length][KVItem] records written by TreeBuilder.build (T/tree/TreeBuilder.scala:23-101) / JTMTree.writeTree, read by
 * DistTree.loadData (T/tree/DistTree.scala:40-87) — parsed in the library: dm_load_tree_tdm + dm_load_id_maps + dm_tdm_set_node_probs. */
int dm_load_tree_file(dm_handle_t h, const char *path);
/* TDMTree.idToCode (T/tree/TDMTree.scala:35-56); host-side helper, same logic the kernels run on device */
int dm_tdm_id_to_code(dm_handle_t h, const int32_t *item_ids, int n, int32_t *codes, int32_t *mask_pos,
                      int *n_mask);
/* Recommender.getLevelStart (T/model/Recommender.scala:210-216) in integer arithmetic */
int dm_level_start(int candidate_num, int *start_code, int *level);

/* ---- scorer weights (replaces Serialization.loadModel + DIN.buildModel) ---- */

/* compact parameter vector in Graph.parameters order (S/nn/graphnn/Graph.scala:37-48,
 * S/nn/mixin/Module.scala:9-45; DIN: T/model/DIN.scala:18-42):
 *   [emb num_index x E ; att.W E x E ; l1.W E x 2E ; l1.b E ; l2.W 1 x E ; l2.b 1]
 * E: any size 1..128 (the reference's embedSize is free).  The kernels are built for 16 / 32 / 64 / 128; other sizes are zero-padded to
 * the next of them on the device (same function: zero columns change no product, the softmax scale stays 1 / sqrt(E)); every vector
 * that crosses the boundary (this one, dm_train_download, the checkpoint) keeps the MODEL's layout.  dm_load_weights_din_dev* and the
 * raw device-pointer exchange (dm_train_dense_block / _export_rows / _add_rows) take native sizes only. */
int dm_load_weights_din(dm_handle_t h, int dtype, int E, int64_t num_index, const void *compact,
                        int64_t n_elems);

/* The reference's second node scorer, DeepFM (T/model/DeepFM.scala:11-45; `deep_model DeepFM` in the TDM conf files); training: dm_deepfm_train_*, below:
 * compact vector in Graph.parameters order (S/nn/graphnn/Graph.scala:37-48; EmbeddingShare DeepFM.scala:18, Linear :35, Linear :39 —
 * FM holds no parameters), T = L + 1:
 *   [emb num_index x E ; l1.W T x (T E) ; l1.b T ; l2.W 1 x T ; l2.b 1]          n_elems = num_index E + T T E + 2 T + 1
 * dtype: DM_F32 only (DM_F64 -> DM_ERR_UNSUPPORTED).  E 1..128, zero-padded on the device like DIN's.  L 1..32 is part of the model
 * (l1.W is sized by it) and is kept on the handle; a wrong n_elems, L or E is DM_ERR_INVALID.  The handle records which scorer is
 * loaded (dm_get_scorer_kind: *seq_len is DeepFM's L, 0 for DIN); loading DIN weights afterwards switches it back.  dm_clone clones
 * serve the same model through the shared storage.
 * With a DeepFM model loaded: dm_deepfm_forward, dm_deepfm_pairs_forward and dm_tdm_beam_search / _trace / _dev serve it, and
 * dm_deepfm_jtm_* learn the tree with it (the searches through the per-level
 * pipeline for every L, use_mask must be 0 — the graph has no mask, T/model/TDM.scala:26-29 — and L must be the model's: DM_ERR_INVALID
 * otherwise); dm_get_leaf_embeddings, dm_cluster_tree_model, dm_save_model / dm_load_model work as for DIN; every entry point that
 * evaluates DIN (dm_din_forward, dm_otm_*, dm_tdm_bruteforce_topk, dm_jtm_*, dm_train_*, dm_adam_step, dm_tdm_make_train_batch,
 * dm_tdm_sample_train_batch_dev, dm_set_scorer_mode) returns DM_ERR_UNSUPPORTED and leaves the handle usable (training and its
 * sampler have DeepFM entry points of their own, below, and so has JTM's scoring: dm_deepfm_jtm_*; OTM's beam search and training
 * iteration: dm_deepfm_otm_*, below; OTMConstructTree's child weights: dm_deepfm_otm_child_weights / dm_deepfm_otm_tree_*, below). */
enum { DM_KIND_DIN = 0, DM_KIND_DEEPFM = 1 };
int dm_load_weights_deepfm(dm_handle_t h, int dtype, int E, int L, int64_t num_index, const void *compact, int64_t n_elems);
int dm_get_scorer_kind(dm_handle_t h, int *kind, int *seq_len);
/* Module.forward(Table(item, seq)) of the DeepFM graph for rows that each carry their own history (call sites: T/model/Recommender.scala:
 * 93-94 with SeqModelInputs, TDM.predict): codes [B], seqs [B*L] node codes, -1 = a zero row; an index outside [0, num_index) is
 * DM_ERR_INDEX as in dm_din_forward; L must equal the model's seq_len; logits [B] float.  DM_ERR_STATE on a DIN model. */
int dm_deepfm_forward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, int64_t B, int L, float *logits);
/* The same logits for P (node, history) pairs whose histories are shared: pair i is scored against history i / seq_div of
 * seqs [ceil(P / seq_div)][L] (seq_div >= 1; 1: one history per pair).  This is the scorer of dm_deepfm_jtm_* on host arrays — a
 * per-history set-up kernel, then a per-pair kernel: a pair's logit depends on its (code, history) only, not on
 * P, seq_div or its neighbours, and two runs give the same bytes.  Errors as dm_deepfm_forward. */
int dm_deepfm_pairs_forward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, int64_t P, int L, int seq_div, float *logits);

/* Checkpoint (replaces TDM.saveModel / loadModel, T/utils/Serialization.scala:60-101 — a Java ObjectOutputStream of the module graph
 * there; tdm/src/test/scala/TdmModelTrainSpec.scala:85-96 pins save -> load -> identical recommendations): one flat little-endian
 * file with the compact parameter vector in the loaded dtype plus the tree nodes and the item id -> leaf code map when they are
 * loaded (layout: dismember_amd/csrc/checkpoint.hip.inc; the header names the scorer, DIN or DeepFM).  No optimizer state, like the reference.  dm_load_model replaces whatever
 * tree / id maps / weights the handle holds with the file's. */
int dm_save_model(dm_handle_t h, const char *path);
int dm_load_model(dm_handle_t h, const char *path);

/* Arithmetic of the beam-search scorer (dm_tdm_beam_search*, dm_otm_beam_search*; no reference counterpart: the
 * reference's Linear / MatMul call MKL sgemm, S/tensor/TensorNumeric.scala:265-266).
 *   DM_SCORER_F32        fp32-input MFMA for every product.
 *   DM_SCORER_SPLIT_F16  the three products of a scored row (attention scores q.k, the W1a half and the attention half of
 *                        linear1) take each fp32 operand as hi + lo fp16 halves (22 significand bits, scaled by a power of
 *                        two into the fp16 range) and run hi*hi + hi*lo + lo*hi on the fp16 matrix pipe with fp32
 *                        accumulation: per-product relative error <= 3 * 2^-22, below the fp32 summation-order noise that
 *                        separates any two fp32 implementations over E terms (measured: DESIGN.md).  E must be 32, 64 or
 *                        128.  Same stated tolerance as the F32 mode (rtol 1e-4 / atol 1e-5 against the oracle); ids are
 *                        the exact beam search on the scores produced.
 *   DM_SCORER_AUTO       (default) SPLIT_F16 where the embedding size allows it, F32 otherwise (E = 16); and for the OTM
 *                        searches (dm_otm_beam_search*) of a model loaded as DM_F64: DM_SCORER_F64.
 *   DM_SCORER_F64        OTM searches in the reference's own arithmetic (otm/.../model/DIN.scala:12-39 is DIN[Double]):
 *                        every product on the fp64 matrix cores, node ids bit-exact against the fp64 oracle given the
 *                        same scores, scores within 1e-10 / 1e-9.  Needs f64 weights.  This is the parity mode; F32 /
 *                        SPLIT_F16 (on the f32 copy of the table) remain the throughput modes and can be forced.
 * The brute-force recall oracle (dm_tdm_bruteforce_topk) and every other entry point always use fp32 / fp64 arithmetic.
 * dm_get_scorer_mode: the setting, the arithmetic in effect for the loaded model, and the power-of-two shifts in use
 * (after the first search). */
enum { DM_SCORER_F32 = 0, DM_SCORER_SPLIT_F16 = 1, DM_SCORER_AUTO = 2, DM_SCORER_F64 = 3 };
int dm_set_scorer_mode(dm_handle_t h, int mode);
int dm_get_scorer_mode(dm_handle_t h, int *mode, int *effective, int *shift_emb, int *shift_w);

/* ---- operator level: Module.forward(Table(items, seqs, masks)) ---------- */

/* call sites: T/model/Recommender.scala:93-94, O/model/CandidateSearcher.scala:40-50,
 * O/tree/OTMTree.scala:167-172, jtm/.../optim/TreeLearning.scala:166-168.
 * codes [B], seqs [B*L] (node codes, -1 = padding), pad_flat_idx [n_pad] = flat
 * positions i*L+j to mask (S/nn/Mask.scala:27-32).  logits: B values of the
 * loaded dtype (float or double). */
int dm_din_forward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, const int32_t *pad_flat_idx,
                   int64_t n_pad, int64_t B, int L, void *logits);

/* ---- TDM beam search: Recommender._recommend + TDM.recommend -------------- */

typedef struct {
  int beam;           /* candidateNum */
  int topk;
  int use_mask;       /* 1 for DIN (TDM.apply, T/model/TDM.scala:26-29) */
  int widen_consumed; /* 1 = recommendItems semantics: beam_u = max((consumed_u+topk)/2, beam)  (:28-33) */
} dm_tdm_search_opts;

/* seq_item_ids [U*L] raw item ids (0 = padding).  consumed_off [U+1] / consumed_ids: CSR of
 * already-consumed item ids per user, or NULL/NULL.  Outputs: out_item_ids/out_scores [U*topk]
 * (scores are LOGITS; the facade applies sigmoid in double like T/model/TDM.scala:56-58),
 * out_counts [U] (<= topk).
 * L = seq_len, 1 .. 32 (the reference's Attention takes any length, S/nn/Attention.scala:34-53; its configs use 10): up to 16 positions run on
 * the one-wave kernel, 17 .. 32 on the fused LDS-fed kernel's two-key-tile instance (f32 models; fp64 OTM searches on the fp64 kernel's);
 * L > 32 is DM_ERR_INVALID, never a truncated history. */
int dm_tdm_beam_search(dm_handle_t h, const int32_t *seq_item_ids, int64_t U, int L, const dm_tdm_search_opts *opts,
                       const int64_t *consumed_off, const int32_t *consumed_ids, int32_t *out_item_ids,
                       float *out_scores, int32_t *out_counts);

/* Same search, additionally dumping every scored level (parity instrumentation):
 * trace_codes/trace_scores [U * max_levels * cap], trace_counts [U * max_levels];
 * cap = 2*beam rounded up to 16; slots past a user's last level have count 0. */
int dm_tdm_beam_search_trace(dm_handle_t h, const int32_t *seq_item_ids, int64_t U, int L,
                             const dm_tdm_search_opts *opts, int32_t *out_item_ids, float *out_scores,
                             int32_t *out_counts, int max_levels, int32_t *trace_codes, float *trace_scores,
                             int32_t *trace_counts);

/* ---- OTM beam search: CandidateSearcher.beamSearch (O/model/CandidateSearcher.scala:58-80) ----
 * seq_codes [U*L] are node ids (OTM.recommend has already mapped items, O/model/OTM.scala:15);
 * complete tree, no existence filter.  out_node_ids/out_scores [U * 2*beam] = the leaf-level
 * candidates in order (f32 scorer; the reference runs this path in f64 — tolerance in DESIGN.md). */
int dm_otm_beam_search(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                       int32_t *out_node_ids, float *out_scores, int32_t *out_counts);

/* The same two searches with double outputs, always in fp64 arithmetic (f64 weights required): the scores the reference's
 * DIN[Double] produces, for the 1e-10 / 1e-9 parity contract. */
int dm_otm_beam_search_f64(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                           int32_t *out_node_ids, double *out_scores, int32_t *out_counts);
int dm_otm_beam_search_trace_f64(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                                 int32_t *out_node_ids, double *out_scores, int32_t *out_counts, int max_levels,
                                 int32_t *trace_codes, double *trace_scores, int32_t *trace_counts);

/* Same, dumping every level's scored candidates = OTMTree.beamSearchNodes (O/tree/OTMTree.scala:67-91), which OTM
 * training consumes: trace_* [U * max_levels * cap] / [U * max_levels], cap = 2*beam rounded up to 16 (min 32). */
int dm_otm_beam_search_trace(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                             int32_t *out_node_ids, float *out_scores, int32_t *out_counts, int max_levels,
                             int32_t *trace_codes, float *trace_scores, int32_t *trace_counts);

/* ---- brute force over every leaf (build-defined recall@k oracle) ---- */
int dm_tdm_bruteforce_topk(dm_handle_t h, const int32_t *seq_item_ids, int64_t U, int L, int topk, int use_mask,
                           int32_t *out_item_ids, float *out_scores, int32_t *out_counts);

/* ---- JTM / OTM tree learning (jtm/src/main/scala/com/mass/jtm/optim/TreeLearning.scala) ---------------
 * One gap step of JTM.optimize (jtm/.../optim/JTM.scala:29-70) for n_items items:
 *   row_off [n_items+1] / row_item_ids [rows*L]: the item's training rows = itemSequenceMap (:34-46), raw item
 *   ids, L per row; item_node [n_items]: node code (at old_level) each item currently sits in.
 * weights [n_items * 2^(level-old_level)] = aggregateWeights (:152-174) per child, children ordered as
 * JTMTree.getChildrenAtLevel (jtm/.../tree/JTMTree.scala:53-57); items without rows get -1e6 (:160).
 * The DIN forwards run on the GPU; Tensor.sum and the chain accumulation keep the reference's fp32 order. */
int dm_jtm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, const int32_t *item_node,
                         int64_t n_items, int L, int old_level, int level, int hierarchical, int min_level, int use_mask,
                         float *weights);
/* The same with the catalogue's training rows (itemSequenceMap, built once per run: TreeLearning.scala:34-46) kept on the device
 * across the gap steps of one JTM.optimize: dm_jtm_cache_rows uploads row_off [n_items+1] (row_off[0] == 0) / row_item_ids once
 * (n_items == 0 drops the copy); dm_jtm_child_weights_cached scores the items [i_lo, i_lo + n_items) of that catalogue
 * (item_node and weights are indexed from i_lo: a rank's item shard) and uploads nothing but item_node. */
int dm_jtm_cache_rows(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, int64_t n_items, int L);
/* Sharded runs (one handle per rank, dm_jtm_optimize_cached with a communicator attached / dm_jtm_optimize_all): a rank only ever scores
 * the items [i_lo, i_hi) that dm_jtm_shard_range(n_items, rank, nranks, ...) gives it (the reference's contiguous split of the items
 * over its workers, JTM.scala:47-52).  dm_jtm_cache_rows_range takes the SAME full arrays and keeps row_off for all items, but uploads
 * only that range's training rows — the upload, the row arrays and the per-row history codes then scale with 1 / nranks.  Scoring items
 * outside the range on such a handle is DM_ERR_STATE. */
int dm_jtm_shard_range(int64_t n_items, int rank, int nranks, int64_t *i_lo, int64_t *i_hi);
int dm_jtm_cache_rows_range(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, int64_t n_items, int L, int64_t i_lo, int64_t i_hi);
int dm_jtm_child_weights_cached(dm_handle_t h, const int32_t *item_node, int64_t i_lo, int64_t n_items, int old_level, int level,
                                int hierarchical, int min_level, int use_mask, float *weights);
/* One whole gap step of JTM.optimize (JTM.scala:36-72) over the cached catalogue on the device: the child weights of every item
 * (as dm_jtm_child_weights_cached) and the greedy re-balance of every parent node of old_level (as dm_jtm_rebalance_all) with the
 * [n_items x 2^gap] weight matrix kept in HBM.  item_node [n_items] = current node of every item, old_node [n_items] =
 * tree.getAncestorAtLevel(item, level); out_node [n_items] = the item's node at `level` after the step.  n_items must be the
 * cached catalogue's size (single-rank runs; sharded runs keep the two separate calls around their all-gather). */
int dm_jtm_step_cached(dm_handle_t h, const int32_t *item_node, const int32_t *old_node, int64_t n_items, int old_level, int level,
                       int hierarchical, int min_level, int use_mask, int max_assign, int32_t *out_node);
/* JTM.optimize (JTM.scala:22-73) over the cached catalogue in ONE call: every item starts at the root; each gap step scores the children
 * chains and re-balances every parent node on the device, and its result feeds the next step without leaving HBM.  item_code [n_items] =
 * the items' current leaf codes (tree.getAncestorAtLevel is taken from them per step); out_proj [n_items] = every item's new leaf code;
 * step_seconds (may be NULL) [2] = seconds spent scoring / re-balancing.
 * With a communicator attached (dm_comm_attach, > 1 rank) the call is COLLECTIVE and the run is sharded the way the reference's workers
 * split it (JTM.scala:33-68, JTMAsync.scala:43-75): every rank holds the cached catalogue and scores the rows of ITS contiguous item range
 * (sizes as taskSize / extraSize, :47-52); the [items x 2^gap] weight slices are all-gathered in place, device to device (RCCL over xGMI;
 * host staging on DM_COMM_HOST); the greedy re-balance runs replicated while a level has fewer parent nodes than ranks and afterwards
 * over each rank's contiguous range of parent nodes, followed by an all-gather of (item, new node) pairs.  Each weight is one GPU's
 * sequential fp32 sum and each parent's list keeps item order, so out_proj is bit-identical to the single-rank result on every rank. */
int dm_jtm_optimize_cached(dm_handle_t h, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical, int min_level,
                           int use_mask, int32_t *out_proj, double *step_seconds);
/* the same from ONE process driving all ranks of a dm_comm_create_all clique (the reference's shape: one JVM, numThreads workers):
 * hs[i] carries rank i and its own cached catalogue; ranks run on host threads of this call.  The ranks' projections are compared
 * (DM_ERR_STATE if they differ) and out_proj receives the common one.  n == 1 is dm_jtm_optimize_cached. */
int dm_jtm_optimize_all(dm_handle_t *hs, int n, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical,
                        int min_level, int use_mask, int32_t *out_proj, double *step_seconds);
/* JTM tree learning with a DeepFM model (TreeLearning.aggregateWeights runs dlModel.forward on whatever graph the model file holds,
 * TreeLearning.scala:152-174): the twins of dm_jtm_child_weights, dm_jtm_child_weights_cached, dm_jtm_step_cached and
 * dm_jtm_optimize_cached, with the same arguments and results; the pairs are scored as dm_deepfm_pairs_forward scores them.
 * dm_jtm_cache_rows[_range], dm_jtm_rebalance*, dm_jtm_optimize_stats and dm_jtm_last_step_seconds hold no scorer and serve both.
 * DM_ERR_STATE on a DIN model; DM_ERR_INVALID for use_mask != 0 (the DeepFM graph has no mask input) and for an L (the call's, or the
 * cached catalogue's) that is not the model's; DM_ERR_INDEX for a history code outside the table; DM_ERR_UNSUPPORTED while a
 * communicator of more than one rank is attached (nothing of DeepFM runs multi-GPU).  The handle stays usable after every refusal. */
int dm_deepfm_jtm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, const int32_t *item_node,
                                int64_t n_items, int L, int old_level, int level, int hierarchical, int min_level, int use_mask,
                                float *weights);
int dm_deepfm_jtm_child_weights_cached(dm_handle_t h, const int32_t *item_node, int64_t i_lo, int64_t n_items, int old_level, int level,
                                       int hierarchical, int min_level, int use_mask, float *weights);
int dm_deepfm_jtm_step_cached(dm_handle_t h, const int32_t *item_node, const int32_t *old_node, int64_t n_items, int old_level, int level,
                              int hierarchical, int min_level, int use_mask, int max_assign, int32_t *out_node);
int dm_deepfm_jtm_optimize_cached(dm_handle_t h, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical,
                                  int min_level, int use_mask, int32_t *out_proj, double *step_seconds);
/* measurement — what the last dm_jtm_optimize_cached on this handle did: out10[0..9] = ranks, transport (DM_COMM_*; 2^64-1 = no
 * communicator), items this rank scored summed over the gap steps, items it re-balanced in node-sharded steps, steps with a replicated
 * re-balance, node-sharded steps, weight bytes all-gathered, projection bytes all-gathered, 0, 0; secs3 = scoring, re-balance,
 * exchange seconds. */
int dm_jtm_optimize_stats(dm_handle_t h, uint64_t *out10, double *secs3);
/* measurement: seconds the last dm_jtm_step_cached spent in its scoring pass and in its re-balance (copies included) */
int dm_jtm_last_step_seconds(dm_handle_t h, double *scoring_s, double *rebalance_s);
/* getChildrenProjection after scoring (:58-97) for the items of ONE parent `node`: sortNodeWeights (stable
 * descending), first choice, greedy capacity-bounded reBalance (:217-265).  old_node [n] =
 * tree.getAncestorAtLevel(item, level); out_node [n] = assigned child code (-1: dropped by the greedy loop).
 * Host-side exact integer logic (parents are independent; callers may run it from several threads on
 * different handles). */
int dm_jtm_rebalance(dm_handle_t h, const float *weights, const int32_t *old_node, int64_t n, int32_t node, int old_level,
                     int level, int max_assign, int32_t *out_node);

/* The same for EVERY parent node of a level in one call (the loop over currentNodes of JTM.optimize, J/optim/JTM.scala:36-70;
 * TreeConstruction.run, O/tree/TreeConstruction.scala:44-101): items are grouped by item_node [n] (the node each item sits in at
 * old_level) in the order given; out_node [n] = the new child code, or the old node for items the greedy loop drops. */
int dm_jtm_rebalance_all(dm_handle_t h, const float *weights, const int32_t *old_node, const int32_t *item_node, int64_t n,
                         int old_level, int level, int max_assign, int32_t *out_node);
int dm_otm_rebalance_all(dm_handle_t h, const double *weights, const int32_t *old_node, const int32_t *item_node, int64_t n,
                         int old_level, int level, int max_assign, int32_t *out_node);

/* OTM twin (otm/src/main/scala/com/mass/otm/tree/TreeConstruction.scala): the item sequences hold NODE ids (-1 =
 * paddingIdx, :218-232), the scorer runs in the loaded dtype (fp64 in the reference) and sums are double:
 * dm_otm_child_weights = aggregateWeights (:194-212) per child of getChildrenAtLevel (:281-285);
 * dm_otm_rebalance     = sortNodeWeights (:180-192) + first choice + reBalance (:304-352), same logic as the JTM one. */
int dm_otm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_codes, const int32_t *item_node,
                         int64_t n_items, int L, int old_level, int level, int use_mask, double *weights);
int dm_otm_rebalance(dm_handle_t h, const double *weights, const int32_t *old_node, int64_t n, int32_t node, int old_level,
                     int level, int max_assign, int32_t *out_node);
/* The same child weights with a DeepFM model (TreeConstruction.scala:215-230 builds Table(nodes, seq) when useMask = false): fp32 model,
 * double sums.  dm_deepfm_otm_child_weights has dm_otm_child_weights' signature (use_mask must be 0, L the model's, one rank); the
 * histories go up once per call and are never expanded into pairs: the per-history part of the score is computed once, the per-node
 * part once per (item, 16 chain nodes).  A (row, chain node) logit is dm_deepfm_pairs_forward's byte for byte; an item's rows are
 * summed in segments of 256 (DM_DFM_OTM_TREE_SEG), the segment sums left to right: with at most 256 rows this is strict row order.
 * An item's weights depend on its own rows and node only.
 * The prepared form, on the owning handle: dm_deepfm_otm_tree_prepare uploads the histories of a catalogue and keeps their per-history
 * part on the device (a second prepare replaces the first); dm_deepfm_otm_tree_weights runs one gap step on it and returns the same
 * bytes as the one-shot call — DM_ERR_STATE if nothing is prepared, if n_items differs or if the model changed since the prepare (a
 * load, an Adam step); dm_deepfm_otm_tree_release drops it (a weight release and dm_destroy do too).
 * DM_ERR_STATE on a DIN model; DM_ERR_INVALID for null arguments, n_items < 0, level <= old_level, level - old_level > 8, an item_node
 * that is not a node of old_level, use_mask != 0, an L that is not the model's; DM_ERR_INDEX when 2^(level + 1) - 1 > num_index or a
 * history code lies outside [-1, num_index); DM_ERR_UNSUPPORTED with a communicator of more than one rank.  Every refusal comes before
 * anything is allocated and leaves the handle usable. */
int dm_deepfm_otm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_codes, const int32_t *item_node,
                                int64_t n_items, int L, int old_level, int level, int use_mask, double *weights);
int dm_deepfm_otm_tree_prepare(dm_handle_t h, const int64_t *row_off, const int32_t *row_codes, int64_t n_items, int L);
int dm_deepfm_otm_tree_weights(dm_handle_t h, const int32_t *item_node, int64_t n_items, int old_level, int level, double *weights);
int dm_deepfm_otm_tree_release(dm_handle_t h);

/* ---- training step (tdm/src/main/scala/com/mass/tdm/optim/LocalOptimizer.scala:58-187) ------------------
 * One handle == one worker (the reference's per-thread model clone).  A step is
 *   dm_train_forward_backward  == trainBatch (:139-162): zero-initialised gradients accumulate the mean-BCE
 *                                  gradient of this worker's rows (BCECriterionWithLogits + Module.backward)
 *   [exchange between workers]  == syncGradients (:164-187): sum over workers, then / n_workers
 *   dm_adam_step(1/n_workers)   == Adam.optimize (scalann/.../optim/Adam.scala:19-73), DENSE over the whole
 *                                  compact vector (untouched embedding rows still move through s, r), then
 *                                  the gradient is zeroed (zeroGradParameters).
 * The step runs in the LOADED dtype: f32 models (TDM / JTM, T/model/DIN.scala) train in fp32, f64 models (the reference's OTM,
 * DIN[Double]: O/model/DIN.scala:12-39, O/optim/LocalOptimizer.scala:55-140,217-233) in fp64 on v_mfma_f64_16x16x4_f64 with an
 * fp64 gradient and fp64 Adam state.  Labels are float in both (0 / 1, or pseudo targets clipped to [0, 1]); `loss` is the
 * value rounded to float, dm_train_last_loss returns it in the model's precision.  Vectors that cross the boundary
 * (dm_train_download, dm_train_dense_block, dm_train_export_rows, dm_train_add_rows) hold elements of the loaded dtype. */
typedef struct { double lr, lr_decay, beta1, beta2, eps; } dm_adam_opts;   /* reference defaults: 1e-3, 0, 0.9, 0.999, 1e-8 */
int dm_train_init(dm_handle_t h, const dm_adam_opts *opts);
int dm_train_forward_backward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, const int32_t *pad_flat_idx,
                              int64_t n_pad, const float *labels, int64_t B, int L, float *loss);
int dm_adam_step(dm_handle_t h, float grad_scale);
/* The step visits the embedding rows a gradient has ever reached since dm_train_init plus the small matrices: for every other row
 * g = s = r = 0 and the reference's dense update leaves the weight bit-identical (0 / (sqrt(0) + eps) = 0, w + (-0) = w), so the result IS
 * the dense Adam's, without streaming a table that cannot change (dense stream again once a quarter of the rows are active, when eps == 0,
 * or with DM_ADAM_DENSE=1 in the environment).  Measurement: rows visited by the last step, and whether it took the active-rows path. */
int dm_adam_last_step_rows(dm_handle_t h, uint64_t *rows, int *active_rows_only);
int dm_train_last_loss(dm_handle_t h, double *loss);
/* what: 0 weights, 1 gradient, 2 Adam s, 3 Adam r — host copy of the full compact-layout vector (tests, checkpoints) */
int dm_train_download(dm_handle_t h, int what, void *out, int64_t n);
/* Gradient exchange for N workers on N GPUs: the dense block [att.W ; l1.W ; l1.b ; l2.W ; l2.b]
 * is all-reduced in place through the returned device pointer (RCCL); embedding gradients are row-sparse:
 * export this worker's unique touched rows (index + gradient row, device buffers), all-gather them, add the
 * other workers' rows.  Replicas stay bit-identical because every rank applies the same sums in the same order. */
int dm_train_dense_block(dm_handle_t h, void **d_ptr, int64_t *n);
int dm_train_export_rows(dm_handle_t h, int32_t *d_rows, void *d_grads, int64_t cap, int64_t *n);   /* NULL buffers: size query */
int dm_train_add_rows(dm_handle_t h, const int32_t *d_rows, const void *d_grads, int64_t n);

/* ---- multi-GPU: communicators and the gradient exchange ------------------------------------------
 * The reference's data parallelism is N worker threads in one JVM whose gradient buffers are averaged in place
 * (LocalOptimizer.syncGradients, T/optim/LocalOptimizer.scala:164-187; O/optim/LocalOptimizer.scala:217-233).  Here a worker
 * is a handle on its own GPU; a dm_comm_t connects the workers:
 *   DM_COMM_RCCL  RCCL over xGMI, one rank per GPU.  Either one process per GPU (dm_comm_create_rccl with an id from
 *                 dm_comm_unique_id that the host distributes itself, or dm_comm_create_tcp which distributes it), or ONE
 *                 process driving every GPU like the reference's JVM (dm_comm_create_all + dm_allreduce_grads).
 *   DM_COMM_HOST  a TCP star through rank 0, device buffers staged through host memory: several workers sharing one GPU
 *                 (RCCL refuses two ranks per device) and CPU-only processes for the host-buffer collectives.
 * dm_train_sync_gradients(h) == syncGradients minus the division (dm_adam_step(1/N) folds it in): all-reduce(sum) of the
 * dense block + all-gather of (touched row, gradient row) lists, each touched row rebuilt as 0 + g_0 + g_1 + ... in rank
 * order, so every replica ends with bit-identical gradients (the RCCL dense sum is identical on all ranks but in RCCL's
 * reduction order, not rank order; the HOST transport sums in rank order).  RCCL transport: one ncclAllGather of 16-byte
 * {count, ok} records + ONE host read-back, then one ncclAllReduce and one ncclAllGather of max-padded row blocks.
 * Collective: every rank must call it; a rank whose touched-row list overflowed makes EVERY rank return DM_ERR_STATE.
 * dm_train_sync_stats: what the last exchange on this handle moved — out[0..7] = nranks, transport, touched rows of this
 * rank, touched rows of all ranks, bytes sent, bytes received, host synchronisations, 0. */
typedef struct dm_comm *dm_comm_t;
enum { DM_COMM_HOST = 0, DM_COMM_RCCL = 1 };
#define DM_COMM_ID_BYTES 128
int dm_comm_unique_id(void *id128);                                  /* ncclGetUniqueId, padded to DM_COMM_ID_BYTES */
int dm_comm_create_rccl(int nranks, int rank, const void *id128, int device_id, dm_comm_t *out);
/* rendezvous at addr:port (rank 0 listens); transport DM_COMM_RCCL: the sockets only carry the id.  device_id is ignored
 * by DM_COMM_HOST (no GPU needed for the host-buffer collectives). */
int dm_comm_create_tcp(int nranks, int rank, const char *addr, int port, int transport, int device_id, dm_comm_t *out);
int dm_comm_create_all(int n, const int *devices, dm_comm_t *out /* [n] */);   /* ncclCommInitAll: one process, n GPUs */
int dm_comm_destroy(dm_comm_t c);
const char *dm_comm_last_error(dm_comm_t c);                          /* c may be NULL: last create-time error */
int dm_comm_rank(dm_comm_t c, int *rank, int *nranks, int *transport);
int dm_comm_barrier(dm_comm_t c);
int dm_comm_allreduce_f64(dm_comm_t c, double *vals, int n, int op /* 0 sum (rank order), 1 max */);   /* host values, in place */
/* var-size all-gather of host buffers: recv gets the blocks in rank order, sizes[nranks] their byte lengths; recv == NULL
 * only fills sizes */
int dm_comm_all_gather_v(dm_comm_t c, const void *send, size_t bytes, void *recv, size_t recv_cap, uint64_t *sizes);
int dm_comm_attach(dm_handle_t h, dm_comm_t c);                       /* the handle does not own c; NULL detaches */
int dm_comm_all_gather_dev(dm_handle_t h, const void *d_send, size_t bytes, void *d_recv, size_t recv_cap, uint64_t *sizes);
int dm_train_sync_gradients(dm_handle_t h);
int dm_train_sync_stats(dm_handle_t h, uint64_t *out8);
/* SURVEY.md §8b `dm_allreduce_grads(h[], n_gpu)`: the same exchange for ALL ranks of a dm_comm_create_all clique from one
 * thread (hs[i] must carry rank i); n == 1 is dm_train_sync_gradients. */
int dm_allreduce_grads(dm_handle_t *hs, int n);

/* ---- OTM training iteration (otm/src/main/scala/com/mass/otm/optim/LocalOptimizer.scala:55-109) ---------------------------
 * One LocalOptimizer iteration for this worker's batch of U users, every list on the device:
 *   targets   OTMTree.optimalPseudoTargets (O/tree/OTMTree.scala:27-46; computeTargets :104-129 with its mirrored prediction offsets,
 *             computeChildrenScores :131-165) — target_mode 0 — or OTMTree.normalTargets (:50-63) — target_mode 1;
 *   beams     OTMTree.beamSearchNodes (:67-91), weights fixed (the per-level trace of the OTM beam search);
 *   per level MiniBatch.batchTransform (O/dataset/MiniBatch.scala:17-40) -> trainBatch (LocalOptimizer.scala:111-131) ->
 *             syncGradients (:133-141: dm_train_sync_gradients when a communicator with > 1 rank is attached — the call is then
 *             COLLECTIVE) -> Adam.optimize with 1 / ranks.
 * seq_codes [U*L] node ids (-1 = padding); target_off [U+1] / target_nodes: CSR of every user's target LEAF nodes (OTMSample.targetItems
 * after the item -> node mapping); level_losses [leaf_level - floor(log2 beam)] receives the per-level losses averaged over the ranks
 * (levelLoss of :73-80, first level first), *n_levels their number.  Needs dm_train_init; runs in the loaded dtype (the reference's
 * OTM is DIN[Double]: fp64 search, fp64 training); the Adam step of every level moves the weights, like the reference. */
typedef struct {
  int beam;          /* beamSize */
  int leaf_level;    /* leaf level of the complete tree; the start level is floor(log2 beam) */
  int use_mask;      /* 1 for DIN */
  int target_mode;   /* 0 "pseudo" (optimalPseudoTargets), 1 "normal" (normalTargets) */
} dm_otm_train_opts;
int dm_otm_train_batch(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                       const dm_otm_train_opts *opts, double *level_losses, int *n_levels);
/* the target lists alone (parity instrumentation; no training state needed): out_nodes / out_labels [levels x target_off[U]] in the CSR of
 * target_off (a user's list at a level occupies the first out_counts[level][u] of its slots; unused slots hold -1 / 0), out_counts
 * [levels x U]; level index li <-> tree level floor(log2 beam) + 1 + li. */
int dm_otm_pseudo_targets(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                          const dm_otm_train_opts *opts, int32_t *out_nodes, double *out_labels, int32_t *out_counts);
/* measurement — the last dm_otm_train_batch on this handle: out6 = users, levels, rows of the pseudo-target forwards, rows trained, 0, 0;
 * secs5 = pseudo targets, beam search, forward / backward, gradient exchange, Adam (seconds) */
int dm_otm_train_stats(dm_handle_t h, uint64_t *out6, double *secs5);

/* ---- OTM with the DeepFM scorer (examples/.../otm/OTMTrainDeepModel.scala:41-47 builds O/model/DeepFM.scala:10-49; fp32 like the loader,
 * where the reference runs DeepFM[Double]; the contract is the one dm_otm_beam_search states for f32 models).  The dm_otm_* entry points keep
 * refusing a DeepFM handle (DM_ERR_UNSUPPORTED); these are their twins.
 * All of them: DM_ERR_STATE on a DIN model; L must be the model's seq_len (DM_ERR_INVALID); beam <= 512 (DM_ERR_UNSUPPORTED above: the
 * prune sorts in LDS); there is no mask (O/model/OTM.scala:14-22,32,58: useMask = false) — opts->use_mask must be 0 (DM_ERR_INVALID).
 *
 * dm_deepfm_otm_beam_search         OTM.recommend's search: CandidateSearcher.beamSearch (O/model/CandidateSearcher.scala:58-80, buildBeamNodes
 *                                   :109-122) as ONE kernel, one workgroup per user; arguments, outputs and DM_ERR_INDEX as dm_otm_beam_search
 * dm_deepfm_otm_beam_search_trace   + every level's candidates (OTMTree.beamSearchNodes, O/tree/OTMTree.scala:67-91,174-212); layouts of
 *                                   dm_otm_beam_search_trace (cap = 2 beam rounded up to 16, at least 32)
 * dm_deepfm_otm_beam_search_dev     device-resident request, as dm_otm_beam_search_dev (codes outside the table count as padding)
 * Two runs, any batch mates and any grid give the same bytes; dm_clone clones serve them. */
int dm_deepfm_otm_beam_search(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                              int32_t *out_node_ids, float *out_scores, int32_t *out_counts);
int dm_deepfm_otm_beam_search_trace(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                                    int32_t *out_node_ids, float *out_scores, int32_t *out_counts, int max_levels,
                                    int32_t *trace_codes, float *trace_scores, int32_t *trace_counts);
int dm_deepfm_otm_beam_search_dev(dm_handle_t h, const int32_t *d_seq_codes, int64_t U, int L, int beam, int leaf_level,
                                  int32_t *d_out_node_ids, float *d_out_scores, int32_t *d_out_counts);
/* OTMTree.optimalPseudoTargets (O/tree/OTMTree.scala:27-46) / normalTargets (:50-63), arguments and outputs of dm_otm_pseudo_targets.
 * Without a mask computeChildrenScores feeds the sibling tensor to both forwards (:156-161), so posPreds(i) >= negPreds(i) compares a
 * value with itself and every node keeps its own label: no forward is run, and target_mode 0 gives, per level, the targets' ancestors in
 * first-appearance order with clip(sum of child labels, 0, 1).  (The reference differs only where a logit is NaN.) */
int dm_deepfm_otm_pseudo_targets(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                                 const dm_otm_train_opts *opts, int32_t *out_nodes, double *out_labels, int32_t *out_counts);
/* LocalOptimizer.optimize's body for one batch (O/optim/LocalOptimizer.scala:55-109), arguments of dm_otm_train_batch: the targets as
 * above, the beam nodes from ONE fused traced search with the weights fixed, then per level MiniBatch.batchTransform -> the DeepFM row
 * step (dm_deepfm_train_forward_backward_dev) -> dm_deepfm_adam_step with grad_scale 1.  Needs dm_deepfm_train_init (DM_ERR_STATE);
 * owner only; a communicator with more than one rank is DM_ERR_UNSUPPORTED (the gradient exchange for DeepFM is not built), and so is a
 * batch whose U * 2 beam rows exceed the row step's limits (4 194 240 rows, rows (L + 1) < 2^31).  dm_otm_train_stats reads the same
 * block (rows of the pseudo-target forwards: 0). */
int dm_deepfm_otm_train_batch(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                              const dm_otm_train_opts *opts, double *level_losses, int *n_levels);

/* Level-wise negative sampling + batch expansion, ON THE DEVICE: NegativeSampler.sample
 * (tdm/.../utils/NegativeSampler.scala:76-158: uniform and sample_with_probability modes) + MiniBatch.convert
 * (tdm/.../dataset/MiniBatch.scala:49-88).  One wave per (target, level); counter-based stream splitmix64(seed, target,
 * level, draw) — the reference's RNG is unseeded, so parity with it is distributional; the CPU oracle reproduces this
 * stream bit for bit.
 * seq_item_ids [T*L], target_item_ids [T]; neg_counts = model.layer_negative_counts (>= max_level+1 entries).
 * Rows per target = sum_{l=start_level}^{level of the target} (1 + neg_counts[l]) (targets outside the tree: none);
 * out_codes == NULL returns the upper bound T * sum_{l=start_level}^{max_level} (1 + neg_counts[l]) in *n_rows.
 * out_rowmask bit j = history position j masked; seq_len <= 32. */
typedef struct {
  int start_level;     /* model.start_sample_level (>= 1) */
  int with_prob;       /* model.sample_with_probability: draw from the level's node probabilities (dm_tdm_set_node_probs) */
  int tolerance;       /* model.sample_tolerance: categorical draws per level = neg + tolerance, then a uniform fill */
  int use_mask;        /* 1 for DIN */
  uint64_t seed;
} dm_sample_opts;
/* Node.probality of the tree nodes (T/tree/DistTree.scala:60-75; levelProbs, NegativeSampler.scala:59-66) */
int dm_tdm_set_node_probs(dm_handle_t h, const int32_t *codes, const float *probs, int64_t n);
/* host buffers in and out (the sampling itself runs on the device) */
int dm_tdm_make_train_batch(dm_handle_t h, const int32_t *seq_item_ids, const int32_t *target_item_ids, int64_t T, int L,
                            const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *out_codes,
                            int32_t *out_seqs, uint32_t *out_rowmask, float *out_labels, int64_t cap, int64_t *n_rows);
/* device buffers in and out: the rows land where dm_train_forward_backward_dev reads them; neg_counts is a host array */
int dm_tdm_sample_train_batch_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                  const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                  int32_t *d_seqs, uint32_t *d_rowmask, float *d_labels, int64_t cap, int64_t *n_rows);
/* dm_train_forward_backward on rows that already live in device memory (the output of dm_tdm_sample_train_batch_dev or of
 * a caller's own sampler).  Asynchronous unless `loss` is non-NULL.  The ids are NOT range-checked (the host-buffer entry
 * point validates them like LookupTable.scala:29-53): every code / history entry must be -1 or in [0, num_index). */
int dm_train_forward_backward_dev(dm_handle_t h, const int32_t *d_codes, const int32_t *d_seqs, const uint32_t *d_rowmask,
                                  const float *d_labels, int64_t B, int L, float *loss);
/* The same step for a batch in which every user contributes `rows_per_user` candidate rows that share the user's history — what
 * MiniBatch.batchTransform (otm/.../dataset/MiniBatch.scala:17-40) and MiniBatch.transformWithMask (tdm/.../dataset/MiniBatch.scala:
 * 129-147) build by replicating the history per row: d_seq_codes [U][L] (-1 = padding), d_user_mask [U] (bit j: position j masked;
 * NULL = nothing masked), d_codes / d_labels [U * rows_per_user] user-major (code -1 = a zero item row).  Same loss and gradients as
 * dm_train_forward_backward_dev on the expanded rows (fp64 sums in a different order); an f64 model with L <= 16 takes the per-user
 * kernels (train_grouped_f64.hip.inc), anything else is expanded to plain rows.  Ids are not range-checked. */
int dm_train_forward_backward_grouped_dev(dm_handle_t h, const int32_t *d_seq_codes, const uint32_t *d_user_mask, const int32_t *d_codes,
                                          const float *d_labels, int64_t U, int rows_per_user, int L, float *loss);
/* the DIN step of an f32 model on a ragged user-grouped batch (T/dataset/MiniBatch.scala:129-147 replicates one
 * history over a target's sampled nodes, T/optim/LocalOptimizer.scala:139-162 is the step): rows d_row_off[u] .. d_row_off[u + 1] of
 * d_codes / d_labels [B] belong to user u and read d_seq_codes[u] [L] with the mask word d_umask[u] (bit j = position j masked, as
 * dm_train_forward_backward_dev's rowmask; d_umask may be NULL); a user may have no rows.  ADDS the batch's gradient (mean BCE over the B
 * rows) into the handle's gradient like dm_train_forward_backward_dev, with which it may be mixed before one dm_adam_step; *loss (host, or
 * NULL) and dm_train_last_loss give the loss.  No floating-point atomics: the same batch gives the same bytes, whatever the grid
 * (DM_DIN_TRAIN_GRID=n forces one).  The offsets are validated on the device before anything is read through them or added to the
 * gradient: d_row_off[0] == 0, non-decreasing, d_row_off[U] == B, else DM_ERR_INVALID naming the first offending user.  Device arrays, ids
 * NOT range-checked (an id outside [0, num_index) is read as -1).  U <= 0, B <= 0, a null array other than d_umask, L outside 1 .. 32:
 * DM_ERR_INVALID; L = 17 .. 32 (histories longer than 16 keep the row step), an f64 model (it keeps dm_train_forward_backward_grouped_dev),
 * B > 4 194 240, U > 2 097 120 or B + U L >= 2^31: DM_ERR_UNSUPPORTED; no weights / no dm_train_init: DM_ERR_STATE. */
int dm_train_forward_backward_csr_dev(dm_handle_t h, const int32_t *d_seq_codes, const uint32_t *d_umask, const int64_t *d_row_off, const int32_t *d_codes,
                                      const float *d_labels, int64_t U, int64_t B, int L, float *loss);
/* dm_tdm_sample_train_batch_dev in the form dm_train_forward_backward_csr_dev reads (NegativeSampler.scala:76-158, MiniBatch.scala:129-147):
 * the same d_codes / d_labels bytes and row order from the same seed and options, d_seq_codes [T][L] = every target's history as codes,
 * written once per target (also for a target that yields no rows), d_umask [T] = the rowmask word the row sampler gives the target's rows
 * (0 when opts->use_mask is 0), d_row_off [T + 1] = the first row of every target.  No [cap][L] histories are written.  Size query
 * (d_codes == NULL), checks and refusals: the row twin's. */
int dm_tdm_sample_train_batch_csr_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                      const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                      int32_t *d_seq_codes, uint32_t *d_umask, int64_t *d_row_off, float *d_labels, int64_t cap, int64_t *n_rows);
int dm_memcpy_d2d(dm_handle_t h, void *dst, const void *src, size_t bytes);

/* ---- device-resident variants (bench: inputs already in HBM when the clock starts) ---- */
int dm_dev_alloc(dm_handle_t h, size_t bytes, void **dptr);
int dm_dev_free(dm_handle_t h, void *dptr);
int dm_memcpy_h2d(dm_handle_t h, void *dst, const void *src, size_t bytes);
int dm_memcpy_d2h(dm_handle_t h, void *dst, const void *src, size_t bytes);
/* asynchronous on the handle's stream; all pointers are device pointers; consumed_* may be NULL */
int dm_tdm_beam_search_dev(dm_handle_t h, const int32_t *d_seq_item_ids, int64_t U, int L,
                           const dm_tdm_search_opts *opts, const int64_t *d_consumed_off,
                           const int32_t *d_consumed_ids, int32_t *d_out_item_ids, float *d_out_scores,
                           int32_t *d_out_counts);
/* OTM.recommend's search (dm_otm_beam_search) on a device-resident request: d_seq_codes [U][L] node ids (-1 = padding; codes
 * outside the table count as padding), outputs [U][2*beam] leaf-level node ids (-1 filled) and scores, [U] counts. */
int dm_otm_beam_search_dev(dm_handle_t h, const int32_t *d_seq_codes, int64_t U, int L, int beam, int leaf_level,
                           int32_t *d_out_node_ids, float *d_out_scores, int32_t *d_out_counts);

/* ---- Deep-Retrieval serving ----
 * D/ = deep-retrieval/src/main/scala/com/mass/dr/.  Item ids here are the INTERNAL ids of
 * MappingOp.itemIdMapping (D/model/DeepRetrieval.scala:32,45 map in and out; the host facade keeps doing that);
 * -1 is paddingIdx (D/package.scala:19). */
typedef struct dm_dr_model {
  int32_t dtype;        /* DM_F32 | DM_F64: element type of every array below AND the arithmetic type of the path
                         * (the reference computes in fp64: TensorNumeric.NumericDouble, D/model/LayerModel.scala:7) */
  int32_t on_device;    /* 0: host arrays; 1: device arrays (copied device-to-device, the caller keeps ownership) */
  int32_t embed;        /* embedSize, multiple of 16 */
  int32_t seq_len;      /* seqLen */
  int32_t num_node;     /* K = numNode */
  int32_t num_layer;    /* D = numLayer, 2..4 (D/model/LayerModel.scala:12 requires >= 2) */
  int64_t num_item;
  const void *layer_emb;        /* LayerModel.embedParams   [(num_item + K(D-1)) x E]      D/model/LayerModel.scala:15,24 */
  const void *const *layer_w;   /* [D] LayerModel.linearParams(d).head  [K x (seq_len+d)E] D/model/LayerModel.scala:16-18,31-36 */
  const void *const *layer_b;   /* [D] LayerModel.linearParams(d).last  [K] */
  const void *rerank_emb;       /* RerankModel.embedParams  [num_item x E]                 D/model/RerankModel.scala:13 */
  const void *rerank_w;         /* RerankModel.linearParams.head [E x seq_len*E]           D/model/RerankModel.scala:14,32-34 */
  const void *rerank_b;         /* RerankModel.linearParams.last [E] */
  const void *softmax_w;        /* RerankModel.softmaxWeights [num_item x E]               D/model/RerankModel.scala:15 */
  const void *softmax_b;        /* RerankModel.softmaxBiases  [num_item]                   D/model/RerankModel.scala:16 */
                                /* the five rerank arrays may all be NULL: beam search only */
} dm_dr_model;
/* replaces the state DeepRetrieval.loadModel / LayerModel / RerankModel hold (D/model/DeepRetrieval.scala:90-106);
 * also precomputes the per-(layer, position) node tables, see DESIGN.md.  Float models with E % 64 == 0 additionally keep a second
 * copy of the item / node embedding rows (4 E bytes per row, as the first) split into fp16 hi/lo records for the 256 x 256 history GEMM
 * of batches that fill whole rounds of its tiles (4 096 users, 8 192 and more at config 5's shape); DM_DR_GEMM_X=0 in the environment at load time skips that copy and its kernel. */
int dm_dr_load_model(dm_handle_t h, const dm_dr_model *model);
/* MappingOp.pathItemMapping (D/model/MappingOp.scala:14-28) as a CSR over DISTINCT paths: path_nodes [n_paths x D],
 * items of path i = items[item_off[i] .. item_off[i+1]) in the order searchCandidate should yield them
 * (D/model/CandidateSearcher.scala:14-19).  Any path order; duplicate paths -> DM_ERR_INVALID. */
int dm_dr_load_path_items(dm_handle_t h, const int32_t *path_nodes, int64_t n_paths, const int64_t *item_off,
                          const int32_t *items);
/* CandidateSearcher.beamSearch (D/model/CandidateSearcher.scala:22-60) for U users: seq_ids [U x seq_len] internal ids;
 * out_paths [U x beam x D] nodes in layer order (-1 beyond the count), out_probs [U x beam] path probabilities in
 * descending order (ties: earlier parent path, then lower node — the stable sortBy of :49-51), out_counts [U]. */
int dm_dr_beam_search(dm_handle_t h, const int32_t *seq_ids, int64_t U, int beam, int32_t *out_paths, double *out_probs,
                      int32_t *out_counts);
/* DeepRetrieval.recommend (D/model/DeepRetrieval.scala:26-46) on internal ids: searchCandidate + RerankModel.inference
 * (D/model/RerankModel.scala:43-52) + stable descending sort + take(topk).  out_ids [U x topk] internal item ids
 * (-1 beyond the count; an item reachable through several top paths appears once per path, as in the reference),
 * out_scores [U x topk] rerank LOGITS (the reference applies sigmoid in double afterwards, :45). */
int dm_dr_recommend(dm_handle_t h, const int32_t *seq_ids, int64_t U, int beam, int topk, int32_t *out_ids,
                    double *out_scores, int32_t *out_counts);
/* device-resident variants (asynchronous on the handle's stream; ids are NOT range-checked) */
int dm_dr_beam_search_dev(dm_handle_t h, const int32_t *d_seq_ids, int64_t U, int beam, int32_t *d_out_paths,
                          double *d_out_probs, int32_t *d_out_counts);
int dm_dr_recommend_dev(dm_handle_t h, const int32_t *d_seq_ids, int64_t U, int beam, int topk, int32_t *d_out_ids,
                        double *d_out_scores, int32_t *d_out_counts);

/* ---- Deep-Retrieval M-step: per-item path scores on the device ----
 * CoordinateDescent.batchPathScore + aggregatePathScore + computeItemOccurrence (D/optim/CoordinateDescent.scala:117-163): one beam search with
 * beam = num_candidate_path (C) per sample, and per target item the summed probability of every path its samples' beams hold.
 * seq_ids [N x seq_len] internal ids (-1 = padding), targets [N] in [0, num_item).  The result is a CSR over ALL items: item v's candidates
 * are out_codes / out_scores [out_item_off[v], out_item_off[v + 1]), at most C, descending by score, equal scores in ascending path code
 * (code = sum_d node_d * num_node^(D-1-d)); an item that is never a target has an empty range.  A score is the fp64 sum of the path's
 * probabilities over the item's samples in ASCENDING SAMPLE INDEX, left to right from the first term: the same inputs give the same bytes,
 * whatever the chunk the call searched in.  out_item_off [num_item + 1]; out_occurrence [num_item] (samples per item) may be NULL;
 * *out_total = entries written.  cap = capacity of out_codes / out_scores: when it is too small the call returns DM_ERR_INVALID, writes
 * nothing to the arrays and leaves the needed size in *out_total; min(N, num_item) * C is always enough.
 * trace_paths [N x C x D], trace_probs [N x C], trace_counts [N]: all NULL or all set; they receive every sample's beam as the call
 * aggregated it (dm_dr_beam_search's output).  The samples are searched in chunks (a multiple of 32 768; DM_DR_MSTEP_CHUNK in the
 * environment forces a size) and the node ids of one chunk only are held, unless a trace asks for all.
 * Refused before anything is read or allocated: no Deep-Retrieval model DM_ERR_STATE; C outside [1, 2048], a null required array, N < 0,
 * a partly given trace DM_ERR_INVALID; N * C >= 2^31 (pair indices are 32-bit) and ceil(log2 num_item) + ceil(log2 num_node^D) > 63 (item
 * and path code share a 64-bit sort key) DM_ERR_UNSUPPORTED.  Host entry only: an id outside its range DM_ERR_INDEX.  N == 0: DM_OK, every
 * offset 0.  After dm_dr_adam_step the call searches with re-derived weights, as every search does.  The handle stays usable. */
int dm_dr_mstep_path_scores(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N, int num_candidate_path,
                            int64_t cap, int64_t *out_item_off, int64_t *out_codes, double *out_scores,
                            int64_t *out_occurrence, int64_t *out_total,
                            int32_t *trace_paths, double *trace_probs, int32_t *trace_counts);
/* the same with device arrays (ids are NOT range-checked); out_total stays a host pointer; returns when the results are in place */
int dm_dr_mstep_path_scores_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_targets, int64_t N, int num_candidate_path,
                                int64_t cap, int64_t *d_out_item_off, int64_t *d_out_codes, double *d_out_scores,
                                int64_t *d_out_occurrence, int64_t *out_total,
                                int32_t *d_trace_paths, double *d_trace_probs, int32_t *d_trace_counts);

/* ---- Deep-Retrieval M-step, streaming mode: decayed running path scores folded on the device ----
 * CoordinateDescent.streamingPathScore (D/optim/CoordinateDescent.scala:162-212): one beam search with beam = num_candidate_path (C) per
 * sample; per target item a running list of at most C (path code, score) entries, updated with the item's samples in ASCENDING SAMPLE
 * INDEX.  The first sample's beam is the list as it stands.  Every later sample merges its beam into the list: with m = the smallest score
 * of the list, a path in both scores decay_factor * old + new, a path of the beam only decay_factor * m + new, a path of the list only
 * decay_factor * old; fp64, each product and each sum rounded on its own; the new list is the first C of the union by (score descending,
 * path code ascending).  The reference's mini-batches do not enter the result.  Arguments, the CSR result, cap / out_total, the trace
 * arrays, the chunked search and every refusal are those of dm_dr_mstep_path_scores; in addition decay_factor must be finite and in [0, 1]
 * (DM_ERR_INVALID).  An item with one sample keeps that sample's beam in the beam's order; every other list is descending by score, equal
 * scores in ascending path code.  The same inputs give the same bytes.  The handle stays usable after every refusal. */
int dm_dr_mstep_streaming_path_scores(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N, int num_candidate_path,
                                      double decay_factor, int64_t cap, int64_t *out_item_off, int64_t *out_codes, double *out_scores,
                                      int64_t *out_occurrence, int64_t *out_total,
                                      int32_t *trace_paths, double *trace_probs, int32_t *trace_counts);
/* the same with device arrays (ids are NOT range-checked); out_total stays a host pointer; returns when the results are in place */
int dm_dr_mstep_streaming_path_scores_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_targets, int64_t N,
                                          int num_candidate_path, double decay_factor, int64_t cap, int64_t *d_out_item_off,
                                          int64_t *d_out_codes, double *d_out_scores, int64_t *d_out_occurrence, int64_t *out_total,
                                          int32_t *d_trace_paths, double *d_trace_probs, int32_t *d_trace_counts);

/* ---- Deep-Retrieval M-step: the greedy penalised path assignment on the device ----
 * The coordinate-descent loop of CoordinateDescent.optimize (D/optim/CoordinateDescent.scala:48-82; penaltyFunc :112-115) over the per-item
 * CSR of dm_dr_mstep_path_scores / dm_dr_mstep_streaming_path_scores: item_off [num_item + 1], codes / scores [total], occurrence
 * [num_item].  For t = 1 .. num_iteration, over the items v with occurrence[v] > 0 in ascending id, for j = J - 1 down to 0: (t > 1) the
 * path slot j held gives its place back (size - 1); every candidate c of v not yet chosen in this visit scores
 *   g = nv (log1p(prob_c + partial) - log1p(partial)) - penalty_factor ((s + 1)^p / p - s^p / p),  s = size[code_c], nv = occurrence[v], fp64;
 * the largest g wins, among equal g the lowest CSR position (maxBy :62-70); size[best] + 1; partial += g (the GAIN, :76); out[v][j] = best.
 * An item with occurrence 0 gets J random paths (generateRandomPath, :52): node d of path j uniform in [0, num_node) from a counter-based
 * splitmix64 keyed by (seed, v, j, d) — the reference draws from an unseeded Random, so the stream is this library's own.
 * out_codes [num_item x J].  out_path_codes / out_path_sizes / out_num_paths: all NULL or all set; they receive the distinct codes of the CSR
 * in ascending order (at most total), their final sizes (int32) and their number.  trace_sel (int32) / trace_gain [num_iteration x n_hit x J]
 * (n_hit = items with occurrence > 0, in ascending id): both NULL or both set; the chosen candidate position inside the item's range and the
 * gain as computed, for every decision.  Needs a handle, not a model.
 * Refused before anything is read or allocated (DM_ERR_INVALID): J < 1, num_iteration < 1, penalty_poly_order outside [1, 8], penalty_factor
 * not finite or negative, num_node^num_layer not below 2^62, a null required array, a partly given optional group; DM_ERR_UNSUPPORTED:
 * total >= 2^31 or num_item * J >= 2^31.  Checked on the device before the loop runs (DM_ERR_INVALID, the first offending item in the
 * message, nothing written): offsets that decrease or leave [0, total] (item_off[0] = 0, item_off[num_item] = total), a hit item with fewer
 * than J or more than 2048 candidates, a code outside [0, num_node^num_layer), a score that is not finite or is negative, a path listed twice
 * by a hit item.  partial <= -1 or a winning gain that is not finite stops the loop: DM_ERR_INVALID with the item in the message (where
 * math.log1p raises on the host route).  num_item == 0 or no hit item: DM_OK.  The same inputs give the same bytes; the handle stays usable. */
int dm_dr_mstep_assign_paths(dm_handle_t h, const int64_t *item_off, const int64_t *codes, const double *scores, const int64_t *occurrence,
                             int64_t num_item, int64_t total, int num_node, int num_layer, int num_path_per_item, int num_iteration,
                             double penalty_factor, int penalty_poly_order, uint64_t seed, int64_t *out_codes, int64_t *out_path_codes,
                             int32_t *out_path_sizes, int64_t *out_num_paths, int32_t *trace_sel, double *trace_gain);
/* the same with device arrays; out_num_paths stays a host pointer; returns when the results are in place */
int dm_dr_mstep_assign_paths_dev(dm_handle_t h, const int64_t *d_item_off, const int64_t *d_codes, const double *d_scores,
                                 const int64_t *d_occurrence, int64_t num_item, int64_t total, int num_node, int num_layer,
                                 int num_path_per_item, int num_iteration, double penalty_factor, int penalty_poly_order, uint64_t seed,
                                 int64_t *d_out_codes, int64_t *d_out_path_codes, int32_t *d_out_path_sizes, int64_t *out_num_paths,
                                 int32_t *d_trace_sel, double *d_trace_gain);
/* CoordinateDescent.optimize (:29-83) in one call: the path scores of dm_dr_mstep_path_scores (mode 0) or
 * dm_dr_mstep_streaming_path_scores (mode 1, with decay_factor) and the assignment above on them; the candidates and the CSR never leave the
 * device.  Host arrays in, out_codes [num_item x J] out; num_node / num_layer are the loaded model's.  Every check of
 * dm_dr_mstep_path_scores holds as it is, then those of the assignment; mode outside {0, 1}: DM_ERR_INVALID. */
int dm_dr_mstep_optimize(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N, int num_candidate_path, int mode,
                         double decay_factor, int num_path_per_item, int num_iteration, double penalty_factor, int penalty_poly_order,
                         uint64_t seed, int64_t *out_codes);

/* ---- Deep-Retrieval: the mapping and the training set resident on the device ----
 * All of it is state of the loaded model: dm_dr_load_model drops it, every entry point below is refused on a clone and without a model
 * (DM_ERR_STATE), and every refusal leaves the handle usable and allocates nothing.
 *
 * MappingOp.itemPathMapping: item_paths [num_item x J x D] nodes (host).  The table stays on the device, and the path -> items CSR is built
 * from it there (no host sort): exactly what dm_dr_load_path_items leaves behind for the host inversion of the same table - distinct path
 * codes sum_d node_d K^(D-1-d) ascending, the items of a path in ascending id, an item that lists one path twice counted once.  A node
 * outside [0, num_node): DM_ERR_INDEX; J < 1 or a null array: DM_ERR_INVALID; num_item J >= 2^31 or num_node^num_layer >= 2^62: DM_ERR_UNSUPPORTED. */
int dm_dr_set_item_paths(dm_handle_t h, const int32_t *item_paths, int J);
/* the CSR after either loader: sizes, then codes [n_paths], item_off [n_paths + 1], items [n_items] (host).  DM_ERR_STATE before a loader. */
int dm_dr_path_items_size(dm_handle_t h, int64_t *n_paths, int64_t *n_items);
int dm_dr_path_items_download(dm_handle_t h, int64_t *codes, int64_t *item_off, int32_t *items);
/* the resident table [num_item x J x D]; n must be that product (DM_ERR_INVALID); DM_ERR_STATE before dm_dr_set_item_paths */
int dm_dr_item_paths_download(dm_handle_t h, int32_t *out, int64_t n);
/* the training set: seq_ids [N x L] internal ids (-1 = padding), targets [N]; uploaded once, the order set to the identity.  An id outside
 * [-1, num_item) or a target outside [0, num_item): DM_ERR_INDEX; N < 1 or a null array: DM_ERR_INVALID; N >= 2^31: DM_ERR_UNSUPPORTED. */
int dm_dr_train_set_load(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N);
int dm_dr_train_set_free(dm_handle_t h);                            /* the model, the mapping and the training state stay */
/* what the handle holds: the samples of the resident set (0: none) and the paths per item of the resident table (0: none) - the extents of
 * dm_dr_train_set_order_download's out [N], dm_dr_item_paths_download's n and dm_dr_train_set_mstep's out_codes [num_item x J] */
int dm_dr_train_set_size(dm_handle_t h, int64_t *n_samples, int32_t *n_paths_per_item);
/* The order of an epoch: the sample indices sorted (stable) ascending by the 64-bit key splitmix(splitmix(seed ^ splitmix(epoch)) + i).
 * LocalDataSet.scala shuffles with an unseeded Random, so this stream is the library's own, as the rerank sampler's is.  DM_ERR_STATE
 * without a set. */
int dm_dr_train_set_shuffle(dm_handle_t h, uint64_t seed, int64_t epoch);
int dm_dr_train_set_order_download(dm_handle_t h, int32_t *out);   /* out [N] */
/* One layer step on the samples order[offset .. offset + length): their histories and the [J x D] paths of their targets are gathered on
 * the device, then dm_dr_train_forward_backward_grouped_dev (grouped != 0) or dm_dr_train_forward_backward_dev on the expanded batch of
 * transformLayerData (grouped == 0) runs as it is; out_loss [D] (host, or NULL).  No Adam step and no exchange: dm_dr_adam_step and
 * dm_dr_train_sync_gradients follow as after the host-batch calls.  DM_ERR_STATE without a set, a mapping or dm_dr_train_init;
 * length < 1 or a range outside [0, N]: DM_ERR_INVALID; the row limits of the step it runs: DM_ERR_UNSUPPORTED. */
int dm_dr_train_set_forward_backward(dm_handle_t h, int64_t offset, int64_t length, int grouped, double *out_loss);
/* the rerank step on the same range: dm_dr_rerank_forward_backward_dev with the negatives drawn on the device.  DM_ERR_STATE without a set
 * or dm_dr_rerank_train_init; the range as above; that step's row limits and 2 num_sampled > num_item: DM_ERR_UNSUPPORTED. */
int dm_dr_train_set_rerank_forward_backward(dm_handle_t h, int64_t offset, int64_t length, double *out_loss);
/* dm_dr_mstep_optimize over the resident set, always in STORAGE order (the streaming fold depends on the order of the samples; a shuffle
 * does not change the result); the number of paths per item is the resident table's.  The new codes are decoded on the device into the
 * table and the CSR is rebuilt from it; out_codes [num_item x J] (host) may be NULL.  DM_ERR_STATE without a set or a mapping; every other
 * check of dm_dr_mstep_optimize holds. */
int dm_dr_train_set_mstep(dm_handle_t h, int num_candidate_path, int mode, double decay_factor, int num_iteration, double penalty_factor,
                          int penalty_poly_order, uint64_t seed, int64_t *out_codes);

/* ---- DeepFM: one training step on the device ----
 * LocalOptimizer.trainBatch with the DeepFM graph (T/optim/LocalOptimizer.scala:139-162, useMask = false; T/model/DeepFM.scala:11-45;
 * S/nn/FM.scala:24-71, S/nn/Linear.scala, S/nn/BCECriterionWithLogits.scala:27-64 averaged over the batch; S/optim/Adam.scala:19-73).
 * A batch is B rows (codes[r], seqs[r][0..L), labels[r]): node codes, -1 = a zero row that receives no gradient; L is the model's seq_len.
 * The trained vector is the model's own [emb ; l1.W ; l1.b ; l2.W ; l2.b]; fp32; no floating-point atomics, every sum in a fixed order:
 * the same state and batch give the same bytes.  Entry points of their own because the DIN ones (dm_train_*, dm_adam_step,
 * dm_tdm_make_train_batch, dm_tdm_sample_train_batch_dev) keep answering DM_ERR_UNSUPPORTED while a DeepFM model is loaded.
 * All of them: owner only (DM_ERR_STATE on a dm_clone clone), DM_ERR_STATE without a model or on a DIN model; the handle stays usable after
 * every refusal.  Any later dm_load_weights_* / dm_load_model drops the training state. */
int dm_deepfm_train_init(dm_handle_t h, const dm_adam_opts *opts);      /* zero gradient and moments; bad options: DM_ERR_INVALID */
int dm_deepfm_train_free(dm_handle_t h);                                /* the model keeps serving */
/* replaces the gradient with this batch's (zeroGradParameters + forward + backward, LocalOptimizer.scala:139-162); *out_loss (host, or NULL)
 * = the mean BCE-with-logits loss.  Host arrays, range-checked like LookupTable.scala:29-53 (an id outside [-1, num_index): DM_ERR_INDEX).
 * L != the model's seq_len, B <= 0 or a null array: DM_ERR_INVALID; before dm_deepfm_train_init: DM_ERR_STATE; B (L + 1) >= 2^31 or more
 * than 4 194 240 rows: DM_ERR_UNSUPPORTED. */
int dm_deepfm_train_forward_backward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, const float *labels, int64_t B, int L, double *out_loss);
/* the same on device arrays, NOT range-checked (an id outside [0, num_index) is read as -1); out_loss is still a host pointer */
int dm_deepfm_train_forward_backward_dev(dm_handle_t h, const int32_t *d_codes, const int32_t *d_seqs, const float *d_labels, int64_t B, int L, double *out_loss);
/* the same step on a user-grouped batch: U histories d_seq_codes [U][L] and rows_per_user candidate rows per user,
 * d_codes / d_labels [U * rows_per_user] user-major; row u * rows_per_user + r reads history u, B = U * rows_per_user.  Every history is
 * read once per user, never once per row; the gradient is the row step's on the expanded rows up to float32 rounding (other, fixed
 * summation orders).  Device arrays, NOT range-checked (an id outside [0, num_index) is read as -1); out_loss is a host pointer or NULL.
 * U <= 0, rows_per_user <= 0, a null array or L != the model's seq_len: DM_ERR_INVALID; before dm_deepfm_train_init: DM_ERR_STATE;
 * B > 4 194 240 or B + U L >= 2^31: DM_ERR_UNSUPPORTED.  dm_deepfm_otm_train_batch takes it for its level batches under
 * DM_DFM_TRAIN_GROUPED=1 (read per call). */
int dm_deepfm_train_forward_backward_grouped_dev(dm_handle_t h, const int32_t *d_seq_codes, const int32_t *d_codes, const float *d_labels, int64_t U,
                                                 int rows_per_user, int L, double *out_loss);
/* the same step on a ragged user-grouped batch: rows d_row_off[u] .. d_row_off[u + 1] of d_codes / d_labels [B] belong
 * to user u and read d_seq_codes[u]; a user may have no rows (its history is then never read).  The offsets are validated on the device
 * before anything is read through them: d_row_off[0] == 0, non-decreasing, d_row_off[U] == B, else DM_ERR_INVALID naming the first offending
 * user.  With uniform offsets the bytes of dm_deepfm_train_forward_backward_grouped_dev.  Device arrays, ids NOT range-checked (an id outside
 * [0, num_index) is read as -1); out_loss is a host pointer or NULL.  U <= 0, B <= 0, a null array or L != the model's seq_len:
 * DM_ERR_INVALID; before dm_deepfm_train_init: DM_ERR_STATE; U or B > 4 194 240 or B + U L >= 2^31: DM_ERR_UNSUPPORTED. */
int dm_deepfm_train_forward_backward_csr_dev(dm_handle_t h, const int32_t *d_seq_codes, const int64_t *d_row_off, const int32_t *d_codes, const float *d_labels,
                                             int64_t U, int64_t B, int L, double *out_loss);
/* Adam.optimize (S/optim/Adam.scala:19-73) over the vector with dm_dr_adam_step's rules: the embedding rows a gradient has ever reached plus
 * the dense blocks, or the whole vector when eps == 0, when a quarter of the rows is active or under DM_ADAM_DENSE=1 - the same bytes
 * either way.  Rebuilds every copy the searches read and tells the clones: serving continues with the new weights. */
int dm_deepfm_adam_step(dm_handle_t h, float grad_scale);
/* LocalOptimizer.syncGradients (T/optim/LocalOptimizer.scala:164-187) minus the division, which dm_deepfm_adam_step(1 / N) folds in, over the
 * communicator attached with dm_comm_attach: after any of the three steps above, every replica holds for every table
 * row any rank reached ((0 + g_0) + g_1) + ... in rank order (ranks that did not reach the row are skipped) and the rank-ordered sum of the
 * dense blocks, on BOTH transports: the fp32 sum of the ranks' local gradients bit for bit, no floating-point atomics.  One var-size
 * all-gather of [row ids | gradient rows | dense blocks] through the path of dm_comm_all_gather_dev; the table never moves.  A rank that
 * ran no step since its last Adam step (its sampler drew no rows) takes part with no rows and a zero dense part.  Collective: every rank
 * calls it.  Ranks that train different shapes (num_index, padded embed size, seq_len) ALL return DM_ERR_STATE before any gradient
 * moves.  Before any collective, with the handle left usable: DM_ERR_STATE without a communicator, without dm_deepfm_train_init, on a clone,
 * on a DIN model, and for a second exchange with no forward/backward or Adam step in between (it would sum a sum).  A one-rank
 * communicator: DM_OK, nothing moves.  dm_train_sync_stats reports what the call moved (host synchronisations: waits on the handle's
 * stream). */
int dm_deepfm_train_sync_gradients(dm_handle_t h);
int dm_deepfm_train_param_count(dm_handle_t h, int64_t *n);             /* of the model's own (unpadded) layout */
/* what: 0 weights (needs no training state), 1 gradient, 2 first moment, 3 second moment, in the model's own layout; n must be the
 * parameter count (DM_ERR_INVALID) */
int dm_deepfm_train_download(dm_handle_t h, int what, float *out, int64_t n);
/* dm_tdm_make_train_batch / dm_tdm_sample_train_batch_dev for a DeepFM model (NegativeSampler.scala:76-158 + MiniBatch.convert,
 * T/dataset/MiniBatch.scala:49-88 without transformWithMask): the same rows from the same seed, no row mask.  opts->use_mask must be 0 and
 * L the model's seq_len (DM_ERR_INVALID). */
int dm_deepfm_make_train_batch(dm_handle_t h, const int32_t *seq_item_ids, const int32_t *target_item_ids, int64_t T, int L,
                               const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *out_codes,
                               int32_t *out_seqs, float *out_labels, int64_t cap, int64_t *n_rows);
int dm_deepfm_sample_train_batch_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                     const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                     int32_t *d_seqs, float *d_labels, int64_t cap, int64_t *n_rows);
/* dm_deepfm_sample_train_batch_dev in the form dm_deepfm_train_forward_backward_csr_dev reads: the same d_codes / d_labels from the same seed,
 * d_seq_codes [T][L] = every target's history as codes, written once per target (also for a target that yields no rows), d_row_off [T + 1] =
 * the first row of every target.  No [cap][L] histories are written.  Size query (d_codes == NULL), checks and refusals: the row twin's. */
int dm_deepfm_sample_train_batch_csr_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                         const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                         int32_t *d_seq_codes, int64_t *d_row_off, float *d_labels, int64_t cap, int64_t *n_rows);

/* ---- Deep-Retrieval E-step: one training step of the LAYER model on the device ----
 * D/model/LayerModel.scala:22-49, D/dataset/MiniBatch.scala:18-50, D/loss/CrossEntropyLayer.scala, D/optim/LocalOptimizer.scala:58-116.
 * A batch is B rows, one per (training sample, one of the target item's J paths) — the host expands the J paths per item, as
 * transformLayerData does: seq_ids [B x seq_len] internal ids (-1 = padding: a zero row that receives no gradient), paths [B x D] nodes
 * in [0, K).  Per layer d: Z_d = X_d W_d^T + b_d over X_d[r] = [emb[seq] ; emb[num_item + t K + path[r][t]], t < d], loss_d = the mean
 * over the B rows of -log softmax(Z_d[r])[path[r][d]] (targets 0-based, sizeAverage), and the gradient of sum_d loss_d.
 * The gradient is the mean over the WHOLE batch: the reference splits a batch over its threads and averages the per-thread means
 * (LocalOptimizer.scala:135-194), the same value whenever the thread count divides B.
 * The trainable vector is [layer_emb ; W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}], in the model's type (DM_F64 is the reference's); the rerank
 * arrays are neither read nor written (their step: dm_dr_rerank_*, below).  There is one copy of the embedding table: the search reads the vector's first section.
 * Every sum has a fixed order: the same state and the same batch give the same bytes in gradient and weights, run to run.
 * All of these are refused on a clone (DM_ERR_STATE); dm_dr_load_model on a training handle drops the training state. */
int dm_dr_train_init(dm_handle_t h, const dm_adam_opts *opts);      /* needs dm_dr_load_model (DM_ERR_STATE); zero gradient and moments */
int dm_dr_train_free(dm_handle_t h);                                /* the model keeps serving */
/* replaces the gradient with this batch's (zeroGradParameters + forward + backward); out_loss [D] (host) or NULL.  Range-checks ids and
 * nodes (DM_ERR_INDEX); B <= 0 or a null array is DM_ERR_INVALID; DM_ERR_STATE before dm_dr_train_init; more than 4 194 240 rows, or
 * B (L + D - 1) >= 2^31, is DM_ERR_UNSUPPORTED. */
int dm_dr_train_forward_backward(dm_handle_t h, const int32_t *seq_ids, const int32_t *paths, int64_t B, double *out_loss);
/* the same on device arrays, NOT range-checked; out_loss is still a host pointer (the call synchronizes) */
int dm_dr_train_forward_backward_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_paths, int64_t B, double *out_loss);
/* The same step on a sample-grouped batch: S samples, seq_ids [S x L], each with J >= 1 paths, paths [S x J x D];
 * row r = s J + j, R = S J, every mean over R.  The value of dm_dr_train_forward_backward on the expanded batch (each history repeated
 * J times), re-associated: every history product runs once per sample instead of once per row.  Fixed summation order, no floating-point
 * atomics; the handle is left as the row call leaves it, so dm_dr_adam_step and dm_dr_train_sync_gradients follow either.  Range-checks
 * ids and nodes before anything is uploaded (DM_ERR_INDEX); S <= 0, J <= 0 or a null array DM_ERR_INVALID; DM_ERR_STATE before
 * dm_dr_load_model / dm_dr_train_init and on a clone; S J > 4 194 240 or S L + S J (D - 1) >= 2^31 DM_ERR_UNSUPPORTED. */
int dm_dr_train_forward_backward_grouped(dm_handle_t h, const int32_t *seq_ids, const int32_t *paths, int64_t S, int64_t J, double *out_loss);
/* the same on device arrays, NOT range-checked; out_loss is still a host pointer (the call synchronizes) */
int dm_dr_train_forward_backward_grouped_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_paths, int64_t S, int64_t J, double *out_loss);
/* Evaluator.evaluateLayerModel (D/evaluation/Evaluator.scala): the per-layer cross-entropy out_loss [D] of the grouped batch, the mean
 * over its S J rows; forward only, in chunks of samples (DM_DR_LAYER_LOSS_ROWS in the environment forces a chunk size), chunk sums added in
 * chunk order.  Needs a loaded model and no training state; gradient, remembered rows and optimizer state are neither read nor written.
 * Host arrays, range-checked (DM_ERR_INDEX); S <= 0, J <= 0 or a null argument DM_ERR_INVALID; J > 4 194 240 DM_ERR_UNSUPPORTED; a clone
 * DM_ERR_STATE. */
int dm_dr_layer_loss(dm_handle_t h, const int32_t *seq_ids, const int32_t *paths, int64_t S, int64_t J, double *out_loss);
/* Adam.optimize (scalann/.../optim/Adam.scala:19-73) over the vector with dm_adam_step's kernels and rules (lr_decay, bias correction,
 * gradient scaled by grad_scale and zeroed): the embedding rows a gradient has ever reached plus the dense blocks, or the whole vector
 * when eps == 0, when a quarter of the rows is active or under DM_ADAM_DENSE=1 — the same bytes either way.  Marks the search's derived
 * copies (history columns, node tables, split planes) stale: the next search rebuilds them, not every step. */
int dm_dr_adam_step(dm_handle_t h, float grad_scale);
/* LocalOptimizer.syncGradients (D/optim/LocalOptimizer.scala:167-194) minus the division, which dm_dr_adam_step(1 / P) folds in, over the
 * communicator attached with dm_comm_attach: after dm_dr_train_forward_backward on each rank's slice, every replica
 * holds for every embedding row any rank reached ((0 + g_0) + g_1) + ... in rank order (ranks that did not reach the row are skipped) and
 * the rank-ordered sum of the dense blocks [W_0 ; b_0 ; ...], in the model's dtype and on BOTH transports: the sum of the ranks' local
 * gradients bit for bit, no floating-point atomics.  One var-size all-gather of [row ids | gradient rows | dense blocks]; the table
 * never moves.  A rank that ran no step since dm_dr_train_init or its last Adam step takes part with no rows and a zero dense part.
 * Collective: every rank calls it.  Ranks that train different shapes or dtypes ALL return DM_ERR_STATE before any gradient moves.
 * Before any collective, with the handle left usable: DM_ERR_STATE without a Deep-Retrieval model, without dm_dr_train_init, on a clone,
 * without a communicator, and for a second exchange with no forward/backward or Adam step in between (it would sum a sum).  A one-rank
 * communicator: DM_OK, nothing moves.  dm_train_sync_stats reports what the call moved. */
int dm_dr_train_sync_gradients(dm_handle_t h);
int dm_dr_train_param_count(dm_handle_t h, int64_t *n);
/* what: 0 weights (needs no training state), 1 gradient, 2 first moment, 3 second moment; n must be the parameter count (DM_ERR_INVALID) */
int dm_dr_train_download(dm_handle_t h, int what, void *out, int64_t n);

/* ---- Deep-Retrieval E-step: one training step of the RERANK model on the device ----
 * D/model/RerankModel.scala, scalann nn/SampledSoftmaxLoss.scala + nn/mixin/ParameterOptimizer.scala, D/dataset/MiniBatch.scala:52-61,
 * D/optim/LocalOptimizer.scala:118-133, D/evaluation/Evaluator.scala:83-93.  The second half of LocalOptimizer.optimize; independent of the
 * layer model's training state (dm_dr_train_*), and possible on the same handle at the same time.
 * A batch is B samples: seq_ids [B x seq_len] internal ids (-1 = padding: a zero row that receives no gradient), targets [B] in
 * [0, num_item).  With S = num_sampled: U = X rerank_w^T + rerank_b over X[r] = [rerank_emb[seq[r][j]]]; the classes of row r are its
 * target (slot 0) and S negatives; z[r][s] = softmax_w[class] . U[r] + softmax_b[class]; loss = the mean over the rows of
 * -log softmax(z[r])[0]; and the gradient of that loss with respect to all five arrays.
 * Two trainable vectors in the model's type, each with its own Adam: vec 0 = [rerank_emb ; rerank_w ; rerank_b] (the graph's optimizer,
 * gradient replaced by every batch) and vec 1 = [softmax_w ; softmax_b] (the criterion's own optimizer).  The reference never clears the
 * criterion's gradient (ParameterOptimizer.scala:65-88 only adds): accumulate != 0 keeps that running sum over all batches since init and
 * is what parity with the reference means; accumulate == 0 replaces it per batch, as every other gradient here.
 * dm_dr_recommend reads the two vectors in place: what a step wrote is what the next recommend serves, no copy, nothing to refresh.
 * Every sum has a fixed order and there are no floating-point atomics: the same state, batch, seed and step give the same bytes.
 * All of these are refused on a clone, on a model loaded without the five rerank arrays and (except init) before init (DM_ERR_STATE);
 * dm_dr_load_model drops the state. */
/* softmax == NULL: the reference's criterion optimizer (lr = graph->lr, beta 0.9 / 0.999, eps 1e-7, no decay).  num_sampled < 1 or
 * >= num_item is DM_ERR_INVALID (the reference requires numSampled < numClasses), num_sampled + 1 > 256 DM_ERR_UNSUPPORTED.  Zero
 * gradients and moments, both time steps at 0; released again when any allocation fails. */
int dm_dr_rerank_train_init(dm_handle_t h, const dm_adam_opts *graph, const dm_adam_opts *softmax, int num_sampled, uint64_t seed, int accumulate);
int dm_dr_rerank_train_free(dm_handle_t h);                         /* the model keeps serving */
/* forward + backward of one batch; out_loss: one double (host) or NULL.  negatives [B x num_sampled] or NULL.  NULL: the device draws
 * them (distinct, != target, uniform, ascending; `step` = the number of forward_backward calls on this state so far, what
 * dm_dr_rerank_sample reproduces) — offered for 2 num_sampled <= num_item, DM_ERR_UNSUPPORTED above ("pass the negatives").  Given
 * negatives are range-checked like sequence ids and targets (DM_ERR_INDEX) but may repeat within a row and may equal the target.  More
 * than 4 194 240 rows, or B max(seq_len, num_sampled + 1) >= 2^31, is DM_ERR_UNSUPPORTED; B <= 0 or a null array DM_ERR_INVALID. */
int dm_dr_rerank_forward_backward(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, const int32_t *negatives, int64_t B, double *out_loss);
/* the same on device arrays, NOT range-checked; out_loss is still a host pointer (the call synchronizes) */
int dm_dr_rerank_forward_backward_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_targets, const int32_t *d_negatives, int64_t B, double *out_loss);
/* the draw alone: out [B x num_sampled] (host) for (seed of init, step, row).  Advances nothing. */
int dm_dr_rerank_sample(dm_handle_t h, const int32_t *targets, int64_t B, int64_t step, int32_t *out);
/* both Adam updates, each with its own time step; dm_dr_adam_step's rules per vector (active rows, or the whole vector when eps == 0,
 * when a quarter of the rows is active or under DM_ADAM_DENSE=1).  The accumulating criterion's gradient is left as it is. */
int dm_dr_rerank_adam_step(dm_handle_t h, float grad_scale);
/* vec: 0 [rerank_emb ; rerank_w ; rerank_b], 1 [softmax_w ; softmax_b]; what: 0 weights (needs no training state), 1 gradient, 2 first
 * moment, 3 second moment; n must be the vector's length (DM_ERR_INVALID) */
int dm_dr_rerank_download(dm_handle_t h, int vec, int what, void *out, int64_t n);
/* Evaluator.evaluateReRankModel's fullEvaluate: -mean log softmax(U softmax_w^T + softmax_b)[target] over ALL num_item classes, in row
 * chunks under 256 MB of logits (DM_DR_FULL_LOSS_ROWS in the environment forces a chunk size), chunk sums added in chunk order.
 * Needs no training state. */
int dm_dr_rerank_full_loss(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t B, double *out);

/* ---- synthetic-data helpers (bench / tests only; nothing in the reference corresponds) ---- */
/* fill d_ptr[0..n) (float, device) with N(mean, std): counter-based splitmix64 + Box-Muller, reproducible per (seed, index) */
int dm_fill_normal(dm_handle_t h, float *d_ptr, int64_t n, float mean, float std, uint64_t seed);
/* the same values (the f32 draws, widened) into a double buffer: an fp64 model with the weights of the f32 one */
int dm_fill_normal_f64(dm_handle_t h, double *d_ptr, int64_t n, float mean, float std, uint64_t seed);
/* tree-correlated table for a heap of `depth` levels below the root: row(root) ~ N(0, std),
 * row(c) = rho * row(parent(c)) + sqrt(1 - rho^2) * N(0, std) — a stand-in for a trained index, where
 * a node's embedding summarises its subtree (with iid rows beam search has nothing to follow and
 * recall vs brute force is ~0 by construction). */
int dm_fill_tree_normal(dm_handle_t h, float *d_emb, int E, int depth, float rho, float std, uint64_t seed);
/* like dm_load_weights_din(DM_F32) but the compact vector already lives in device memory; the handle
 * takes ownership of d_compact (freed with the handle / on the next load). */
int dm_load_weights_din_dev(dm_handle_t h, int E, int64_t num_index, float *d_compact, int64_t n_elems);
/* the same for an fp64 model (dm_load_weights_din(DM_F64): the reference's OTM scorer is DIN[Double]) */
int dm_load_weights_din_dev_f64(dm_handle_t h, int E, int64_t num_index, double *d_compact, int64_t n_elems);

/* ---- TDMClusterTree: the balanced recursive 2-means tree rebuild ----------------
 * RecursiveCluster.run (T/cluster/RecursiveCluster.scala:34-60,141-198, ForkJoinProcess.scala): every node fits 2-means on its
 * items' embeddings (k-means++ seeds, Lloyd, `restarts` independent restarts, the lowest distortion wins — smile's
 * PartitionClustering.run), takes every item's squared distance to centroid 0 — here the cluster seeded FIRST; smile's order is as
 * arbitrary — and sends the n/2 nearest to child 2c+1 and the other n - n/2 to 2c+2, down to single items.  A node of two items
 * puts its first left and its second right.  The reference is unseeded; here the result is a pure function of (embeddings, seed).
 * Lloyd's stopping rule, the tie rules and the empty-cluster rule are stated in dismember_amd/csrc/cluster.hip.inc and restated
 * in tests/cluster_ref.py.  max_level = ceil(log2 n); leaf codes come out on levels max_level - 1 and max_level (before
 * TreeBuilder.flattenLeaves).  1 <= n <= 2^30, 1 <= E <= 128, 1 <= restarts <= 32.  n = 1 gives code 0. */

/* Optional diagnostics, host buffers owned by the caller (any pointer may be NULL).  Per-node arrays are indexed by the internal
 * node's code c < 2^max_level - 1; nodes that were never fitted (fewer than three items) keep NaN / -1 / 0. */
typedef struct {
  int64_t node_cap;    /* entries the per-node arrays hold: >= 2^max_level - 1 */
  int32_t level_cap;   /* rows `dist` holds: >= max_level */
  float *centroid0;    /* [node_cap, E] centroid 0 of the winning restart */
  int32_t *seeds;      /* [node_cap, 2] row numbers (into the embeddings given) of the winning restart's two seeds */
  int32_t *iters;      /* [node_cap] its Lloyd iterations */
  double *distortion;  /* [node_cap] its final distortion */
  float *dist;         /* [level_cap, n] by row: the distance the item had at the node of that level where it was split; NaN where
                          it was a leaf already or the node had two items */
  int32_t *perm;       /* [n] rows in final leaf order: the items of node (level l, index j) are one contiguous run of it */
} dm_cluster_trace;

typedef struct {
  int32_t levels_streamed, levels_lds;  /* levels split by passes over the table / finished inside the LDS */
  int64_t lloyd_passes, bytes_streamed; /* Lloyd iterations summed over the streamed levels; bytes of embeddings read by all passes */
  double seeding_s, lloyd_s, split_s, lds_s; /* wall seconds per phase */
} dm_cluster_stats;

/* emb: host, [n, E] row-major, every value finite: a NaN or an infinity is refused with DM_ERR_INVALID (the message names the first
 * such row) before any kernel runs, by this entry point and by dm_cluster_tree_model alike.  codes_out [n]: leaf code of row i. */
int dm_cluster_tree(dm_handle_t h, const float *emb, int64_t n, int E, int restarts, int max_iter, double tol, uint64_t seed,
                    int32_t *codes_out, const dm_cluster_trace *trace, dm_cluster_stats *stats);
/* The embeddings are the loaded DIN table's rows at the items' CURRENT leaf codes in the loaded tree (what TDM.saveModel writes to
 * embed_path, T/utils/Serialization.scala:15-58), gathered on the device.  DM_ERR_STATE without a tree or weights, DM_ERR_INVALID
 * for an id that is not a leaf of the tree. */
int dm_cluster_tree_model(dm_handle_t h, const int32_t *item_ids, int64_t n, int restarts, int max_iter, double tol, uint64_t seed,
                          int32_t *codes_out, const dm_cluster_trace *trace, dm_cluster_stats *stats);
/* the same rows read back: out [n, E] with E the model's embed size */
int dm_get_leaf_embeddings(dm_handle_t h, const int32_t *item_ids, int64_t n, float *out);

/* ---- measurement ----------------------------------------------------------- */
/* HIP events on the handle's stream around every beam-search kernel launched since the last
 * reset: number of launches and their summed duration. */
/* HIP-event pairs around the kernels launched since the last reset (at most the 4096 most recent launches) */
int dm_kernel_timing_reset(dm_handle_t h);
int dm_kernel_timing_get(dm_handle_t h, int *launches, double *total_ms);
/* the same, one kind of launch only: 0 = the search kernels proper, 1 = the second pass over the users the
 * one-wave-per-SIMD beam kernel hands to the LDS-fed kernel (one launch per search, empty on most inputs).
 * A Deep-Retrieval search is several launches: by default ONE pair brackets the whole search (kind 0); with
 * DM_DR_TIME_LAUNCHES=1 in the environment (read per call) every launch gets its own pair — kind 0 the history
 * GEMM, 11 layer 0, 10 + 2d / 11 + 2d the statistics / cut of layer d — at 2 - 14 % of the search's wall time.
 * Kind 30: the general-rows scorer (dm_din_forward, JTM child weights: dm_din_rows_split*_kernel), one pair per launch.
 * Kinds 40 / 41: a DeepFM search's user set-up (dfm_user_kernel, one per pass of users) / its level kernel (dfm_level_kernel, one per level).
 * Kinds 42 / 43: the DeepFM pair scorer's per-history set-up (dfm_jtm_rows_kernel) / its per-pair kernel (dfm_jtm_pairs_kernel), one
 * pair each per slice of histories of a chunk. */
int dm_kernel_timing_get_kind(dm_handle_t h, int kind, int *launches, double *total_ms);
/* name (with template arguments) of the kernel that ran the last TDM / OTM beam search, as a profiler lists it
 * (owned by the handle, valid until the next search) */
const char *dm_last_beam_kernel(dm_handle_t h);
/* scored rows (node, user) pairs of the last beam-search call, for roofline accounting */
int dm_last_scored_rows(dm_handle_t h, int64_t *rows);

#ifdef __cplusplus
}
#endif
#endif /* DISMEMBER_HIP_H */
