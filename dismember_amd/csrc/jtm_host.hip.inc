// JTM / OTM tree-learning re-assignment (SURVEY.md §8 row A9).
//   scoring   : TreeLearning.aggregateWeights (jtm/src/main/scala/com/mass/jtm/optim/TreeLearning.scala:152-174)
//               -> every (training row of an item) x (node on a child->parent chain) is one row of the
//               general-rows DIN kernel; the per-(item,node) Tensor.sum() and the chain accumulation are
//               redone in the reference's sequential fp32 order (on the device for JTM, on the host in double for OTM).
//   assignment: sortNodeWeights (:137-150) + reBalance (:217-265), exact integer/float logic on the host.

// JTMTree.getAncestorAtLevel (jtm/.../tree/JTMTree.scala:36-43)
static inline int32_t jtm_ancestor_code(int32_t code, int level) {
  const int64_t lim = ((int64_t)1 << (level + 1)) - 1;
  while (code >= lim) code = (code - 1) >> 1;
  return code;
}

static int java_float_compare_h(float x, float y) {
  if (x < y) return -1;
  if (x > y) return 1;
  int32_t a, b;
  if (x != x) a = 0x7fc00000; else memcpy(&a, &x, 4);
  if (y != y) b = 0x7fc00000; else memcpy(&b, &y, 4);
  return a == b ? 0 : (a < b ? -1 : 1);
}

// ---- device side of the scoring: pairs (training row of an item) x (node on a child->parent chain) are expanded, scored
//      and summed on the GPU; the host only slices the items into chunks.  Pair order inside a chunk: item, row, chain node
//      (levels old+1 .. level, left to right): the 2^(gap+1) - 2 pairs of one training row are ADJACENT, so the rows of a
//      16-row scorer tile share their history and the tile's key loads coalesce to two or three distinct histories instead of
//      sixteen (the order in which the reference runs its forwards — node, then row — only matters to the sums, which
//      dm_jtm_sum_kernel redoes in that order).
struct JtmExpandParams {
  const int64_t *row_off;      // [n_items + 1] (chunk-local item index, absolute row numbers)
  const int32_t *row_item;     // [rows of the chunk] item index of every row, minus item_base = chunk-local
  int32_t item_base;
  const int32_t *row_ids;      // [rows of the chunk][L] raw item ids
  const int32_t *item_node;    // [n_items]
  const int32_t *id_to_code;
  int64_t R0, n_rows, num_index;
  int L, gap, old_level, hierarchical, min_level, use_mask;
  int32_t non_leaf_offset, max_code;
  int32_t *codes, *seqs;       // [pairs], [pairs][L]
  unsigned *rmask;             // [pairs]
  int *bad;                    // set when a history code falls outside the embedding table
};

__global__ void dm_jtm_expand_kernel(JtmExpandParams p) {
  const int nchain = (2 << p.gap) - 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.n_rows * nchain) return;
  const int64_t R = t / nchain;                 // chunk-local row
  const int x = (int)(t - R * nchain);          // chain node, level-major
  const int i = p.row_item[R] - p.item_base;
  const int64_t nr = p.row_off[i + 1] - p.row_off[i];
  const int64_t r = (p.R0 + R) - p.row_off[i];
  const int d = 31 - __clz(x + 2);              // depth below the item's node: nodes [2^d - 2, 2^(d+1) - 2)
  const int c = x - ((1 << d) - 2);
  const int lv = p.old_level + d;
  const int64_t q = ((p.row_off[i] - p.R0) + r) * nchain + x;
  (void)nr;
  p.codes[q] = (int32_t)(((int64_t)p.item_node[i] << d) + (1 << d) - 1 + c);
  unsigned m = 0;
  for (int j = 0; j < p.L; j++) {               // JTMTree.idToCodeWithMask, JTMTree.scala:86-113
    const int32_t id = p.row_ids[R * p.L + j];
    int32_t cd;
    if (id == 0) { cd = -1; m |= 1u << j; }
    else if (id < p.non_leaf_offset && id >= 0 && p.id_to_code[id] >= 0) {
      cd = p.id_to_code[id];
      if (p.hierarchical && lv >= p.min_level) {
        const int64_t lim = ((int64_t)1 << (lv + 1)) - 1;
        while (cd >= lim) cd = (cd - 1) >> 1;
      }
    } else {
      cd = (int32_t)((uint32_t)id - (uint32_t)p.non_leaf_offset);
      if (cd > p.max_code) cd = -1;
    }
    if (cd < -1 || cd >= p.num_index) { *p.bad = 1; cd = -1; }
    p.seqs[q * p.L + j] = cd;
  }
  p.rmask[q] = p.use_mask ? m : 0u;
}

// Round 5: with the catalogue's rows cached on the device (dm_jtm_cache_rows) and the ancestors NOT taken per level, a training row's
// history codes are the same in every gap step and for every chain node: they are built once per cached catalogue
// (dm_jtm_rowseq_kernel, JTMTree.idToCodeWithMask, JTMTree.scala:86-113), the scorer reads them per ROW (seq_div = chain nodes per row)
// and a gap step only writes the pairs' node codes (dm_jtm_codes_kernel): 4 bytes per pair instead of 4 + 4 L + 4 written and read back.
__global__ void dm_jtm_rowseq_kernel(const int32_t *row_ids, int64_t n_rows, int L, const int32_t *id_to_code, int32_t non_leaf_offset,
                                     int32_t max_code, int64_t num_index, int32_t *rseq, unsigned *rmask, int *bad) {
  const int64_t R = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (R >= n_rows) return;
  unsigned m = 0;
  for (int j = 0; j < L; j++) {
    const int32_t id = row_ids[R * L + j];
    int32_t cd;
    if (id == 0) { cd = -1; m |= 1u << j; }
    else if (id < non_leaf_offset && id >= 0 && id_to_code[id] >= 0) cd = id_to_code[id];
    else {
      cd = (int32_t)((uint32_t)id - (uint32_t)non_leaf_offset);
      if (cd > max_code) cd = -1;
    }
    if (cd < -1 || cd >= num_index) { *bad = 1; cd = -1; }
    rseq[R * L + j] = cd;
  }
  rmask[R] = m;
}
__global__ void dm_jtm_codes_kernel(const int64_t *row_off, const int32_t *row_item, int32_t item_base, const int32_t *item_node, int64_t R0,
                                    int64_t n_rows, int gap, int32_t *codes) {
  const int nchain = (2 << gap) - 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * nchain) return;
  const int64_t R = t / nchain;
  const int x = (int)(t - R * nchain);
  const int i = row_item[R] - item_base;
  const int d = 31 - __clz(x + 2);
  const int c = x - ((1 << d) - 2);
  codes[t] = (int32_t)(((int64_t)item_node[i] << d) + (1 << d) - 1 + c);     // (pair order = row-major: the same q as dm_jtm_expand_kernel's)
}

// Tensor.sum() per (item, node) in row order, then the child -> parent chain accumulation (TreeLearning.scala:163-171),
// both sequential fp32 like the reference; one thread per (item, child).
__global__ void dm_jtm_sum_kernel(const int64_t *row_off, int64_t R0, int64_t n_items, int gap, const float *logits, float *weights) {
#pragma clang fp contract(off)
  const int nchild = 1 << gap, nchain = (2 << gap) - 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items * nchild) return;
  const int64_t i = t / nchild;
  const int c = (int)(t - i * nchild);
  const int64_t nr = row_off[i + 1] - row_off[i];
  if (nr == 0) { weights[t] = -1e6f; return; }       // items that never appeared as a target (:160)
  const float *lg = logits + (row_off[i] - R0) * nchain;
  float w = 0.0f;
  int idx = c;
  for (int d = gap; d >= 1; d--) {
    const float *sc = lg + ((1 << d) - 2 + idx);
    float s = 0.0f;
    for (int64_t r = 0; r < nr; r++) s = s + sc[r * nchain];
    w = w + s;
    idx >>= 1;
  }
  weights[t] = w;
}

// DM_JTM_MAX_PAIRS=<positive integer>: scored rows per chunk of the child-weight loops, read per call like DM_JTM_REBALANCE (tests: chunk
// boundaries at catalogue sizes a test can afford); unset or invalid: the caller's default
static int64_t jtm_max_pairs(int64_t dflt) {
  const char *e = env_str("DM_JTM_MAX_PAIRS");
  if (!e || !*e) return dflt;
  char *end = nullptr;
  const long long v = strtoll(e, &end, 10);
  return (*end == 0 && v > 0) ? (int64_t)v : dflt;
}

// The scorer of the pairs is a parameter (DM_KIND_DIN: din_rows_dev, history masks included; DM_KIND_DEEPFM: dfm_pairs_dev of
// dfm_jtm.hip.inc, which has no mask input); the expansion, the chunk loop and the sums are shared.
static int dfm_pairs_dev(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, int64_t P, int L, float *d_out, int seq_div);
static int dfm_jtm_enter(dm_ctx *h, const char *who, int use_mask, int L);
static inline int jtm_max_L(int scorer) { return scorer == DM_KIND_DEEPFM ? 32 : DM_MAXL; }      // (32: DFM_MAXL)

// row_off / row_item_ids: host arrays of the items [0, n_items) — or, with cached = true, the handle's device copies made by
// dm_jtm_cache_rows (then the items are [i_lo, i_lo + n_items) of the cached catalogue and nothing but item_node goes up)
static int jtm_child_weights_impl(dm_ctx *h, int scorer, const int64_t *row_off, const int32_t *row_item_ids, bool cached, int64_t i_lo,
                                  const int32_t *item_node, int64_t n_items, int L, int old_level, int level, int hierarchical,
                                  int min_level, int use_mask, float *weights, const int32_t *d_item_node_all = nullptr,
                                  float *d_weights_all = nullptr) {
  // d_item_node_all / d_weights_all (both or neither): the assignment is already on the device and the weights stay there
  // (dm_jtm_step_cached: scoring and re-balance of a gap step without a host round trip)
  const bool resident = d_item_node_all != nullptr;
  if (resident) { item_node = (const int32_t *)1; weights = (float *)1; }    // host arrays unused
  if (!h->ids_loaded || !h->w_loaded) return fail(h, DM_ERR_STATE, "dm_jtm_child_weights: id maps and weights must be loaded first");
  if (h->dtype != DM_F32) return fail(h, DM_ERR_UNSUPPORTED, "dm_jtm_child_weights: f32 weights only");
  if (!row_off || !item_node || !weights || n_items < 0 || L <= 0 || L > jtm_max_L(scorer) || level <= old_level || level - old_level > 8)
    return fail(h, DM_ERR_INVALID, "dm_jtm_child_weights: bad arguments");
  if ((((int64_t)1) << (level + 1)) - 1 > h->num_index) return fail(h, DM_ERR_INDEX, "dm_jtm_child_weights: level exceeds the embedding table");
  HIPCHK(h, hipSetDevice(h->device));
  const int gap = level - old_level;
  const int nchild = 1 << gap;
  const int nchain = (2 << gap) - 2;            // distinct nodes below the item's node, levels old+1..level
  const int64_t max_pairs = jtm_max_pairs((int64_t)16 << 20);  // scored rows per chunk (640 MB of history codes at L = 10)
  std::vector<int32_t> row_item;
  int64_t *d_off = nullptr;
  int32_t *d_ritem = nullptr, *d_rids = nullptr, *d_node = nullptr, *d_codes = nullptr, *d_seqs = nullptr;
  unsigned *d_mask = nullptr;
  float *d_out = nullptr, *d_w = nullptr;
  int *d_bad = nullptr;
  size_t cap_pairs = 0, cap_rows = 0, cap_items = 0;
  // what this call allocates is t's; d_off / d_ritem / d_rids of a cached catalogue are the handle's and only pass through
  DevTemps t(h);
  int rc;
  if ((rc = t.alloc(d_bad, 4)) != DM_OK) return rc;
  (void)hipMemsetAsync(d_bad, 0, 4, h->stream);
  // the cached catalogue's per-row history codes (non-hierarchical scoring): built once per cached catalogue and id map
  const bool per_row = cached && !hierarchical;
  if (per_row && (!h->d_jtm_rseq || h->jtm_rseq_ids_epoch != h->ids_epoch || h->jtm_rseq_num_index != h->num_index)) {      // (the codes were bounds-checked against THAT table)
    const int64_t Rall = h->jtm_off[(size_t)h->jtm_i_hi] - h->jtm_R_base;       // the rows on this device (dm_jtm_cache_rows_range)
    dm_release(h->d_jtm_rseq, h->d_jtm_rmask);
    if ((rc = dm_alloc(h, (void **)&h->d_jtm_rseq, (size_t)(Rall > 0 ? Rall : 1) * L * 4)) != DM_OK ||
        (rc = dm_alloc(h, (void **)&h->d_jtm_rmask, (size_t)(Rall > 0 ? Rall : 1) * 4)) != DM_OK) return rc;
    if (Rall > 0 && (rc = LAUNCH(h, dm_jtm_rowseq_kernel, dim3((unsigned)((Rall + 255) / 256)), dim3(256), 0, h->d_jtm_rids, Rall, L, h->d_id_to_code, h->non_leaf_offset,
                                 h->max_code, h->num_index, h->d_jtm_rseq, h->d_jtm_rmask, d_bad)) != DM_OK) return rc;
    h->jtm_rseq_ids_epoch = h->ids_epoch; h->jtm_rseq_num_index = h->num_index;
  }
  if (cached && n_items > 0 && (i_lo < h->jtm_i_lo || i_lo + n_items > h->jtm_i_hi))
    return fail(h, DM_ERR_STATE, "dm_jtm_child_weights: items outside the range whose rows this handle holds (dm_jtm_cache_rows_range)");
  const int64_t Rb = cached ? h->jtm_R_base : 0;          // row numbers are absolute, the cached arrays start at the range's first row
  for (int64_t i0 = 0; i0 < n_items;) {
    int64_t i1 = i0, pairs = 0;
    while (i1 < n_items) {
      const int64_t add = (row_off[i1 + 1] - row_off[i1]) * nchain;
      if (pairs > 0 && pairs + add > max_pairs) break;
      pairs += add; i1++;
    }
    const int64_t ni = i1 - i0, R0 = row_off[i0], nrows = row_off[i1] - R0;
    const size_t own_rows = cached ? 0 : (size_t)nrows;       // rows this call has to hold itself
    if ((size_t)ni > cap_items) {
      t.drop(d_off); t.drop(d_node); t.drop(d_w);
      cap_items = (size_t)ni;
      if (!cached && (rc = t.alloc(d_off, (cap_items + 1) * 8)) != DM_OK) return rc;
      if (!resident && (rc = t.alloc(d_node, cap_items * 4)) != DM_OK) return rc;
      if (!resident && (rc = t.alloc(d_w, cap_items * nchild * 4)) != DM_OK) return rc;
    }
    if (own_rows > cap_rows) {
      t.drop(d_ritem); t.drop(d_rids);
      cap_rows = own_rows;
      if ((rc = t.alloc(d_ritem, cap_rows * 4)) != DM_OK) return rc;
      if ((rc = t.alloc(d_rids, cap_rows * L * 4)) != DM_OK) return rc;
    }
    if ((size_t)pairs > cap_pairs) {
      t.drop(d_codes); t.drop(d_seqs); t.drop(d_mask); t.drop(d_out);
      cap_pairs = (size_t)pairs;
      if ((rc = t.alloc(d_codes, cap_pairs * 4)) != DM_OK) return rc;
      if (!per_row && (rc = t.alloc(d_seqs, cap_pairs * L * 4)) != DM_OK) return rc;
      if (!per_row && (rc = t.alloc(d_mask, cap_pairs * 4)) != DM_OK) return rc;
      if ((rc = t.alloc(d_out, cap_pairs * 4)) != DM_OK) return rc;
    }
    hipError_t e = hipSuccess;
    if (cached) {
      d_off = h->d_jtm_off + (i_lo + i0);
      d_ritem = h->d_jtm_ritem + (R0 - Rb);
      d_rids = h->d_jtm_rids + (R0 - Rb) * L;
    } else {
      row_item.resize((size_t)nrows);
      for (int64_t i = i0; i < i1; i++)
        for (int64_t R = row_off[i]; R < row_off[i + 1]; R++) row_item[(size_t)(R - R0)] = (int32_t)(i - i0);
      e = hipMemcpyAsync(d_off, row_off + i0, (size_t)(ni + 1) * 8, hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess && nrows > 0) e = hipMemcpyAsync(d_ritem, row_item.data(), (size_t)nrows * 4, hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess && nrows > 0) e = hipMemcpyAsync(d_rids, row_item_ids + R0 * L, (size_t)nrows * L * 4, hipMemcpyHostToDevice, h->stream);
    }
    if (e == hipSuccess && !resident) e = hipMemcpyAsync(d_node, item_node + i0, (size_t)ni * 4, hipMemcpyHostToDevice, h->stream);
    const int32_t *d_node_use = resident ? d_item_node_all + i0 : d_node;
    float *d_w_use = resident ? d_weights_all + i0 * nchild : d_w;
    if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_jtm_child_weights: upload failed");
    if (pairs > 0 && per_row) {
      rc = LAUNCH(h, dm_jtm_codes_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, d_off, d_ritem, (int32_t)(i_lo + i0), d_node_use, R0, nrows, gap, d_codes);
      if (rc != DM_OK) return rc;
      rc = scorer == DM_KIND_DEEPFM ? dfm_pairs_dev(h, d_codes, h->d_jtm_rseq + (R0 - Rb) * L, pairs, L, d_out, nchain)
                                    : din_rows_dev(h, d_codes, h->d_jtm_rseq + (R0 - Rb) * L, use_mask ? h->d_jtm_rmask + (R0 - Rb) : nullptr, pairs, L, d_out, nchain);
      if (rc != DM_OK) return rc;
    } else if (pairs > 0) {
      JtmExpandParams p;
      p.row_off = d_off; p.row_item = d_ritem; p.item_base = cached ? (int32_t)(i_lo + i0) : 0; p.row_ids = d_rids; p.item_node = d_node_use;
      p.id_to_code = h->d_id_to_code;
      p.R0 = R0; p.n_rows = nrows; p.num_index = h->num_index; p.L = L; p.gap = gap; p.old_level = old_level;
      p.hierarchical = hierarchical; p.min_level = min_level; p.use_mask = use_mask;
      p.non_leaf_offset = h->non_leaf_offset; p.max_code = h->max_code;
      p.codes = d_codes; p.seqs = d_seqs; p.rmask = d_mask; p.bad = d_bad;
      if ((rc = LAUNCH(h, dm_jtm_expand_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, p)) != DM_OK) return rc;
      // (hierarchical: the histories differ per chain depth, so the DeepFM set-up runs once per pair here)
      rc = scorer == DM_KIND_DEEPFM ? dfm_pairs_dev(h, d_codes, d_seqs, pairs, L, d_out, 1) : din_rows_dev(h, d_codes, d_seqs, d_mask, pairs, L, d_out);
      if (rc != DM_OK) return rc;
    }
    if ((rc = LAUNCH(h, dm_jtm_sum_kernel, dim3((unsigned)((ni * nchild + 255) / 256)), dim3(256), 0, d_off, R0, ni, gap, d_out, d_w_use)) != DM_OK) return rc;
    e = resident ? hipSuccess : hipMemcpyAsync(weights + i0 * nchild, d_w, (size_t)ni * nchild * 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);       // row_item (host staging) is reused by the next chunk
    if (e != hipSuccess) return fail(h, DM_ERR_HIP, std::string("dm_jtm_child_weights: ") + hipGetErrorString(e));
    i0 = i1;
  }
  int bad = 0;
  if (hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DM_ERR_HIP, "dm_jtm_child_weights: readback failed");
  if (bad) {
    // the per-row code cache was built with the offending positions cleared: drop it, so that a retry reports the same error instead of scoring them as pads
    dm_release(h->d_jtm_rseq, h->d_jtm_rmask); h->jtm_rseq_ids_epoch = 0;
    return fail(h, DM_ERR_INDEX, "dm_jtm_child_weights: history code outside the embedding table");
  }
  return DM_OK;
}

int dm_jtm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, const int32_t *item_node,
                         int64_t n_items, int L, int old_level, int level, int hierarchical, int min_level, int use_mask,
                         float *weights) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  DM_DIN_ONLY(h, "dm_jtm_child_weights");
  return jtm_child_weights_impl(h, DM_KIND_DIN, row_off, row_item_ids, false, 0, item_node, n_items, L, old_level, level, hierarchical, min_level, use_mask, weights);
}

// The DeepFM twins of the scoring entry points (dm_deepfm_jtm_*): the same signatures, the pairs scored by dfm_pairs_dev.  use_mask must
// be 0 (the graph has no mask input), L the model's, one rank.
int dm_deepfm_jtm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, const int32_t *item_node,
                                int64_t n_items, int L, int old_level, int level, int hierarchical, int min_level, int use_mask,
                                float *weights) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  const int rc = dfm_jtm_enter(h, "dm_deepfm_jtm_child_weights", use_mask, L);
  if (rc != DM_OK) return rc;
  return jtm_child_weights_impl(h, DM_KIND_DEEPFM, row_off, row_item_ids, false, 0, item_node, n_items, L, old_level, level, hierarchical, min_level, 0, weights);
}

static void jtm_drop_cache(dm_ctx *h) {
  dm_release(h->d_jtm_off, h->d_jtm_ritem, h->d_jtm_rids, h->d_jtm_rseq, h->d_jtm_rmask);
  h->jtm_off.clear(); h->jtm_L = 0; h->jtm_i_lo = h->jtm_i_hi = h->jtm_R_base = 0;
}

// contiguous split of [0, n): sizes differ by at most one, earlier ranks take the extra (JTM.scala:47-52)
static inline void jtm_shard_range(int64_t n, int r, int W, int64_t *lo, int64_t *hi) {
  const int64_t base = n / W, rem = n % W;
  *lo = (int64_t)r * base + std::min<int64_t>(r, rem);
  *hi = *lo + base + (r < rem ? 1 : 0);
}

// itemSequenceMap of the catalogue, kept on the device for the gap steps of one JTM.optimize (TreeLearning.scala:34-46 builds it once
// per run too); n_items == 0 drops it.  _range: row_off describes ALL items (the re-balance and the exchange need every item's
// bookkeeping), but only the rows of the items [i_lo, i_hi) go up — the range this rank scores in a sharded run (dm_jtm_shard_range):
// the upload, the row arrays and the per-row history codes shrink with the number of ranks.  row_item_ids is the full array either way
// (indexed by absolute row number); rows outside the range are never read.
int dm_jtm_shard_range(int64_t n_items, int rank, int nranks, int64_t *i_lo, int64_t *i_hi) {
  if (n_items < 0 || nranks < 1 || rank < 0 || rank >= nranks || !i_lo || !i_hi) return DM_ERR_INVALID;
  jtm_shard_range(n_items, rank, nranks, i_lo, i_hi);
  return DM_OK;
}

int dm_jtm_cache_rows_range(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, int64_t n_items, int L, int64_t i_lo, int64_t i_hi) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  jtm_drop_cache(h);
  if (n_items == 0) return DM_OK;
  if (!row_off || !row_item_ids || n_items < 0 || L <= 0 || L > jtm_max_L(h->scorer_kind) || n_items >= ((int64_t)1 << 31) || i_lo < 0 || i_hi < i_lo || i_hi > n_items)
    return fail(h, DM_ERR_INVALID, "dm_jtm_cache_rows: bad arguments");
  for (int64_t i = 0; i < n_items; i++)
    if (row_off[i + 1] < row_off[i]) return fail(h, DM_ERR_INVALID, "dm_jtm_cache_rows: row_off must be non-decreasing");
  if (row_off[0] != 0) return fail(h, DM_ERR_INVALID, "dm_jtm_cache_rows: row_off[0] must be 0");
  const int64_t Rb = row_off[i_lo], R = row_off[i_hi] - Rb;
  h->jtm_off.assign(row_off, row_off + n_items + 1);
  std::vector<int32_t> ritem((size_t)(R > 0 ? R : 1));
  for (int64_t i = i_lo; i < i_hi; i++)
    for (int64_t r = row_off[i]; r < row_off[i + 1]; r++) ritem[(size_t)(r - Rb)] = (int32_t)i;
  ALLOC(h, h->d_jtm_off, (size_t)(n_items + 1) * 8);
  ALLOC(h, h->d_jtm_ritem, ritem.size() * 4);
  ALLOC(h, h->d_jtm_rids, (size_t)(R > 0 ? R : 1) * L * 4);
  HIPCHK(h, hipMemcpy(h->d_jtm_off, row_off, (size_t)(n_items + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_jtm_ritem, ritem.data(), ritem.size() * 4, hipMemcpyHostToDevice));
  if (R > 0) HIPCHK(h, hipMemcpy(h->d_jtm_rids, row_item_ids + Rb * L, (size_t)R * L * 4, hipMemcpyHostToDevice));
  h->jtm_L = L; h->jtm_i_lo = i_lo; h->jtm_i_hi = i_hi; h->jtm_R_base = Rb;
  return DM_OK;
}

int dm_jtm_cache_rows(dm_handle_t h, const int64_t *row_off, const int32_t *row_item_ids, int64_t n_items, int L) {
  return dm_jtm_cache_rows_range(h, row_off, row_item_ids, n_items, L, 0, n_items < 0 ? 0 : n_items);
}

// dm_jtm_child_weights for the items [i_lo, i_lo + n_items) of the cached catalogue: item_node / weights are indexed from i_lo
static int jtm_child_weights_cached_impl(dm_ctx *h, int scorer, const int32_t *item_node, int64_t i_lo, int64_t n_items, int old_level, int level,
                                         int hierarchical, int min_level, int use_mask, float *weights) {
  if (h->jtm_off.empty()) return fail(h, DM_ERR_STATE, "dm_jtm_child_weights_cached: call dm_jtm_cache_rows first");
  if (i_lo < 0 || n_items < 0 || i_lo + n_items > (int64_t)h->jtm_off.size() - 1) return fail(h, DM_ERR_INVALID, "dm_jtm_child_weights_cached: item range outside the cached catalogue");
  return jtm_child_weights_impl(h, scorer, h->jtm_off.data() + i_lo, nullptr, true, i_lo, item_node, n_items, h->jtm_L, old_level, level, hierarchical,
                                min_level, use_mask, weights);
}
int dm_jtm_child_weights_cached(dm_handle_t h, const int32_t *item_node, int64_t i_lo, int64_t n_items, int old_level, int level,
                                int hierarchical, int min_level, int use_mask, float *weights) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  DM_DIN_ONLY(h, "dm_jtm_child_weights_cached");
  return jtm_child_weights_cached_impl(h, DM_KIND_DIN, item_node, i_lo, n_items, old_level, level, hierarchical, min_level, use_mask, weights);
}
int dm_deepfm_jtm_child_weights_cached(dm_handle_t h, const int32_t *item_node, int64_t i_lo, int64_t n_items, int old_level, int level,
                                       int hierarchical, int min_level, int use_mask, float *weights) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  const int rc = dfm_jtm_enter(h, "dm_deepfm_jtm_child_weights_cached", use_mask, h->jtm_off.empty() ? -1 : h->jtm_L);
  if (rc != DM_OK) return rc;
  return jtm_child_weights_cached_impl(h, DM_KIND_DEEPFM, item_node, i_lo, n_items, old_level, level, hierarchical, min_level, 0, weights);
}

static int java_double_compare_h(double x, double y) {
  if (x < y) return -1;
  if (x > y) return 1;
  int64_t a, b;
  if (x != x) a = 0x7ff8000000000000LL; else memcpy(&a, &x, 8);
  if (y != y) b = 0x7ff8000000000000LL; else memcpy(&b, &y, 8);
  return a == b ? 0 : (a < b ? -1 : 1);
}
static inline int java_compare_w(float x, float y) { return java_float_compare_h(x, y); }
static inline int java_compare_w(double x, double y) { return java_double_compare_h(x, y); }

// sortNodeWeights + first choice + reBalance for the items of one parent; W = float (JTM, TreeLearning.scala:137-150,
// 217-265) or double (OTM, otm/src/main/scala/com/mass/otm/tree/TreeConstruction.scala:180-213,304-352: the same logic)
// Sort key of the greedy cut: (moved out of its old subtree?, weight descending by Float / Double.compare, list position) —
// the position makes the order total, i.e. the order a stable sort by the first two components produces.
struct JtmKeyF {                    // float weights: one 64-bit word
  uint64_t v;
  static JtmKeyF make(int moved, float w, uint32_t pos) {
    uint32_t b;
    if (w != w) b = 0x7fc00000u; else memcpy(&b, &w, 4);
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);          // Float.compare order, ascending
    return JtmKeyF{((uint64_t)(moved & 1) << 63) | ((uint64_t)(~asc) << 31) | pos};
  }
  uint32_t pos() const { return (uint32_t)(v & 0x7fffffffu); }
  bool operator<(const JtmKeyF &o) const { return v < o.v; }
};
struct JtmKeyD {                    // double weights (OTM)
  uint32_t moved, p; uint64_t k;
  static JtmKeyD make(int moved, double w, uint32_t pos) {
    uint64_t b;
    if (w != w) b = 0x7ff8000000000000ull; else memcpy(&b, &w, 8);
    const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return JtmKeyD{(uint32_t)(moved & 1), pos, ~asc};
  }
  uint32_t pos() const { return p; }
  bool operator<(const JtmKeyD &o) const { return moved != o.moved ? moved < o.moved : (k != o.k ? k < o.k : p < o.p); }
};
template <typename W> struct JtmKeyOf;
template <> struct JtmKeyOf<float> { typedef JtmKeyF type; };
template <> struct JtmKeyOf<double> { typedef JtmKeyD type; };

template <typename W>
struct JtmInfo { int64_t it; W w; int next; };
template <typename W>
struct JtmScratch {                     // reused across the parents one thread handles: no allocation per parent
  std::vector<int32_t> cand;
  std::vector<std::vector<JtmInfo<W>>> lst;
  std::vector<JtmInfo<W>> sorted;
  std::vector<typename JtmKeyOf<W>::type> keys;
  std::vector<char> present, processed;
};

// fn(lo, hi) over [0, n) on up to `threads` host threads (contiguous ranges; the caller's work items are independent)
template <typename F>
static void jtm_parallel_ranges(int64_t n, int threads, F fn) {
  if (threads <= 1 || n < (int64_t)threads * 4096) { fn((int64_t)0, n); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) pool.emplace_back([=]() { fn(n * t / threads, n * (t + 1) / threads); });
  for (auto &t : pool) t.join();
}

// std::stable_sort on `threads` host threads: sorted runs, then rounds of pairwise std::inplace_merge (both stable, so the
// result is the one stable order — identical to the single-threaded sort)
template <typename It, typename Cmp>
static void jtm_parallel_stable_sort(It first, It last, Cmp cmp, int threads) {
  const int64_t n = last - first;
  if (threads <= 1 || n < (int64_t)1 << 17) { std::stable_sort(first, last, cmp); return; }
  int runs = 1;
  while (runs * 2 <= threads) runs *= 2;
  std::vector<int64_t> cut(runs + 1);
  for (int r = 0; r <= runs; r++) cut[r] = n * r / runs;
  {
    std::vector<std::thread> pool;
    for (int r = 0; r < runs; r++) pool.emplace_back([=, &cut]() { std::stable_sort(first + cut[r], first + cut[r + 1], cmp); });
    for (auto &t : pool) t.join();
  }
  for (int width = 1; width < runs; width *= 2) {
    std::vector<std::thread> pool;
    for (int r = 0; r + width < runs; r += 2 * width)
      pool.emplace_back([=, &cut]() { std::inplace_merge(first + cut[r], first + cut[r + width], first + cut[std::min(r + 2 * width, runs)], cmp); });
    for (auto &t : pool) t.join();
  }
}

// fn(t, lo, hi) for thread t over a contiguous split of [0, n)
template <typename F>
static void jtm_parallel_ranges_t(int64_t n, int threads, F fn) {
  if (threads <= 1 || n < (int64_t)threads * 4096) { fn(0, (int64_t)0, n); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) pool.emplace_back([=]() { fn(t, n * t / threads, n * (t + 1) / threads); });
  for (auto &t : pool) t.join();
}

// `threads` > 1: this parent is one of a few very large ones (top levels of the tree) and may use that many host threads itself
template <typename W>
static int jtm_rebalance_t(dm_ctx *h, const W *weights, const int32_t *old_node, int64_t n, int32_t node, int old_level,
                           int level, int max_assign, int32_t *out_node, const char *who, JtmScratch<W> *scr = nullptr,
                           int threads = 1) {
  if (!weights || !old_node || !out_node || n < 0 || level <= old_level || level - old_level > 8 || max_assign < 0)
    return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  if (level > JTM_MAX_LEVEL) return jtm_level_refused(h, level, who);
  if (n >= ((int64_t)1 << 31)) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 items under one parent");
  typedef JtmInfo<W> Info;
  typedef typename JtmKeyOf<W>::type Key;
  JtmScratch<W> local;
  JtmScratch<W> &S = scr ? *scr : local;
  const int nchild = 1 << (level - old_level);
  const int64_t first = ((int64_t)node << (level - old_level)) + nchild - 1;
  std::vector<int32_t> &cand = S.cand;
  cand.resize((size_t)n * nchild);
  jtm_parallel_ranges(n, threads, [&cand, weights, nchild](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; i++) {     // sortNodeWeights: stable, descending by Float/Double.compare
      int32_t *c = &cand[(size_t)i * nchild];
      for (int k = 0; k < nchild; k++) c[k] = k;
      const W *w = weights + i * nchild;
      for (int a = 1; a < nchild; a++) {  // stable insertion sort (nchild <= 256, usually 4)
        const int32_t v = c[a];
        int bpos = a - 1;
        while (bpos >= 0 && java_compare_w(w[c[bpos]], w[v]) < 0) { c[bpos + 1] = c[bpos]; bpos--; }
        c[bpos + 1] = v;
      }
    }
  });
  std::vector<std::vector<Info>> &lst = S.lst;
  if ((int)lst.size() < nchild) lst.resize(nchild);
  for (int c = 0; c < nchild; c++) lst[c].clear();
  S.present.assign(nchild, 0); S.processed.assign(nchild, 0);
  std::vector<char> &present = S.present, &processed = S.processed;
  // first choice of every item, in item order (TreeLearning.scala:66-71); large parents: counted and filled on all threads
  {
    const int T = (threads > 1 && n >= (int64_t)threads * 4096) ? threads : 1;
    std::vector<int64_t> cnt((size_t)T * nchild, 0);
    jtm_parallel_ranges_t(n, T, [&](int t, int64_t lo, int64_t hi) {
      int64_t *c_ = &cnt[(size_t)t * nchild];
      for (int64_t i = lo; i < hi; i++) c_[cand[(size_t)i * nchild]]++;
    });
    std::vector<int64_t> offs((size_t)T * nchild);
    for (int c = 0; c < nchild; c++) {
      int64_t acc = 0;
      for (int t = 0; t < T; t++) { offs[(size_t)t * nchild + c] = acc; acc += cnt[(size_t)t * nchild + c]; }
      lst[c].resize((size_t)acc);
      present[c] = acc > 0;
    }
    jtm_parallel_ranges_t(n, T, [&](int t, int64_t lo, int64_t hi) {
      std::vector<int64_t> o(offs.begin() + (size_t)t * nchild, offs.begin() + (size_t)(t + 1) * nchild);
      for (int64_t i = lo; i < hi; i++) { const int c = cand[(size_t)i * nchild]; lst[c][(size_t)o[c]++] = Info{i, weights[i * nchild + c], 1}; }
    });
  }
  for (;;) {
    int64_t best = -1; int bc = 0;
    for (int c = 0; c < nchild; c++) {          // getMaxNode: first maximum in child order
      int64_t v = (!processed[c] && present[c]) ? (int64_t)lst[c].size() : -1;
      if (c == 0 || v > best) { best = v; bc = c; }
    }
    if (best <= max_assign) break;
    processed[bc] = 1;
    const int32_t this_code = (int32_t)(first + bc);
    // The reference sorts the whole list stably by (moved?, -weight) and cuts it at max_assign (TreeLearning.scala:240-246).  The
    // KEPT part belongs to a processed child from here on: it is never sorted or scanned in order again, so only its membership
    // matters; the overflow part is re-distributed in sorted order.  With the list position as the last key component the order
    // is total, so the same two sets come out of a SELECTION of the max_assign-th key plus a sort of the overflow alone (near the
    // root: millions of items per child, a small overflow).
    std::vector<Info> &cur = lst[bc];
    const int64_t m = (int64_t)cur.size();
    std::vector<Key> &keys = S.keys;
    keys.resize((size_t)m);
    const Info *cp = cur.data();
    jtm_parallel_ranges(m, threads, [&keys, cp, old_node, this_code](int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; i++) keys[(size_t)i] = Key::make(old_node[cp[i].it] != this_code, cp[i].w, (uint32_t)i);
    });
    std::nth_element(keys.begin(), keys.begin() + max_assign, keys.end());
    jtm_parallel_stable_sort(keys.begin() + max_assign, keys.end(), [](const Key &x, const Key &y) { return x < y; }, threads);
    std::vector<Info> &kept = S.sorted;
    kept.resize((size_t)max_assign);
    jtm_parallel_ranges((int64_t)max_assign, threads, [&kept, &keys, cp](int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; i++) kept[(size_t)i] = cp[keys[(size_t)i].pos()];
    });
    for (int64_t i = max_assign; i < m; i++) {
      const Info it = cp[keys[(size_t)i].pos()];
      for (int k = it.next; k < nchild; k++) {
        const int c = cand[(size_t)it.it * nchild + k];
        if (!processed[c]) { lst[c].push_back({it.it, weights[it.it * nchild + c], k + 1}); present[c] = 1; break; }
      }
    }
    cur.swap(kept);
  }
  if (threads > 1 && n >= (int64_t)threads * 4096) {
    jtm_parallel_ranges(n, threads, [out_node](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; i++) out_node[i] = -1; });
    for (int c = 0; c < nchild; c++) {
      const Info *lp = lst[c].data();
      const int32_t code = (int32_t)(first + c);
      jtm_parallel_ranges((int64_t)lst[c].size(), threads, [out_node, lp, code](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; i++) out_node[lp[i].it] = code; });
    }
  } else {
    for (int64_t i = 0; i < n; i++) out_node[i] = -1;
    for (int c = 0; c < nchild; c++)
      for (const Info &it : lst[c]) out_node[it.it] = (int32_t)(first + c);
  }
  return DM_OK;
}

int dm_jtm_rebalance(dm_handle_t h, const float *weights, const int32_t *old_node, int64_t n, int32_t node, int old_level,
                     int level, int max_assign, int32_t *out_node) {
  if (!h) return DM_ERR_INVALID;
  return jtm_rebalance_t<float>(h, weights, old_node, n, node, old_level, level, max_assign, out_node, "dm_jtm_rebalance");
}

// getChildrenProjection for EVERY parent node of a level in one call (JTM.optimize's loop over currentNodes, JTM.scala:36-70):
// items are grouped by the node they sit in (item_node), in the order given; out_node[i] = new child code, or the old
// node when the greedy loop drops the item (projections fold with `++`, :72).  Parents are independent.
template <typename W>
static int jtm_rebalance_all_t(dm_ctx *h, const W *weights, const int32_t *old_node, const int32_t *item_node, int64_t n,
                               int old_level, int level, int max_assign, int32_t *out_node, const char *who) {
  if (!weights || !old_node || !item_node || !out_node || n < 0 || level <= old_level || level - old_level > 8 || max_assign < 0)
    return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  if (level > JTM_MAX_LEVEL) return jtm_level_refused(h, level, who);
  const int nchild = 1 << (level - old_level);
  // stable grouping by node: the nodes of a level form a contiguous code range -> counting sort
  std::vector<int64_t> order((size_t)n);
  {
    const int64_t lo = ((int64_t)1 << old_level) - 1, span = (int64_t)1 << old_level;
    bool in_range = true;
    for (int64_t i = 0; i < n && in_range; i++) in_range = item_node[i] >= lo && item_node[i] < lo + span;
    if (in_range && span <= ((int64_t)1 << 28)) {
      std::vector<int64_t> cnt((size_t)span + 1, 0);
      for (int64_t i = 0; i < n; i++) cnt[(size_t)(item_node[i] - lo) + 1]++;
      for (int64_t k = 0; k < span; k++) cnt[(size_t)k + 1] += cnt[(size_t)k];
      for (int64_t i = 0; i < n; i++) order[(size_t)cnt[(size_t)(item_node[i] - lo)]++] = i;
    } else {
      for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
      std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return item_node[a] < item_node[b]; });
    }
  }
  // group boundaries, then the (independent) parents are spread over host threads
  std::vector<int64_t> starts;
  for (int64_t a = 0; a < n;) {
    starts.push_back(a);
    int64_t b = a;
    while (b < n && item_node[order[(size_t)b]] == item_node[order[(size_t)a]]) b++;
    a = b;
  }
  starts.push_back(n);
  const int64_t ng = (int64_t)starts.size() - 1;
  unsigned nthreads = std::thread::hardware_concurrency();
  if (nthreads > 16) nthreads = 16;
  if (nthreads < 1 || n < 20000) nthreads = 1;
  std::atomic<int64_t> next_group(0);
  std::atomic<int> err(DM_OK);
  // groups are handed out in blocks: 64 at a time when there are millions of parents, one at a time near the root, where
  // the few huge parents also get the idle threads for their own sorts
  int64_t block = ng / ((int64_t)nthreads * 8);
  if (block > 64) block = 64;
  if (block < 1) block = 1;
  const int inner = ng < (int64_t)nthreads ? (int)(nthreads / (ng > 0 ? ng : 1)) : 1;
  if ((int64_t)nthreads > ng && ng > 0 && n >= 20000) nthreads = (unsigned)ng;
  auto worker = [&]() {
    std::vector<W> gw;
    std::vector<int32_t> go, gout;
    JtmScratch<W> scratch;
    for (;;) {
      const int64_t g0 = next_group.fetch_add(block);
      if (g0 >= ng) break;
      for (int64_t g = g0; g < g0 + block && g < ng; g++) {
        const int64_t a = starts[(size_t)g], m = starts[(size_t)g + 1] - a;
        {   // items that do not sit in a node of old_level keep their entry: JTM.scala:36 only visits getAllNodesAtLevel(oldLevel)
          const int64_t nd = item_node[order[(size_t)a]], lo_ = ((int64_t)1 << old_level) - 1;
          if (nd < lo_ || nd - lo_ >= ((int64_t)1 << old_level)) {
            for (int64_t k = 0; k < m; k++) out_node[order[(size_t)(a + k)]] = item_node[order[(size_t)(a + k)]];
            continue;
          }
        }
        gw.resize((size_t)m * nchild); go.resize((size_t)m); gout.resize((size_t)m);
        for (int64_t k = 0; k < m; k++) {
          const int64_t i = order[(size_t)(a + k)];
          memcpy(&gw[(size_t)k * nchild], weights + i * nchild, sizeof(W) * nchild);
          go[(size_t)k] = old_node[i];
        }
        const int rc = jtm_rebalance_t<W>(nullptr, gw.data(), go.data(), m, item_node[order[(size_t)a]], old_level, level, max_assign, gout.data(), who, &scratch, inner);
        if (rc != DM_OK) { err.store(rc); return; }
        for (int64_t k = 0; k < m; k++) {
          const int64_t i = order[(size_t)(a + k)];
          out_node[i] = gout[(size_t)k] >= 0 ? gout[(size_t)k] : item_node[i];
        }
      }
    }
  };
  if (nthreads == 1) worker();
  else {
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads; t++) pool.emplace_back(worker);
    for (auto &t : pool) t.join();
  }
  if (err.load() != DM_OK) return fail(h, err.load(), std::string(who) + ": re-balance failed");
  return DM_OK;
}

// the device version (jtm_rebalance_dev.hip.inc) on host arrays: upload, run, download.  DM_JTM_REBALANCE=host keeps the host logic.
static bool jtm_rebalance_on_device(const dm_ctx *h, int64_t n, int old_level, int level) {
  const char *e = env_str("DM_JTM_REBALANCE");
  if (e && !strcmp(e, "host")) return false;
  (void)h;
  return n >= 4096 && level - old_level <= 8 && old_level <= 24 && n < ((int64_t)1 << 31);
}
// upload, device rounds, download (W = float: JTM; double: OTM's TreeConstruction); DM_ERR_UNSUPPORTED -> the caller's host logic
template <typename W>
static int jtm_rebalance_all_staged(dm_ctx *h, const W *weights, const int32_t *old_node, const int32_t *item_node, int64_t n, int old_level,
                                    int level, int max_assign, int32_t *out_node, const char *who) {
  if (level > JTM_MAX_LEVEL) return jtm_level_refused(h, level, who);
  HIPCHK(h, hipSetDevice(h->device));
  const int C = 1 << (level - old_level);
  DevTemps t(h);
  char *A = nullptr;
  const size_t bw = DevArena::up((size_t)n * C * sizeof(W)), bi = DevArena::up((size_t)n * 4);
  int rc = t.alloc(A, bw + 3 * bi);
  if (rc != DM_OK) return rc;
  W *d_w = (W *)A; int32_t *d_old = (int32_t *)(A + bw), *d_node = (int32_t *)(A + bw + bi), *d_out = (int32_t *)(A + bw + 2 * bi);
  if (hipMemcpyAsync(d_w, weights, (size_t)n * C * sizeof(W), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(d_old, old_node, (size_t)n * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(d_node, item_node, (size_t)n * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess)
    return fail(h, DM_ERR_HIP, std::string(who) + ": upload failed");
  if ((rc = jtm_rebalance_all_dev<W>(h, d_w, d_old, d_node, n, old_level, level, max_assign, d_out)) != DM_OK) return rc;
  if (hipMemcpy(out_node, d_out, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DM_ERR_HIP, std::string(who) + ": download failed");
  return DM_OK;
}
int dm_jtm_rebalance_all(dm_handle_t h, const float *weights, const int32_t *old_node, const int32_t *item_node, int64_t n,
                         int old_level, int level, int max_assign, int32_t *out_node) {
  if (!h) return DM_ERR_INVALID;
  if (weights && old_node && item_node && out_node && level > old_level && max_assign >= 0 && jtm_rebalance_on_device(h, n, old_level, level)) {
    const int rc = jtm_rebalance_all_staged<float>(h, weights, old_node, item_node, n, old_level, level, max_assign, out_node, "dm_jtm_rebalance_all");
    if (rc != DM_ERR_UNSUPPORTED) return rc;
  }
  return jtm_rebalance_all_t<float>(h, weights, old_node, item_node, n, old_level, level, max_assign, out_node, "dm_jtm_rebalance_all");
}

// One gap step of JTM.optimize over the WHOLE cached catalogue (JTM.scala:36-72) without a host round trip in between: child
// weights of every item (dm_jtm_child_weights_cached) -> greedy re-balance of every parent node (dm_jtm_rebalance_all) with the
// [n x 2^gap] weight matrix kept in HBM.  item_node / old_node in, out_node out (host, [n_items] each).
static int jtm_step_cached_impl(dm_ctx *h, int scorer, const int32_t *item_node, const int32_t *old_node, int64_t n_items, int old_level, int level,
                                int hierarchical, int min_level, int use_mask, int max_assign, int32_t *out_node) {
  if (h->jtm_off.empty()) return fail(h, DM_ERR_STATE, "dm_jtm_step_cached: call dm_jtm_cache_rows first");
  if (!item_node || !old_node || !out_node || n_items != (int64_t)h->jtm_off.size() - 1 || level <= old_level || level - old_level > 8 || max_assign < 0)
    return fail(h, DM_ERR_INVALID, "dm_jtm_step_cached: bad arguments (n_items must be the cached catalogue)");
  if (n_items == 0) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const int C = 1 << (level - old_level);
  DevTemps t(h);
  char *A = nullptr;
  const size_t bw = DevArena::up((size_t)n_items * C * 4), bi = DevArena::up((size_t)n_items * 4);
  int rc = t.alloc(A, bw + 3 * bi);
  if (rc != DM_OK) return rc;
  float *d_w = (float *)A; int32_t *d_old = (int32_t *)(A + bw), *d_node = (int32_t *)(A + bw + bi), *d_out = (int32_t *)(A + bw + 2 * bi);
  if (hipMemcpyAsync(d_old, old_node, (size_t)n_items * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(d_node, item_node, (size_t)n_items * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess)
    rc = fail(h, DM_ERR_HIP, "dm_jtm_step_cached: upload failed");
  const auto t0 = std::chrono::steady_clock::now();
  if (rc == DM_OK) rc = jtm_child_weights_impl(h, scorer, h->jtm_off.data(), nullptr, true, 0, nullptr, n_items, h->jtm_L, old_level, level, hierarchical,
                                               min_level, use_mask, nullptr, d_node, d_w);
  const auto t1 = std::chrono::steady_clock::now();       // the scoring pass ends with a stream synchronise
  struct Tm { dm_ctx *h; std::chrono::steady_clock::time_point t0, t1; ~Tm() {
    h->jtm_score_s = std::chrono::duration<double>(t1 - t0).count();
    h->jtm_rebal_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count(); } } tm_{h, t0, t1};
  if (rc == DM_OK) {
    rc = jtm_rebalance_on_device(h, n_items, old_level, level)
             ? jtm_rebalance_all_dev(h, d_w, d_old, d_node, n_items, old_level, level, max_assign, d_out) : DM_ERR_UNSUPPORTED;
    if (rc == DM_OK) {
      if (hipMemcpy(out_node, d_out, (size_t)n_items * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DM_ERR_HIP, "dm_jtm_step_cached: download failed");
    } else if (rc == DM_ERR_UNSUPPORTED) {       // shapes the device re-balance does not cover: the host logic on downloaded weights
      std::vector<float> w((size_t)n_items * C);
      if (hipMemcpy(w.data(), d_w, w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DM_ERR_HIP, "dm_jtm_step_cached: download failed");
      else rc = jtm_rebalance_all_t<float>(h, w.data(), old_node, item_node, n_items, old_level, level, max_assign, out_node, "dm_jtm_step_cached");
    }
  }
  return rc;
}
int dm_jtm_step_cached(dm_handle_t h, const int32_t *item_node, const int32_t *old_node, int64_t n_items, int old_level, int level,
                       int hierarchical, int min_level, int use_mask, int max_assign, int32_t *out_node) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  DM_DIN_ONLY(h, "dm_jtm_step_cached");
  return jtm_step_cached_impl(h, DM_KIND_DIN, item_node, old_node, n_items, old_level, level, hierarchical, min_level, use_mask, max_assign, out_node);
}
int dm_deepfm_jtm_step_cached(dm_handle_t h, const int32_t *item_node, const int32_t *old_node, int64_t n_items, int old_level, int level,
                              int hierarchical, int min_level, int use_mask, int max_assign, int32_t *out_node) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  const int rc = dfm_jtm_enter(h, "dm_deepfm_jtm_step_cached", use_mask, h->jtm_off.empty() ? -1 : h->jtm_L);
  if (rc != DM_OK) return rc;
  return jtm_step_cached_impl(h, DM_KIND_DEEPFM, item_node, old_node, n_items, old_level, level, hierarchical, min_level, 0, max_assign, out_node);
}

// JTMTree.getAncestorAtLevel (jtm/.../tree/JTMTree.scala:36-43) of every item's current leaf code
__global__ void jtm_ancestor_kernel(const int32_t *item_code, int64_t n, int level, int32_t *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t c1 = (uint32_t)item_code[i] + 1u;             // heap code + 1 = 1 b_1 b_2 ...: bit length = level + 1
    const int lv = 31 - __clz((int)c1);
    out[i] = (int32_t)((c1 >> (lv > level ? lv - level : 0)) - 1u);
  }
}

// seconds the last dm_jtm_step_cached spent scoring / re-balancing (incl. its copies): measurement
int dm_jtm_last_step_seconds(dm_handle_t h, double *scoring_s, double *rebalance_s) {
  if (!h || !scoring_s || !rebalance_s) return DM_ERR_INVALID;
  *scoring_s = h->jtm_score_s; *rebalance_s = h->jtm_rebal_s;
  return DM_OK;
}

int dm_otm_rebalance_all(dm_handle_t h, const double *weights, const int32_t *old_node, const int32_t *item_node, int64_t n,
                         int old_level, int level, int max_assign, int32_t *out_node) {
  if (!h) return DM_ERR_INVALID;
  // TreeConstruction.reBalance (otm/.../tree/TreeConstruction.scala:304-352) for every parent of the level on the device, like JTM's
  if (weights && old_node && item_node && out_node && level > old_level && max_assign >= 0 && jtm_rebalance_on_device(h, n, old_level, level)) {
    const int rc = jtm_rebalance_all_staged<double>(h, weights, old_node, item_node, n, old_level, level, max_assign, out_node, "dm_otm_rebalance_all");
    if (rc != DM_ERR_UNSUPPORTED) return rc;
  }
  return jtm_rebalance_all_t<double>(h, weights, old_node, item_node, n, old_level, level, max_assign, out_node, "dm_otm_rebalance_all");
}

int dm_otm_rebalance(dm_handle_t h, const double *weights, const int32_t *old_node, int64_t n, int32_t node, int old_level,
                     int level, int max_assign, int32_t *out_node) {
  if (!h) return DM_ERR_INVALID;
  return jtm_rebalance_t<double>(h, weights, old_node, n, node, old_level, level, max_assign, out_node, "dm_otm_rebalance");
}

// OTM twin of the scoring (TreeConstruction.aggregateWeights / buildFeatures, TreeConstruction.scala:194-232): the item
// sequences already hold NODE ids (-1 = padding), the model runs in the loaded dtype (the reference's is fp64) and the
// per-(item, node) Tensor.sum and the chain accumulation are double.
int dm_otm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_codes, const int32_t *item_node,
                         int64_t n_items, int L, int old_level, int level, int use_mask, double *weights) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, "dm_otm_child_weights: weights must be loaded first");
  DM_DIN_ONLY(h, "dm_otm_child_weights");
  if (!row_off || !item_node || !weights || n_items < 0 || L <= 0 || L > 32 || level <= old_level || level - old_level > 8)
    return fail(h, DM_ERR_INVALID, "dm_otm_child_weights: bad arguments");
  if ((((int64_t)1) << (level + 1)) - 1 > h->num_index) return fail(h, DM_ERR_INDEX, "dm_otm_child_weights: level exceeds the embedding table");
  HIPCHK(h, hipSetDevice(h->device));
  const int gap = level - old_level, nchild = 1 << gap, nchain = (2 << gap) - 2;
  const bool f64 = h->dtype == DM_F64;
  const size_t esz = f64 ? 8 : 4;
  const int64_t max_pairs = jtm_max_pairs((int64_t)4 << 20);
  const int64_t all_pairs = n_items > 0 ? (row_off[n_items] - row_off[0]) * nchain : 0;      // every chunk takes the kernel of the whole call
  std::vector<int32_t> codes, seqs;
  std::vector<unsigned> rmask;
  std::vector<double> logits;
  std::vector<float> logits32;
  int32_t *d_codes = nullptr, *d_seqs = nullptr;
  unsigned *d_mask = nullptr;
  void *d_out = nullptr;
  size_t cap_pairs = 0;
  DevTemps t(h);
  int rc = DM_OK;
  for (int64_t i0 = 0; i0 < n_items;) {
    int64_t i1 = i0, pairs = 0;
    while (i1 < n_items) {
      const int64_t add = (row_off[i1 + 1] - row_off[i1]) * nchain;
      if (pairs > 0 && pairs + add > max_pairs) break;
      pairs += add; i1++;
    }
    codes.resize(pairs); seqs.resize((size_t)pairs * L); rmask.resize(pairs); logits.resize(pairs);
    int64_t q = 0;                     // pair order: item, chain node (level old+1 .. level, left to right), row
    for (int64_t i = i0; i < i1 && rc == DM_OK; i++) {
      const int64_t nr = row_off[i + 1] - row_off[i];
      for (int d = 1; d <= gap; d++) {
        const int64_t first = ((int64_t)item_node[i] << d) + (1 << d) - 1;
        for (int c = 0; c < (1 << d); c++)
          for (int64_t r = 0; r < nr; r++, q++) {
            codes[q] = (int32_t)(first + c);
            unsigned m = 0;
            const int32_t *ids = row_codes + (row_off[i] + r) * L;
            for (int j = 0; j < L; j++) {
              const int32_t cd = ids[j];
              if (cd == -1) m |= 1u << j;                       // buildFeatures: masks = positions holding paddingIdx
              else if (cd < 0 || cd >= h->num_index) rc = fail(h, DM_ERR_INDEX, "dm_otm_child_weights: history node outside the embedding table");
              seqs[(size_t)q * L + j] = cd;
            }
            rmask[q] = use_mask ? m : 0u;
          }
      }
    }
    if (rc != DM_OK) return rc;
    if (pairs > 0) {
      if ((size_t)pairs > cap_pairs) {
        t.drop(d_codes); t.drop(d_seqs); t.drop(d_mask); t.drop(d_out);
        cap_pairs = (size_t)pairs;
        if ((rc = t.alloc(d_codes, cap_pairs * 4)) != DM_OK) return rc;
        if ((rc = t.alloc(d_seqs, cap_pairs * L * 4)) != DM_OK) return rc;
        if ((rc = t.alloc(d_mask, cap_pairs * 4)) != DM_OK) return rc;
        if ((rc = t.alloc(d_out, cap_pairs * esz)) != DM_OK) return rc;
      }
      hipError_t e = hipMemcpyAsync(d_codes, codes.data(), (size_t)pairs * 4, hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(d_seqs, seqs.data(), (size_t)pairs * L * 4, hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(d_mask, rmask.data(), (size_t)pairs * 4, hipMemcpyHostToDevice, h->stream);
      if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_otm_child_weights: upload failed");
      if (f64) rc = din_forward_t<double>(h, d_codes, d_seqs, d_mask, pairs, L, (double *)d_out, all_pairs);
      else rc = L <= DM_MAXL ? din_rows_dev(h, d_codes, d_seqs, d_mask, pairs, L, (float *)d_out)
                             : din_forward_t<float>(h, d_codes, d_seqs, d_mask, pairs, L, (float *)d_out);
      if (rc != DM_OK) return rc;
      if (f64) e = hipMemcpyAsync(logits.data(), d_out, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream);
      else { logits32.resize(pairs); e = hipMemcpyAsync(logits32.data(), d_out, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream); }
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e != hipSuccess) return fail(h, DM_ERR_HIP, std::string("dm_otm_child_weights: ") + hipGetErrorString(e));
      if (!f64) for (int64_t k = 0; k < pairs; k++) logits[k] = (double)logits32[k];
    }
    q = 0;
    std::vector<double> score(nchain);
    for (int64_t i = i0; i < i1; i++) {
      const int64_t nr = row_off[i + 1] - row_off[i];
      for (int x = 0; x < nchain; x++) {
        double s = 0.0;
        for (int64_t r = 0; r < nr; r++) s += logits[q++];          // Tensor.sum() in row order
        score[x] = s;
      }
      for (int c = 0; c < nchild; c++) {
        if (nr == 0) { weights[i * nchild + c] = -1e6; continue; }   // never appeared as a target (:201)
        double w = 0.0;
        int idx = c;
        for (int d = gap; d >= 1; d--) { w += score[(1 << d) - 2 + idx]; idx >>= 1; }   // child -> parent chain (:205-210)
        weights[i * nchild + c] = w;
      }
    }
    i0 = i1;
  }
  return DM_OK;
}

// debug (not part of the public header): the two primitives of dev_sort.hip.inc on host arrays — upload, one call on the handle's stream
// with scratch of dev_sort_scratch_bytes, download — so that tests can hold them against numpy at sizes and bit ranges no caller reaches
// (tests/test_gpu_dev_sort.py).  Every device byte is a DevTemps temporary of the call.
extern "C" int dm_debug_sort_pairs(dm_handle_t h, uint64_t *keys, int32_t *vals, int64_t m, int begin_bit, int end_bit, int *where) {
  if (!h) return DM_ERR_INVALID;
  if (!keys || !vals || !where || m < 0 || m >= ((int64_t)1 << 31) || begin_bit < 0 || end_bit < begin_bit || end_bit > 64)
    return fail(h, DM_ERR_INVALID, "dm_debug_sort_pairs: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  DevTemps t(h);
  unsigned long long *k[2] = {nullptr, nullptr};
  int32_t *v[2] = {nullptr, nullptr};
  uint32_t *tmp = nullptr;
  int rc;
  for (int b = 0; b < 2; b++)
    if ((rc = t.alloc(k[b], (size_t)m * 8)) != DM_OK || (rc = t.alloc(v[b], (size_t)m * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(tmp, dev_sort_scratch_bytes(m))) != DM_OK) return rc;
  auto fin = [&](int r) { (void)hipStreamSynchronize(h->stream); return r; };       // nothing is freed under a running kernel
  if (m > 0 && (hipMemcpyAsync(k[0], keys, (size_t)m * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
                hipMemcpyAsync(v[0], vals, (size_t)m * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess))
    return fin(fail(h, DM_ERR_HIP, "dm_debug_sort_pairs: upload failed"));
  int wh = 0;
  const hipError_t e = dev_radix_sort_pairs(h->stream, k[0], v[0], k[1], v[1], m, begin_bit, end_bit, tmp, &wh);
  if (e != hipSuccess) return fin(fail(h, DM_ERR_HIP, std::string("dm_debug_sort_pairs: ") + hipGetErrorString(e)));
  if (m > 0 && (hipMemcpyAsync(keys, k[wh], (size_t)m * 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipMemcpyAsync(vals, v[wh], (size_t)m * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess))
    return fin(fail(h, DM_ERR_HIP, "dm_debug_sort_pairs: download failed"));
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, "dm_debug_sort_pairs: device pass failed");
  *where = wh;
  return DM_OK;
}

// in == NULL: the indices themselves; in2 / out2 (both or neither): a second array that rides along.  out / out2 receive *count elements.
extern "C" int dm_debug_select_flagged(dm_handle_t h, const int32_t *in, const uint64_t *in2, const uint8_t *flag, int64_t n, int32_t *out,
                                       uint64_t *out2, uint64_t *count) {
  if (!h) return DM_ERR_INVALID;
  if (!flag || !out || !count || (in2 && !out2) || n < 0 || n >= ((int64_t)1 << 31))
    return fail(h, DM_ERR_INVALID, "dm_debug_select_flagged: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  DevTemps t(h);
  int32_t *d_in = nullptr, *d_out = nullptr;
  unsigned long long *d_in2 = nullptr, *d_out2 = nullptr, *d_count = nullptr;
  uint8_t *d_flag = nullptr;
  uint32_t *tmp = nullptr;
  int rc;
  if ((rc = t.alloc(d_flag, (size_t)n)) != DM_OK || (rc = t.alloc(d_out, (size_t)n * 4)) != DM_OK || (rc = t.alloc(d_count, 8)) != DM_OK ||
      (rc = t.alloc(tmp, dev_sort_scratch_bytes(n))) != DM_OK)
    return rc;
  if (in && (rc = t.alloc(d_in, (size_t)n * 4)) != DM_OK) return rc;
  if (in2 && ((rc = t.alloc(d_in2, (size_t)n * 8)) != DM_OK || (rc = t.alloc(d_out2, (size_t)n * 8)) != DM_OK)) return rc;
  auto fin = [&](int r) { (void)hipStreamSynchronize(h->stream); return r; };
  if (n > 0 && (hipMemcpyAsync(d_flag, flag, (size_t)n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
                (in && hipMemcpyAsync(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
                (in2 && hipMemcpyAsync(d_in2, in2, (size_t)n * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess)))
    return fin(fail(h, DM_ERR_HIP, "dm_debug_select_flagged: upload failed"));
  const hipError_t e = in2 ? dev_select_flagged<int32_t, unsigned long long>(h->stream, d_in, d_in2, d_flag, d_out, d_out2, d_count, n, tmp)
                           : dev_select_flagged<int32_t>(h->stream, d_in, (const char *)nullptr, d_flag, d_out, (char *)nullptr, d_count, n, tmp);
  if (e != hipSuccess) return fin(fail(h, DM_ERR_HIP, std::string("dm_debug_select_flagged: ") + hipGetErrorString(e)));
  unsigned long long c = 0;
  if (hipMemcpyAsync(&c, d_count, 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
    return fin(fail(h, DM_ERR_HIP, "dm_debug_select_flagged: device pass failed"));
  if ((int64_t)c > n) return fail(h, DM_ERR_HIP, "dm_debug_select_flagged: internal count mismatch");
  if (c > 0 && (hipMemcpy(out, d_out, (size_t)c * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                (in2 && hipMemcpy(out2, d_out2, (size_t)c * 8, hipMemcpyDeviceToHost) != hipSuccess)))
    return fail(h, DM_ERR_HIP, "dm_debug_select_flagged: download failed");
  *count = c;
  return DM_OK;
}
