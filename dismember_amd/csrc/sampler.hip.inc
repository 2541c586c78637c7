// Level-wise negative sampling + batch expansion ON THE DEVICE (row A10).
// NegativeSampler.sample / sampleFromUniformDistribution / sampleFromCategoricalDistribution
// (tdm/src/main/scala/com/mass/tdm/utils/NegativeSampler.scala:76-158), TDMTree.pathNodes (tdm/.../tree/TDMTree.scala:59-78),
// MiniBatch.convert / transformWithMask (tdm/.../dataset/MiniBatch.scala:49-88,129-147).
//
// For every target item: its ancestors at levels start_level..its own level are the positives; per level neg_counts[level]
// DISTINCT existing codes of that level, != the positive, are drawn — uniformly, or (sample_with_probability) from the
// level's node-probability distribution with at most neg + sample_tolerance draws followed by a uniform fill that, as in the
// reference (:131-137), does not exclude the positive — and emitted after the positive in ASCENDING code order
// (BitSet.toList); labels 1, 0, .., 0; the user's history codes and mask are replicated per emitted node.
// The reference draws from an unseeded ThreadLocalRandom / MersenneTwister(nanoTime): parity is distributional.  Here the
// stream is counter-based, splitmix64(seed, target, level, draw), so results do not depend on the launch shape and the
// CPU oracle (oracle/dm_oracle.c: orc_tdm_sample_batch) reproduces them bit for bit.
//
// One wave per (target, level): 64 draws per round, processed in draw order (a draw is accepted iff the sequential loop of
// the reference would accept it: valid, not yet sampled, not equal to an earlier draw of the round), accepted codes in LDS,
// a rank sort at the end, rows written straight into the buffers dm_train_forward_backward_dev reads.

struct SampleParams {
  const int32_t *seq_ids;      // [T][L] raw item ids (0 = padding)
  const int32_t *tgt_ids;      // [T]
  int64_t T;
  int L, start_level, max_level, use_mask, with_prob, tolerance, negmax;
  unsigned long long seed;
  const int32_t *neg;          // [max_level + 1] negatives per level (device)
  const int32_t *lvl_off;      // [max_level + 2] row offset of a level inside one target's block (levels below start: 0)
  const uint32_t *exists_bits;
  const int32_t *id_to_code;
  int64_t n_slots;
  int32_t non_leaf_offset, max_code;
  // categorical mode: per level the existing codes (ascending) and the normalised cumulative probabilities
  const int32_t *lv_codes; const double *lv_cdf; const int64_t *lv_start;   // lv_start [max_level + 2]
  // plan
  int32_t *tcode;              // [T] target code or -1
  int64_t *row_off;            // [T + 1] first row of every target (exclusive scan of the row counts)
  // outputs
  int32_t *codes, *seqs; uint32_t *rowmask; float *labels;      // seqs == nullptr: the per-row history stores are skipped (the CSR twin)
  int64_t cap;
};

__device__ __forceinline__ unsigned long long dm_dev_splitmix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long dm_sample_draw(unsigned long long seed, int64_t t, int level, unsigned long long ctr, int stream) {
  return dm_dev_splitmix(seed ^ dm_dev_splitmix((unsigned long long)t * 64 + (unsigned long long)level + ((unsigned long long)stream << 40)) ^
                         (ctr * 0xD6E8FEB86659FD93ull));
}
__device__ __forceinline__ int dm_code_level(int64_t code) { return 63 - __clzll((unsigned long long)(code + 1)); }
// a raw history id as the code the training steps read (TDMTree.idToCode; 0 = padding -> -1)
__device__ __forceinline__ int32_t dm_sample_hist_code(const SampleParams &p, int32_t id) {
  if (id == 0) return -1;
  if (id < p.non_leaf_offset && id >= 0 && p.id_to_code[id] >= 0) return p.id_to_code[id];
  const int32_t tt = (int32_t)((uint32_t)id - (uint32_t)p.non_leaf_offset);
  return tt > p.max_code ? -1 : tt;
}
// the CSR twin's histories: every target's, once, whether it yields rows or not; umask (or null) [T]: the rowmask word dm_sample_kernel
// gives the target's rows (bit j = position j is padding, 0 without use_mask)
__global__ void dm_sample_hist_kernel(SampleParams p, int32_t *seq_codes, uint32_t *umask) {
  const int64_t n = p.T * p.L;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    seq_codes[i] = dm_sample_hist_code(p, p.seq_ids[i]);
  if (!umask) return;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < p.T; t += (int64_t)gridDim.x * blockDim.x) {
    uint32_t w = 0;
    if (p.use_mask)
      for (int j = 0; j < p.L; j++) w |= (dm_sample_hist_code(p, p.seq_ids[t * p.L + j]) == -1 ? 1u : 0u) << j;
    umask[t] = w;
  }
}

// target ids -> codes and row counts (pathNodes of an unknown / padding target is empty: no rows)
__global__ void dm_sample_plan_kernel(SampleParams p, int64_t *cnt) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < p.T; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t tid = p.tgt_ids[t];
    int32_t tc = -1;
    if (tid > 0 && tid < p.non_leaf_offset && p.id_to_code[tid] >= 0) tc = p.id_to_code[tid];
    if (tc <= 0 || tc >= p.n_slots || !dm_bit(p.exists_bits, tc)) tc = -1;
    p.tcode[t] = tc;
    int64_t rows = 0;
    if (tc > 0) {
      int depth = dm_code_level(tc);
      if (depth > p.max_level) depth = p.max_level;
      if (depth >= p.start_level) rows = p.lvl_off[depth + 1];
    }
    cnt[t] = rows;
  }
}
// exclusive scan of cnt[0..T) into off[0..T]; one block (T is a batch of targets: thousands)
__global__ __launch_bounds__(1024) void dm_sample_scan_kernel(const int64_t *cnt, int64_t *off, int64_t T) {
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const int64_t chunk = (T + 1023) / 1024;
  const int64_t lo = tid * chunk, hi = lo + chunk < T ? lo + chunk : T;
  long long s = 0;
  for (int64_t i = lo; i < hi; i++) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) { long long a = 0; for (int i = 0; i < 1024; i++) { const long long v = part[i]; part[i] = a; a += v; } off[T] = a; }
  __syncthreads();
  long long a = part[tid];
  for (int64_t i = lo; i < hi; i++) { off[i] = a; a += cnt[i]; }
}

__global__ __launch_bounds__(256) void dm_sample_kernel(SampleParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem_s[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t *acc = (int32_t *)smem_s + (size_t)wave * (p.negmax + 64);     // accepted codes of this wave's item
  int32_t *cand = acc + p.negmax;                                        // the round's 64 candidates
  const int n_lv = p.max_level - p.start_level + 1;
  const int64_t n_items = p.T * n_lv;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < n_items; item += (int64_t)gridDim.x * 4) {
    const int64_t t = item / n_lv;
    const int level = p.start_level + (int)(item % n_lv);
    const int32_t tcode = p.tcode[t];
    if (tcode <= 0) continue;
    const int depth = dm_code_level(tcode);
    if (level > depth) continue;
    const int64_t pos = (((int64_t)tcode + 1) >> (depth - level)) - 1;          // ancestor at `level`
    const int64_t lo = ((int64_t)1 << level) - 1, width = (int64_t)1 << level;
    const int want = p.neg[level];
    int n = 0;
    // ---- draws, 64 per round, accepted in draw order
    auto run = [&](int stream, unsigned long long limit, bool categorical, bool exclude_pos) {
      for (unsigned long long base = 0; n < want && base <= limit; base += 64) {
        const unsigned long long ctr = base + lane;
        const unsigned long long rnd = dm_sample_draw(p.seed, t, level, ctr, stream);
        int64_t sc;
        if (categorical) {
          const double u = (double)(rnd >> 11) * (1.0 / 9007199254740992.0);
          const int64_t s0 = p.lv_start[level], ne = p.lv_start[level + 1] - s0;
          int64_t a = 0, b = ne;
          while (a < b) { const int64_t mid = (a + b) >> 1; if (u < p.lv_cdf[s0 + mid]) b = mid; else a = mid + 1; }
          if (a >= ne) a = ne - 1;
          sc = ne > 0 ? p.lv_codes[s0 + a] : -1;
        } else {
          sc = lo + (int64_t)(rnd % (unsigned long long)width);
        }
        bool ok = ctr <= limit && sc >= 0 && sc < p.n_slots && dm_bit(p.exists_bits, sc) && !(exclude_pos && sc == pos);
        cand[lane] = (int32_t)sc;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (ok) for (int i = 0; i < n; i++) ok &= acc[i] != (int32_t)sc;              // already sampled
        // an earlier draw of this round with the same code wins — provided IT is acceptable, which only depends on the code
        // (a rejected code is rejected at every position), so "equal to any earlier candidate" is the sequential rule
        if (ok) for (int j = 0; j < lane; j++) ok &= cand[j] != (int32_t)sc;
        const unsigned long long m = __ballot(ok);
        const int rank = __popcll(m & below);
        if (ok && n + rank < want) acc[n + rank] = (int32_t)sc;
        const int got = __popcll(m);
        n = n + got < want ? n + got : want;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    };
    const unsigned long long ulimit = 64ull * (unsigned long long)(want + 1) + 4096ull * (unsigned long long)width;
    if (want > 0) {
      if (p.with_prob) {
        run(0, (unsigned long long)(want + p.tolerance) - 1ull, true, true);      // :120-126
        run(1, ulimit, false, false);                                             // :127-139 (the positive is NOT excluded there)
      } else {
        run(0, ulimit, false, true);                                              // :146-158
      }
    }
    // ---- emit: positive first, negatives in ascending order (rank sort; codes are distinct)
    const int64_t q0 = p.row_off[t] + p.lvl_off[level];
    unsigned hm = 0;
    for (int r = lane; r <= n; r += 64) {
      int32_t code; int slot;
      if (r == 0) { code = (int32_t)pos; slot = 0; }
      else {
        code = acc[r - 1];
        int rk = 0;
        for (int i = 0; i < n; i++) rk += acc[i] < code;
        slot = 1 + rk;
      }
      const int64_t q = q0 + slot;
      if (q < p.cap) { p.codes[q] = code; p.labels[q] = r == 0 ? 1.0f : 0.0f; }
    }
    // history codes + mask of the target (TDMTree.idToCode), replicated over the n + 1 rows
    int32_t hc = -1;
    if (lane < p.L) hc = dm_sample_hist_code(p, p.seq_ids[t * p.L + lane]);
    const unsigned long long pm = __ballot(lane < p.L && hc == -1);
    hm = p.use_mask ? (unsigned)pm : 0u;
    if (p.seqs || p.rowmask) {                         // (neither: the CSR twin, dm_sample_hist_kernel writes the history once per target)
      for (int r = 0; r <= n; r++) {
        const int64_t q = q0 + r;
        if (q >= p.cap) break;
        if (lane < p.L && p.seqs) p.seqs[q * p.L + lane] = hc;
        if (lane == 0 && p.rowmask) p.rowmask[q] = hm;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------ host
int dm_tdm_set_node_probs(dm_handle_t h, const int32_t *codes, const float *probs, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_tdm_set_node_probs");
  if (!h->tree_loaded) return fail(h, DM_ERR_STATE, "dm_tdm_set_node_probs: load the tree first");
  if (!codes || !probs || n <= 0) return fail(h, DM_ERR_INVALID, "dm_tdm_set_node_probs: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<float> prob_of((size_t)h->n_slots, 0.0f);
  for (int64_t i = 0; i < n; i++) {
    if (codes[i] < 0 || codes[i] >= h->n_slots) return fail(h, DM_ERR_INDEX, "dm_tdm_set_node_probs: code outside the tree");
    if (!(probs[i] >= 0.0f)) return fail(h, DM_ERR_INVALID, "dm_tdm_set_node_probs: probabilities must be non-negative");     // EnumeratedIntegerDistribution
    prob_of[codes[i]] = probs[i];
  }
  // levelProbs (NegativeSampler.scala:59-66): existing codes of a level, ascending; cumulative normalised probabilities
  std::vector<int32_t> lc; std::vector<double> cdf; std::vector<int64_t> st(h->max_level + 2, 0);
  for (int level = 0; level <= h->max_level; level++) {
    st[level] = (int64_t)lc.size();
    const int64_t lo = ((int64_t)1 << level) - 1, hi = lo + ((int64_t)1 << level);
    double sum = 0.0;
    const size_t first = lc.size();
    for (int64_t c = lo; c < hi && c < h->n_slots; c++)
      if ((h->h_exists[c >> 5] >> (c & 31)) & 1u) { lc.push_back((int32_t)c); sum += (double)prob_of[c]; }
    if (lc.size() > first && !(sum > 0.0)) return fail(h, DM_ERR_INVALID, "dm_tdm_set_node_probs: a level has no probability mass");
    double acc = 0.0;
    for (size_t k = first; k < lc.size(); k++) { acc += (double)prob_of[lc[k]] / sum; cdf.push_back(acc); }
  }
  st[h->max_level + 1] = (int64_t)lc.size();
  dm_release(h->d_lv_codes, h->d_lv_cdf, h->d_lv_start);
  model_changed(h);
  ALLOC(h, h->d_lv_codes, lc.size() * 4);
  ALLOC(h, h->d_lv_cdf, cdf.size() * 8);
  ALLOC(h, h->d_lv_start, st.size() * 8);
  HIPCHK(h, hipMemcpy(h->d_lv_codes, lc.data(), lc.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_lv_cdf, cdf.data(), cdf.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_lv_start, st.data(), st.size() * 8, hipMemcpyHostToDevice));
  return DM_OK;
}

// kind: the scorer whose training step the rows feed (DM_KIND_DIN: the two entry points below; DM_KIND_DEEPFM: their twins in dfm_train.hip.inc)
static int sample_check(dm_ctx *h, int kind, int64_t T, int L, const int32_t *neg_counts, int n_counts, const dm_sample_opts *o, int64_t *per_target) {
  if (!h->tree_loaded || !h->ids_loaded) return fail(h, DM_ERR_STATE, "negative sampling: tree and id maps must be loaded first");
  if (kind == DM_KIND_DIN) DM_DIN_ONLY(h, "negative sampling");      // (the rows it makes feed the DIN training step)
  if (!neg_counts || !o || T < 0 || L <= 0 || L > 32 || o->start_level < 1)
    return fail(h, DM_ERR_INVALID, "negative sampling: bad arguments (start_sample_level must be >= 1, seq_len <= 32)");
  // the sampled rows go straight to dm_train_forward_backward_dev, which does not range-check them: an id map or a tree that
  // reaches past the embedding table fails HERE, like LookupTable.embeddingLookup would on the first such row (LookupTable.scala:47-53)
  if (h->w_loaded && (h->max_code >= h->num_index || h->n_slots > h->num_index))
    return fail(h, DM_ERR_INDEX, "negative sampling: tree / id-map codes exceed the embedding table (embeddingLookup would fail)");
  const int total_level = h->max_level + 1;
  if (n_counts < total_level) return fail(h, DM_ERR_INVALID, "negative sampling: Not enough negative sample layers");
  for (int l = 0; l < total_level; l++)
    if (neg_counts[l] < 0 || (int64_t)neg_counts[l] >= ((int64_t)1 << l)) return fail(h, DM_ERR_INVALID, "negative sampling: Num of negative samples must not exceed max numbers in current layer");
  if (o->with_prob && !h->d_lv_cdf) return fail(h, DM_ERR_STATE, "negative sampling: sample_with_probability needs dm_tdm_set_node_probs");
  if (o->with_prob && o->tolerance < 0) return fail(h, DM_ERR_INVALID, "negative sampling: sample_tolerance must be >= 0");
  // a level with fewer than neg + 1 existing nodes can never yield neg distinct negatives: the reference's rejection loop
  // (NegativeSampler.scala:146-158) would spin forever on it; here it is an argument error
  for (int l = o->start_level; l < total_level; l++) {
    int64_t have = 0;
    const int64_t lo = ((int64_t)1 << l) - 1, hi = lo + ((int64_t)1 << l);
    for (int64_t c = lo; c < hi && c < h->n_slots && have <= neg_counts[l]; c++) have += (h->h_exists[c >> 5] >> (c & 31)) & 1u;
    if (have < (int64_t)neg_counts[l] + 1) {
      char b[200];
      snprintf(b, sizeof b, "negative sampling: level %d has only %lld nodes, cannot draw %d distinct negatives besides the positive", l, (long long)have, neg_counts[l]);
      return fail(h, DM_ERR_INVALID, b);
    }
  }
  int64_t per = 0;
  for (int l = o->start_level; l < total_level; l++) per += 1 + neg_counts[l];
  *per_target = per;
  return DM_OK;
}

// all request / output pointers are device pointers; *n_rows = rows produced (a host sync).  d_seq_codes / d_row_off (both or neither; then
// d_seqs is null): the CSR form, histories [T][L] once per target and the plan's offsets [T + 1]; d_umask (with them, or null): [T] mask words
static int sample_dev(dm_ctx *h, const int32_t *d_seq, const int32_t *d_tgt, int64_t T, int L, const int32_t *neg_counts,
                      const dm_sample_opts *o, int32_t *d_codes, int32_t *d_seqs, uint32_t *d_rowmask, float *d_labels, int64_t cap,
                      int64_t *n_rows, int32_t *d_seq_codes = nullptr, int64_t *d_row_off = nullptr, uint32_t *d_umask = nullptr) {
  const int nl = h->max_level + 1;
  std::vector<int32_t> neg(nl), lvl_off(nl + 1, 0);
  int negmax = 1;
  for (int l = 0; l < nl; l++) { neg[l] = neg_counts[l]; if (l >= o->start_level && neg[l] > negmax) negmax = neg[l]; }
  for (int l = 0; l < nl; l++) lvl_off[l + 1] = lvl_off[l] + (l >= o->start_level ? 1 + neg[l] : 0);
  // small per-call device state: [neg | lvl_off | tcode[T] | cnt[T] | off[T + 1]]
  DevArena ar(h->samp, 2);
  const size_t o_neg = ar.add(nl * 4), o_off = ar.add((nl + 1) * 4), o_tc = ar.add((size_t)T * 4 + 4), o_cnt = ar.add((size_t)T * 8 + 8), o_ro = ar.add((size_t)(T + 1) * 8);
  const int rc_a = ar.commit(h);
  if (rc_a != DM_OK) return rc_a;
  SampleParams p{};
  p.neg = ar.ptr<const int32_t>(o_neg); p.lvl_off = ar.ptr<const int32_t>(o_off); p.tcode = ar.ptr<int32_t>(o_tc);
  int64_t *d_cnt = ar.ptr<int64_t>(o_cnt);
  p.row_off = ar.ptr<int64_t>(o_ro);
  HIPCHK(h, hipMemcpyAsync((void *)p.neg, neg.data(), nl * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync((void *)p.lvl_off, lvl_off.data(), (nl + 1) * 4, hipMemcpyHostToDevice, h->stream));
  p.seq_ids = d_seq; p.tgt_ids = d_tgt; p.T = T; p.L = L; p.start_level = o->start_level; p.max_level = h->max_level;
  p.use_mask = o->use_mask; p.with_prob = o->with_prob; p.tolerance = o->tolerance; p.negmax = negmax; p.seed = o->seed;
  p.exists_bits = h->d_exists; p.id_to_code = h->d_id_to_code; p.n_slots = h->n_slots; p.non_leaf_offset = h->non_leaf_offset;
  p.max_code = h->max_code; p.lv_codes = h->d_lv_codes; p.lv_cdf = h->d_lv_cdf; p.lv_start = h->d_lv_start;
  p.codes = d_codes; p.seqs = d_seqs; p.rowmask = d_rowmask; p.labels = d_labels; p.cap = cap;
  if (T > 0) {
    LAUNCHCHK(h, dm_sample_plan_kernel, dim3((unsigned)((T + 255) / 256 < 1024 ? (T + 255) / 256 : 1024)), dim3(256), 0, p, d_cnt);
    LAUNCHCHK(h, dm_sample_scan_kernel, dim3(1), dim3(1024), 0, d_cnt, p.row_off, T);
    const int64_t items = T * (h->max_level - o->start_level + 1);
    int64_t blocks = (items + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    const size_t lds = (size_t)4 * (negmax + 64) * 4;
    if (blocks > 0) LAUNCHCHK(h, dm_sample_kernel, dim3((unsigned)blocks), dim3(256), lds, p);
    if (d_seq_codes) {
      LAUNCHCHK(h, dm_sample_hist_kernel, dim3((unsigned)std::min<int64_t>((T * L + 255) / 256, 1024)), dim3(256), 0, p, d_seq_codes, d_umask);
      HIPCHK(h, hipMemcpyAsync(d_row_off, p.row_off, (size_t)(T + 1) * 8, hipMemcpyDeviceToDevice, h->stream));
    }
    long long total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, p.row_off + T, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_rows = total;
  } else {
    if (d_row_off) HIPCHK(h, hipMemsetAsync(d_row_off, 0, 8, h->stream));
    *n_rows = 0;
  }
  return DM_OK;
}

int dm_tdm_sample_train_batch_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                  const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                  int32_t *d_seqs, uint32_t *d_rowmask, float *d_labels, int64_t cap, int64_t *n_rows) {
  if (!h || !n_rows) return DM_ERR_INVALID;
  int64_t per = 0;
  int rc = sample_check(h, DM_KIND_DIN, T, L, neg_counts, n_counts, opts, &per);
  if (rc != DM_OK) return rc;
  *n_rows = T * per;
  if (!d_codes) return DM_OK;                        // size query: an upper bound (targets outside the tree yield no rows)
  if (!d_seq_item_ids || !d_target_item_ids || !d_seqs || !d_rowmask || !d_labels || cap < T * per)
    return fail(h, DM_ERR_INVALID, "dm_tdm_sample_train_batch_dev: output buffers too small");
  HIPCHK(h, hipSetDevice(h->device));
  return sample_dev(h, d_seq_item_ids, d_target_item_ids, T, L, neg_counts, opts, d_codes, d_seqs, d_rowmask, d_labels, cap, n_rows);
}

int dm_tdm_sample_train_batch_csr_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                      const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                      int32_t *d_seq_codes, uint32_t *d_umask, int64_t *d_row_off, float *d_labels, int64_t cap, int64_t *n_rows) {
  if (!h || !n_rows) return DM_ERR_INVALID;
  int64_t per = 0;
  int rc = sample_check(h, DM_KIND_DIN, T, L, neg_counts, n_counts, opts, &per);
  if (rc != DM_OK) return rc;
  *n_rows = T * per;
  if (!d_codes) return DM_OK;                        // size query: an upper bound, the row twin's
  if (!d_seq_item_ids || !d_target_item_ids || !d_seq_codes || !d_umask || !d_row_off || !d_labels || cap < T * per)
    return fail(h, DM_ERR_INVALID, "dm_tdm_sample_train_batch_csr_dev: output buffers too small");
  HIPCHK(h, hipSetDevice(h->device));
  return sample_dev(h, d_seq_item_ids, d_target_item_ids, T, L, neg_counts, opts, d_codes, nullptr, nullptr, d_labels, cap, n_rows, d_seq_codes, d_row_off, d_umask);
}

int dm_tdm_make_train_batch(dm_handle_t h, const int32_t *seq_item_ids, const int32_t *target_item_ids, int64_t T, int L,
                            const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *out_codes,
                            int32_t *out_seqs, uint32_t *out_rowmask, float *out_labels, int64_t cap, int64_t *n_rows) {
  if (!h || !n_rows) return DM_ERR_INVALID;
  int64_t per = 0;
  int rc = sample_check(h, DM_KIND_DIN, T, L, neg_counts, n_counts, opts, &per);
  if (rc != DM_OK) return rc;
  *n_rows = T * per;
  if (!out_codes) return DM_OK;                       // size query
  if (!seq_item_ids || !target_item_ids || !out_seqs || !out_rowmask || !out_labels || cap < T * per)
    return fail(h, DM_ERR_INVALID, "dm_tdm_make_train_batch: output buffers too small");
  if (T == 0) { *n_rows = 0; return DM_OK; }
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t R = T * per;
  int32_t *d_seq = nullptr, *d_tgt = nullptr, *d_codes = nullptr, *d_seqs = nullptr;
  uint32_t *d_mask = nullptr;
  float *d_lab = nullptr;
  DevTemps t(h);
  if ((rc = t.alloc(d_seq, (size_t)T * L * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_tgt, (size_t)T * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_codes, (size_t)R * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_seqs, (size_t)R * L * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_mask, (size_t)R * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_lab, (size_t)R * 4)) != DM_OK) return rc;
  hipError_t e = hipMemcpyAsync(d_seq, seq_item_ids, (size_t)T * L * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tgt, target_item_ids, (size_t)T * 4, hipMemcpyHostToDevice, h->stream);
  if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_tdm_make_train_batch: upload failed");
  int64_t n = 0;
  if ((rc = sample_dev(h, d_seq, d_tgt, T, L, neg_counts, opts, d_codes, d_seqs, d_mask, d_lab, R, &n)) != DM_OK) return rc;
  if (n > 0) {
    e = hipMemcpy(out_codes, d_codes, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_seqs, d_seqs, (size_t)n * L * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_rowmask, d_mask, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_labels, d_lab, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_tdm_make_train_batch: download failed");
  }
  *n_rows = n;
  return rc;
}
