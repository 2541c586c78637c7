// Deep-Retrieval M-step, the per-item path scores on the device (DESIGN.md §14): batchPathScore + aggregatePathScore + computeItemOccurrence
// (deep-retrieval/.../optim/CoordinateDescent.scala:117-163) as one beam search per sample chunk, one stable sort of the (item, path) pairs,
// segment sums in sample order and a top-C cut per item.  The greedy assignment that follows stays on the host (dr_mstep.assign_paths).
//
// Order contract: a score is acc = p_0; acc += p_1; ... over the item's samples in ascending sample index, in fp64.  The pair value is the
// slot index i * C + c, the sort is stable, a path occurs at most once per beam: inside an (item, path) segment the values ascend with the
// sample.  No floating-point atomics, no tree: the counts are integers.

#define DRM_LANE_MAX 32      // a segment of up to this many terms is one lane's loop; a longer one is walked by the whole wave, 64 gathers at a time

static inline int drm_bits_above(int64_t n) { int b = 0; while (b < 63 && ((int64_t)1 << b) <= n) b++; return b; }      // smallest b with 2^b > n
static inline int drm_ceil_log2(int64_t n) { int b = 0; while (b < 63 && ((int64_t)1 << b) < n) b++; return b; }         // smallest b with 2^b >= n

// slot (i, c) of samples [i0, i0 + n): key = (target << cbits) | path code, value = the slot; a slot at or past the sample's count gets the
// key of item `num_item` (sentinel = num_item << cbits), sorts behind every item and is cut with the tail
__global__ __launch_bounds__(256) void drm_pairs_kernel(const int32_t *paths /* [n][C][D], this chunk */, const int32_t *counts, const int32_t *tgt, int64_t i0, int64_t n,
                                                        int C, int D, int K, int cbits, unsigned long long sentinel, unsigned long long *keys, int32_t *vals) {
  const int64_t slots = n * C;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < slots; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = j / C;
    const int c = (int)(j - i * C);
    const int64_t g = (i0 + i) * C + c;
    unsigned long long key = sentinel;
    if (c < counts[i0 + i]) {
      unsigned long long code = 0;
      for (int d = 0; d < D; d++) code = code * (unsigned long long)K + (unsigned long long)paths[j * D + d];
      key = ((unsigned long long)tgt[i0 + i] << cbits) | code;
    }
    keys[g] = key;
    vals[g] = (int32_t)g;
  }
}
// computeItemOccurrence, and the number of live pairs (integer atomics: the order of integer additions does not matter)
__global__ __launch_bounds__(256) void drm_occ_kernel(const int32_t *tgt, const int32_t *counts, int64_t N, unsigned long long *occ, unsigned long long *live) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < N; base += stride) {       // whole waves stay together: the reduction below is wave-wide
    const int64_t i = base + threadIdx.x;
    unsigned long long c = 0;
    if (i < N) { atomicAdd(&occ[tgt[i]], 1ull); c = (unsigned long long)counts[i]; }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(live, c);
  }
}
// sorted position j starts a segment: a live key that differs from its predecessor
__global__ __launch_bounds__(256) void drm_heads_kernel(const unsigned long long *ks, int64_t m, unsigned long long sentinel, uint8_t *flag) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = ks[j];
    flag[j] = (k < sentinel && (j == 0 || ks[j - 1] != k)) ? 1 : 0;
  }
}

struct DrmSegParams {
  const int32_t *vs; const int32_t *seg_start; const unsigned long long *n_seg, *n_live;
  const double *prob; int64_t m;
  double *seg_score; unsigned long long *key2; int32_t *val2;
};
// Segment s = sorted positions [seg_start[s], seg_start[s + 1]) (the last one ends at the number of live pairs).  A lane folds a short
// segment; the lanes that met a long one hand it to their wave, one after the other: 64 gathered terms per round, added in lane order.
// Every position s < m also gets its pair of the next sort: key = ~bits(score) (ascending = score descending; 63 bits, the sign is
// never set), value = s; positions past the last segment get the largest key.
__global__ __launch_bounds__(256) void drm_seg_sum_kernel(DrmSegParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t S = (int64_t)*p.n_seg, M = (int64_t)*p.n_live;
  const int64_t nw = (int64_t)gridDim.x * 4, w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const unsigned long long mask63 = ~0ull >> 1;
  for (int64_t base = w0 * 64; base < p.m; base += nw * 64) {
    const int64_t s = base + lane;
    const bool live = s < S;
    int64_t a = 0, e = 0;
    if (live) { a = p.seg_start[s]; e = s + 1 < S ? (int64_t)p.seg_start[s + 1] : M; }
    const bool big = live && e - a > DRM_LANE_MAX;
    double acc = 0.0;
    if (live && !big) {
      acc = p.prob[p.vs[a]];
      for (int64_t q = a + 1; q < e; q++) acc += p.prob[p.vs[q]];
    }
    unsigned long long todo = __ballot(big);
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int64_t wa = __shfl(a, src), we = __shfl(e, src);
      double r = 0.0;
      for (int64_t q0 = wa; q0 < we; q0 += 64) {
        const int cnt = (int)(we - q0 < 64 ? we - q0 : 64);
        const double x = lane < cnt ? p.prob[p.vs[q0 + lane]] : 0.0;
        for (int l = 0; l < cnt; l++) {
          const double y = __shfl(x, l);
          r = (q0 == wa && l == 0) ? y : r + y;
        }
      }
      if (lane == src) acc = r;
    }
    if (s < p.m) {
      if (live) p.seg_score[s] = acc;
      p.key2[s] = live ? (~(unsigned long long)__double_as_longlong(acc)) & mask63 : mask63;
      p.val2[s] = (int32_t)s;
    }
  }
}
// the segments in score order get their item as the key of the last sort (in place); positions past the last segment: item `num_item`
__global__ __launch_bounds__(256) void drm_item_keys_kernel(const int32_t *v2, const unsigned long long *ks, const int32_t *seg_start, const unsigned long long *n_seg,
                                                            int64_t m, int cbits, unsigned long long num_item, unsigned long long *key3) {
  const int64_t S = (int64_t)*n_seg;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = v2[j];
    key3[j] = s < S ? ks[seg_start[s]] >> cbits : num_item;
  }
}
// (item, score descending, code ascending): an item's segments are adjacent, so rank < C <=> the element C places ahead is another item's
__global__ __launch_bounds__(256) void drm_keep_kernel(const unsigned long long *k3, int64_t m, int C, unsigned long long num_item, uint8_t *flag) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long it = k3[j];
    flag[j] = (it < num_item && (j < C || k3[j - C] != it)) ? 1 : 0;
  }
}
// kept entry t: the path code and the score of its segment
__global__ __launch_bounds__(256) void drm_emit_kernel(const int32_t *kept_seg, const unsigned long long *n_kept, const unsigned long long *ks, const int32_t *seg_start,
                                                       const double *seg_score, int64_t m, unsigned long long cmask, long long *codes, double *scores) {
  const int64_t T = (int64_t)*n_kept;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T && t < m; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = kept_seg[t];
    codes[t] = (long long)(ks[seg_start[s]] & cmask);
    scores[t] = seg_score[s];
  }
}
// item_off[v] = the first kept entry whose item is >= v (the kept items ascend), v in [0, num_item]
__global__ __launch_bounds__(256) void drm_offsets_kernel(const unsigned long long *kept_item, const unsigned long long *n_kept, int64_t num_item, long long *item_off) {
  const int64_t T = (int64_t)*n_kept;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= num_item; v += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = T;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (kept_item[mid] < (unsigned long long)v) lo = mid + 1; else hi = mid;
    }
    item_off[v] = lo;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// where one call's results lie on the device (in the state's grow-only block) until an entry point hands them out
struct DrmResult {
  const long long *item_off = nullptr, *codes = nullptr; const double *scores = nullptr; const unsigned long long *occ = nullptr;
  const double *prob = nullptr; const int32_t *counts = nullptr;
  int64_t total = 0;
};

static int64_t drm_chunk() {
  if (const long long v_ = env_int("DM_DR_MSTEP_CHUNK")) return v_;
  return 4 * 32768;                                  // whole chunks of the search's own 32 768
}

// every refusal of the two entry points that needs neither the arrays' contents nor memory
static int drm_check(dm_ctx *h, bool ptrs_ok, int64_t N, int C, const void *tp, const void *tpr, const void *tc, const char *who = "dm_dr_mstep_path_scores") {
  dm_dr_state *s = h->dr;
  if (!s || !s->loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": Deep-Retrieval model not loaded");
  if (C < 1 || C > 2048) return fail(h, DM_ERR_INVALID, std::string(who) + ": num_candidate_path must be in [1, 2048]");
  if (!ptrs_ok) return fail(h, DM_ERR_INVALID, std::string(who) + ": null argument");
  if (N < 0) return fail(h, DM_ERR_INVALID, std::string(who) + ": N must not be negative");
  const int n_tr = (tp ? 1 : 0) + (tpr ? 1 : 0) + (tc ? 1 : 0);
  if (n_tr != 0 && n_tr != 3) return fail(h, DM_ERR_INVALID, std::string(who) + ": give all three trace arrays or none");
  if (N * (int64_t)C >= ((int64_t)1 << 31))
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": N * num_candidate_path must be below 2^31 (pair indices are the sort's 32-bit values): split the samples");
  int64_t space = 1;
  for (int d = 0; d < s->D; d++) space *= s->K;      // (at most 4e18: dm_dr_load_model)
  if (drm_ceil_log2(s->num_item) + drm_ceil_log2(space) > 63)
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": ceil(log2 num_item) + ceil(log2 num_node^num_layer) must be at most 63 bits (the sort key holds item and path code)");
  return DM_OK;
}

// d_paths_all: [N x C x D] to keep every chunk's node ids (a trace), or null: one chunk-sized buffer is reused
template <typename T>
static int drm_run(dm_ctx *h, const int32_t *d_seq, const int32_t *d_tgt, int64_t N, int C, int32_t *d_paths_all, DrmResult *res) {
  dm_dr_state *s = h->dr;
  const int K = s->K, D = s->D, L = s->L;
  const int64_t num_item = s->num_item, m = N * C;
  int64_t space = 1;
  for (int d = 0; d < D; d++) space *= K;
  const int cbits = drm_ceil_log2(space), ibits = drm_bits_above(num_item);       // ibits holds num_item itself: the key of a dead slot
  const unsigned long long sentinel = (unsigned long long)num_item << cbits, cmask = cbits ? (~0ull >> (64 - cbits)) : 0ull;
  const int64_t chunk = std::min<int64_t>(drm_chunk(), N);
  const bool detail = dr_time_launches();
  int rc;
  DevArena ar(s->ms, 8);
  size_t o_k[3], o_v[3];
  for (int i = 0; i < 3; i++) { o_k[i] = ar.add((size_t)m * 8); o_v[i] = ar.add((size_t)m * 4); }
  const size_t o_prob = ar.add((size_t)m * 8), o_cnt = ar.add((size_t)N * 4), o_flag = ar.add((size_t)m), o_start = ar.add((size_t)m * 4);
  const size_t o_score = ar.add((size_t)m * 8), o_out = ar.add((size_t)m * 8), o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_off = ar.add((size_t)(num_item + 1) * 8), o_occ = ar.add((size_t)num_item * 8), o_n = ar.add(64);
  const size_t o_paths = d_paths_all ? 0 : ar.add((size_t)chunk * C * D * 4);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  unsigned long long *kb[3]; int32_t *vb[3];
  for (int i = 0; i < 3; i++) { kb[i] = ar.ptr<unsigned long long>(o_k[i]); vb[i] = ar.ptr<int32_t>(o_v[i]); }
  double *prob = ar.ptr<double>(o_prob), *seg_score = ar.ptr<double>(o_score), *out_scores = ar.ptr<double>(o_out);
  int32_t *counts = ar.ptr<int32_t>(o_cnt), *seg_start = ar.ptr<int32_t>(o_start);
  uint8_t *flag = ar.ptr<uint8_t>(o_flag);
  uint32_t *tmp = ar.ptr<uint32_t>(o_tmp);
  long long *item_off = ar.ptr<long long>(o_off);
  unsigned long long *occ = ar.ptr<unsigned long long>(o_occ), *n_seg = ar.ptr<unsigned long long>(o_n), *n_live = n_seg + 1, *n_kept = n_seg + 2;
  HIPCHK(h, hipMemsetAsync(occ, 0, (size_t)num_item * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(n_seg, 0, 64, h->stream));
  // ---- the search, chunk by chunk, and the pairs of each chunk
  for (int64_t i0 = 0; i0 < N; i0 += chunk) {
    const int64_t n = std::min<int64_t>(chunk, N - i0);
    int32_t *paths = d_paths_all ? d_paths_all + i0 * C * D : ar.ptr<int32_t>(o_paths);
    if ((rc = dr_beam_dev_t<T>(h, d_seq + i0 * L, n, C, paths, prob + i0 * C, counts + i0)) != DM_OK) return rc;
    rc = timed(h, EV_DRM_PAIRS, detail, [&] {
      return LAUNCH(h, drm_pairs_kernel, dim3(drt_blocks(h, n * C, 256)), dim3(256), 0, paths, counts, d_tgt, i0, n, C, D, K, cbits, sentinel, kb[0], vb[0]);
    });
    if (rc != DM_OK) return rc;
  }
  if ((rc = timed(h, EV_DRM_OCC, detail, [&] { return LAUNCH(h, drm_occ_kernel, dim3(drt_blocks(h, N, 256)), dim3(256), 0, d_tgt, counts, N, occ, n_live); })) != DM_OK) return rc;
  // ---- (item, path) segments: one stable sort, the heads' positions
  int where = 0;
  rc = timed(h, EV_DRM_SORT, detail, [&]() -> int {
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[0], vb[0], kb[1], vb[1], m, 0, ibits + cbits, tmp, &where));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  const unsigned long long *ks = kb[where];
  const int32_t *vs = vb[where];
  const int f0 = where ^ 1;                              // the pair the first sort left free; pair 2 is the other half of the next two sorts
  rc = timed(h, EV_DRM_HEADS, detail, [&]() -> int {
    if ((rc = LAUNCH(h, drm_heads_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, ks, m, sentinel, flag)) != DM_OK) return rc;
    HIPCHK(h, (dev_select_flagged<int32_t>(h->stream, (const int32_t *)nullptr, (const char *)nullptr, (const uint8_t *)flag, seg_start, (char *)nullptr, n_seg, m, tmp)));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  // ---- the sums, in sample order
  {
    DrmSegParams p{};
    p.vs = vs; p.seg_start = seg_start; p.n_seg = n_seg; p.n_live = n_live; p.prob = prob; p.m = m;
    p.seg_score = seg_score; p.key2 = kb[f0]; p.val2 = vb[f0];
    if ((rc = timed(h, EV_DRM_SEGSUM, detail, [&] { return LAUNCH(h, drm_seg_sum_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, p); })) != DM_OK) return rc;
  }
  // ---- top C per item: stable by score descending, then stable by item -> (item, score descending, code ascending); rank < C survives
  int w2 = 0, w3 = 0;
  rc = timed(h, EV_DRM_SCORE_SORT, detail, [&]() -> int {
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[f0], vb[f0], kb[2], vb[2], m, 0, 63, tmp, &w2));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  const int a2 = w2 ? 2 : f0, b2 = w2 ? f0 : 2;
  rc = timed(h, EV_DRM_ITEM_SORT, detail, [&]() -> int {
    if ((rc = LAUNCH(h, drm_item_keys_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, vb[a2], ks, seg_start, n_seg, m, cbits, num_item, kb[a2])) != DM_OK) return rc;
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[a2], vb[a2], kb[b2], vb[b2], m, 0, ibits, tmp, &w3));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  const int a3 = w3 ? b2 : a2, b3 = w3 ? a2 : b2;
  rc = timed(h, EV_DRM_CUT, detail, [&]() -> int {
    if ((rc = LAUNCH(h, drm_keep_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, kb[a3], m, C, num_item, flag)) != DM_OK) return rc;
    HIPCHK(h, (dev_select_flagged<unsigned long long, int32_t>(h->stream, (const unsigned long long *)kb[a3], (const int32_t *)vb[a3], (const uint8_t *)flag, kb[b3], vb[b3],
                                                               n_kept, m, tmp)));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  long long *out_codes = (long long *)kb[a3];             // (the cut's input is dead)
  rc = timed(h, EV_DRM_EMIT, detail, [&] {
    const int r = LAUNCH(h, drm_emit_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, vb[b3], n_kept, ks, seg_start, seg_score, m, cmask, out_codes, out_scores);
    return r != DM_OK ? r : LAUNCH(h, drm_offsets_kernel, dim3(drt_blocks(h, num_item + 1, 256)), dim3(256), 0, kb[b3], n_kept, num_item, item_off);
  });
  if (rc != DM_OK) return rc;
  unsigned long long total = 0;
  HIPCHK(h, hipMemcpyAsync(&total, n_kept, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));            // the call's one wait before its results move
  res->item_off = item_off; res->codes = out_codes; res->scores = out_scores; res->occ = occ; res->prob = prob; res->counts = counts;
  res->total = (int64_t)total;
  return DM_OK;
}

static int drm_run_any(dm_ctx *h, const int32_t *d_seq, const int32_t *d_tgt, int64_t N, int C, int32_t *d_paths_all, DrmResult *res) {
  return h->dr->dtype == DM_F32 ? drm_run<float>(h, d_seq, d_tgt, N, C, d_paths_all, res) : drm_run<double>(h, d_seq, d_tgt, N, C, d_paths_all, res);
}
static int drm_short_cap(dm_ctx *h, int64_t cap, int64_t need, const char *who = "dm_dr_mstep_path_scores") {
  return fail(h, DM_ERR_INVALID, std::string(who) + ": cap " + std::to_string(cap) + " is too small, " + std::to_string(need) + " entries are needed (out_total)");
}

int dm_dr_mstep_path_scores_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_targets, int64_t N, int num_candidate_path, int64_t cap, int64_t *d_out_item_off,
                                int64_t *d_out_codes, double *d_out_scores, int64_t *d_out_occurrence, int64_t *out_total, int32_t *d_trace_paths, double *d_trace_probs,
                                int32_t *d_trace_counts) {
  if (!h) return DM_ERR_INVALID;
  const int C = num_candidate_path;
  const bool ptrs_ok = d_out_item_off && out_total && cap >= 0 && (N <= 0 || (d_seq_ids && d_targets)) && (cap == 0 || (d_out_codes && d_out_scores));
  int rc = drm_check(h, ptrs_ok, N, C, d_trace_paths, d_trace_probs, d_trace_counts);
  if (rc != DM_OK || (rc = dr_check_search(h, "dm_dr_mstep_path_scores", N, C, false)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_dr_state *s = h->dr;
  if (N == 0) {
    HIPCHK(h, hipMemsetAsync(d_out_item_off, 0, (size_t)(s->num_item + 1) * 8, h->stream));
    if (d_out_occurrence) HIPCHK(h, hipMemsetAsync(d_out_occurrence, 0, (size_t)s->num_item * 8, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *out_total = 0;
    return DM_OK;
  }
  DrmResult r;
  if ((rc = drm_run_any(h, d_seq_ids, d_targets, N, C, d_trace_paths, &r)) != DM_OK) return rc;
  *out_total = r.total;
  if (r.total > cap) return drm_short_cap(h, cap, r.total);
  const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
  HIPCHK(h, hipMemcpyAsync(d_out_item_off, r.item_off, (size_t)(s->num_item + 1) * 8, dd, h->stream));
  if (r.total) {
    HIPCHK(h, hipMemcpyAsync(d_out_codes, r.codes, (size_t)r.total * 8, dd, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_out_scores, r.scores, (size_t)r.total * 8, dd, h->stream));
  }
  if (d_out_occurrence) HIPCHK(h, hipMemcpyAsync(d_out_occurrence, r.occ, (size_t)s->num_item * 8, dd, h->stream));
  if (d_trace_paths) {
    HIPCHK(h, hipMemcpyAsync(d_trace_probs, r.prob, (size_t)N * C * 8, dd, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_trace_counts, r.counts, (size_t)N * 4, dd, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_dr_mstep_path_scores(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N, int num_candidate_path, int64_t cap, int64_t *out_item_off,
                            int64_t *out_codes, double *out_scores, int64_t *out_occurrence, int64_t *out_total, int32_t *trace_paths, double *trace_probs,
                            int32_t *trace_counts) {
  if (!h) return DM_ERR_INVALID;
  const int C = num_candidate_path;
  const bool ptrs_ok = out_item_off && out_total && cap >= 0 && (N <= 0 || (seq_ids && targets)) && (cap == 0 || (out_codes && out_scores));
  int rc = drm_check(h, ptrs_ok, N, C, trace_paths, trace_probs, trace_counts);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, N * s->L)) != DM_OK) return rc;
  for (int64_t i = 0; i < N; i++)
    if (targets[i] < 0 || targets[i] >= s->num_item) return fail(h, DM_ERR_INDEX, "dm_dr_mstep_path_scores: target outside [0, num_item)");
  if ((rc = dr_check_search(h, "dm_dr_mstep_path_scores", N, C, false)) != DM_OK) return rc;
  if (N == 0) {
    memset(out_item_off, 0, (size_t)(s->num_item + 1) * 8);
    if (out_occurrence) memset(out_occurrence, 0, (size_t)s->num_item * 8);
    *out_total = 0;
    return DM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t b_seq = DevArena::up((size_t)N * s->L * 4);
  if ((rc = s->ms_io.reserve(h, b_seq + DevArena::up((size_t)N * 4))) != DM_OK) return rc;
  int32_t *d_seq = (int32_t *)s->ms_io.p, *d_tgt = (int32_t *)((char *)s->ms_io.p + b_seq);
  HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids, (size_t)N * s->L * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_tgt, targets, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
  DevTemps tmp(h);
  int32_t *d_paths_all = nullptr;
  if (trace_paths && (rc = tmp.alloc(d_paths_all, (size_t)N * C * s->D * 4)) != DM_OK) return rc;
  DrmResult r;
  if ((rc = drm_run_any(h, d_seq, d_tgt, N, C, d_paths_all, &r)) != DM_OK) return rc;
  *out_total = r.total;
  if (r.total > cap) return drm_short_cap(h, cap, r.total);
  const hipMemcpyKind dh = hipMemcpyDeviceToHost;
  HIPCHK(h, hipMemcpyAsync(out_item_off, r.item_off, (size_t)(s->num_item + 1) * 8, dh, h->stream));
  if (r.total) {
    HIPCHK(h, hipMemcpyAsync(out_codes, r.codes, (size_t)r.total * 8, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(out_scores, r.scores, (size_t)r.total * 8, dh, h->stream));
  }
  if (out_occurrence) HIPCHK(h, hipMemcpyAsync(out_occurrence, r.occ, (size_t)s->num_item * 8, dh, h->stream));
  if (trace_paths) {
    HIPCHK(h, hipMemcpyAsync(trace_paths, d_paths_all, (size_t)N * C * s->D * 4, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(trace_probs, r.prob, (size_t)N * C * 8, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(trace_counts, r.counts, (size_t)N * 4, dh, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}
