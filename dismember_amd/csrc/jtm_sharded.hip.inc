// JTM.optimize (jtm/src/main/scala/com/mass/jtm/optim/JTM.scala:22-73) over the cached catalogue, all gap steps in one call — on one
// GPU, or sharded over the ranks of the attached communicator (BASELINE configs[3]; SURVEY.md §8e).
//
// The reference's multi-worker schedule (JTM.scala:33-68; JTMAsync.scala:43-75 is the same switch): while a level has fewer parent
// nodes than workers the workers split the ITEMS of a node, afterwards each worker takes a contiguous range of parent NODES
// (taskSize / extraSize, :47-52).  Here a worker is a GPU and a gap step is
//   (a) scoring, always item-sharded: rank r scores the cached rows of its contiguous item range [lo_r, hi_r) into ITS slice of the
//       [items x 2^gap] weight matrix — every weight is one GPU's sequential fp32 sum, so the matrix is bit-identical to the
//       single-rank one whatever the world size;
//   (b) ONE in-place all-gather of the slices, device to device (RCCL over xGMI: rank r's slice is broadcast from where it was
//       written; 160 MB at 10 M items, gap 2).  The host transport (several workers on one GPU: the tests) stages through host memory;
//   (c) the greedy re-balance: replicated on every rank while the level has fewer parents than ranks; from then on rank r
//       re-balances the parents [p_lo_r, p_hi_r) only — their items compacted in item order, so each parent's list order and hence
//       its result is the single-rank one — and the ranks all-gather (item, new node) pairs (80 MB at 10 M items).
// Nothing but the final projection leaves HBM.  Single rank (no communicator, or one rank): steps (a) and (c) over everything.


// (jtm_shard_range — the contiguous split of the items over the ranks — lives in jtm_host.hip.inc: dm_jtm_shard_range exports it)

__global__ void jtm_owner_flag_kernel(const int32_t *item_node, int64_t n, int32_t lo_code, int64_t p_lo, int64_t p_hi, uint8_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = (int64_t)item_node[i] - lo_code;       // items outside the level (p < 0) belong to nobody and keep their entry
    flag[i] = p >= p_lo && p < p_hi;
  }
}
__global__ void jtm_compact_kernel(const int32_t *sel, int64_t m, int C, const float *w, const int32_t *old_node, const int32_t *item_node,
                                   float *c_w, int32_t *c_old, int32_t *c_node) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m * C; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = t / C;
    const int c = (int)(t - k * C);
    const int64_t i = sel[k];
    c_w[t] = w[i * C + c];
    if (c == 0) { c_old[k] = old_node[i]; c_node[k] = item_node[i]; }
  }
}
__global__ void jtm_scatter_kernel(const int32_t *sel, const int32_t *val, int64_t m, int32_t *out) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) out[sel[k]] = val[k];
}

// in-place all-gather on the handle's stream: block r = bytes [off[r], off[r+1]) of d_buf, written by rank r
static int jtm_all_gather_inplace(dm_ctx *h, char *d_buf, const std::vector<uint64_t> &off) {
  dm_comm *c = h->comm;
  const int W = c->nranks;
  std::vector<uint64_t> sizes(W);
  for (int r = 0; r < W; r++) sizes[r] = off[r + 1] - off[r];
  if (c->kind == DM_COMM_RCCL) {
    const int rc = rccl_all_gather_v_dev(c, d_buf + off[c->rank], d_buf, sizes, h->stream);
    return rc == DM_OK ? DM_OK : fail(h, rc, c->err);
  }
  std::vector<char> mine((size_t)sizes[c->rank]), all;
  std::vector<uint64_t> got;
  if (!mine.empty()) HIPCHK(h, hipMemcpyAsync(mine.data(), d_buf + off[c->rank], mine.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int rc = host_all_gather_v(c, mine.data(), mine.size(), all, got);
  if (rc != DM_OK) return fail(h, rc, c->err);
  for (int r = 0; r < W; r++)
    if (got[r] != sizes[r]) return fail(h, DM_ERR_STATE, "dm_jtm_optimize_cached: the ranks disagree on the shard sizes (different catalogues?)");
  if (!all.empty()) HIPCHK(h, hipMemcpy(d_buf + off[0], all.data(), all.size(), hipMemcpyHostToDevice));
  return DM_OK;
}

// variable-size all-gather of device blocks (block of this rank: d_send, `bytes`); d_recv receives the blocks in rank order,
// sizes[r] their lengths.  One host round trip for the sizes.
static int jtm_all_gather_v(dm_ctx *h, const char *d_send, size_t bytes, char *d_recv, size_t recv_cap, std::vector<uint64_t> &sizes) {
  dm_comm *c = h->comm;
  const int W = c->nranks;
  if (c->kind == DM_COMM_RCCL) {
    std::vector<char> buf; std::vector<uint64_t> sz;
    const uint64_t mine = bytes;
    int rc = comm_all_gather_v_host(c, &mine, 8, buf, sz);
    if (rc != DM_OK) return fail(h, rc, c->err);
    sizes.assign(W, 0);
    memcpy(sizes.data(), buf.data(), 8 * (size_t)W);
    uint64_t total = 0;
    for (auto v : sizes) total += v;
    if (total > recv_cap) return fail(h, DM_ERR_STATE, "dm_jtm_optimize_cached: projection exchange larger than the catalogue");
    HIPCHK(h, hipSetDevice(h->device));
    rc = rccl_all_gather_v_dev(c, d_send, d_recv, sizes, h->stream);
    return rc == DM_OK ? DM_OK : fail(h, rc, c->err);
  }
  std::vector<char> mine(bytes), all;
  if (bytes) HIPCHK(h, hipMemcpyAsync(mine.data(), d_send, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int rc = host_all_gather_v(c, mine.data(), bytes, all, sizes);
  if (rc != DM_OK) return fail(h, rc, c->err);
  if (all.size() > recv_cap) return fail(h, DM_ERR_STATE, "dm_jtm_optimize_cached: projection exchange larger than the catalogue");
  if (!all.empty()) HIPCHK(h, hipMemcpy(d_recv, all.data(), all.size(), hipMemcpyHostToDevice));
  return DM_OK;
}

// replicated re-balance of every parent on this rank: the device rounds, or — shapes they do not cover — the host logic on
// downloaded arrays (identical results; jtm_rebalance_all_t)
static int jtm_rebalance_step(dm_ctx *h, const float *d_w, const int32_t *d_old, const int32_t *d_proj, int64_t n, int old_level, int level,
                              int max_assign, int32_t *d_next) {
  int rc = jtm_rebalance_on_device(h, n, old_level, level) ? jtm_rebalance_all_dev(h, d_w, d_old, d_proj, n, old_level, level, max_assign, d_next)
                                                          : DM_ERR_UNSUPPORTED;
  if (rc != DM_ERR_UNSUPPORTED) return rc;
  const int C = 1 << (level - old_level);
  std::vector<float> w((size_t)n * C);
  std::vector<int32_t> hp((size_t)n), ho((size_t)n), hn((size_t)n);
  if (hipMemcpy(w.data(), d_w, w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hp.data(), d_proj, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ho.data(), d_old, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: download failed");
  rc = jtm_rebalance_all_t<float>(h, w.data(), ho.data(), hp.data(), n, old_level, level, max_assign, hn.data(), "dm_jtm_optimize_cached");
  if (rc == DM_OK && hipMemcpy(d_next, hn.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: upload failed");
  return rc;
}

static int jtm_optimize_impl(dm_ctx *h, int scorer, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical, int min_level,
                             int use_mask, int32_t *out_proj, double *step_seconds) {
  if (h->jtm_off.empty()) return fail(h, DM_ERR_STATE, "dm_jtm_optimize_cached: call dm_jtm_cache_rows first");
  if (!item_code || !out_proj || n_items != (int64_t)h->jtm_off.size() - 1 || max_level < 1 || max_level > 30 || gap < 1 || gap > 8)
    return fail(h, DM_ERR_INVALID, "dm_jtm_optimize_cached: bad arguments (n_items must be the cached catalogue)");
  dm_jtm_stats &st = h->jtm_stats;
  st = dm_jtm_stats{};
  dm_comm *c = h->comm;
  const int W = c ? c->nranks : 1, rank = c ? c->rank : 0;
  st.nranks = W; st.transport = c ? c->kind : -1;
  if (n_items == 0) return DM_OK;
  for (int64_t i = 0; i < n_items; i++)
    if (item_code[i] < 0) return fail(h, DM_ERR_INVALID, "dm_jtm_optimize_cached: negative item code");
  HIPCHK(h, hipSetDevice(h->device));
  const int Cmax = 1 << gap;
  char *A = nullptr;
  const size_t bw = DevArena::up((size_t)n_items * Cmax * 4), bi = DevArena::up((size_t)n_items * 4);
  // sharded runs add: owner flags [n], (item, node) pairs of this rank [2n] and of all ranks [2n], select scratch
  size_t tmp_sel = 0;
  if (W > 1) tmp_sel = dev_sort_scratch_bytes(n_items);
  const size_t extra = W > 1 ? DevArena::up((size_t)n_items) + 4 * bi + DevArena::up(tmp_sel) + 256 : 0;
  // (a rank-local failure from here to the first gap step is AGREED below before anybody enters a collective: returning at once would
  //  leave the peers waiting in the first step's agreement)
  DevTemps t(h);
  int rc = t.alloc(A, bw + 4 * bi + extra);
  float *d_w = (float *)A;
  int32_t *d_code = (int32_t *)(A + bw), *d_old = (int32_t *)(A + bw + bi), *d_proj = (int32_t *)(A + bw + 2 * bi), *d_next = (int32_t *)(A + bw + 3 * bi);
  char *X = A + bw + 4 * bi;
  uint8_t *d_flag = (uint8_t *)X;
  int32_t *d_pack = (int32_t *)(X + DevArena::up((size_t)n_items)), *d_all = (int32_t *)(X + DevArena::up((size_t)n_items) + 2 * bi);
  void *d_tmp = X + DevArena::up((size_t)n_items) + 4 * bi;
  unsigned long long *d_cnt = (unsigned long long *)(X + DevArena::up((size_t)n_items) + 4 * bi + DevArena::up(tmp_sel));
  char *B = nullptr;                 // compact copies of this rank's parents' items (node-sharded steps), grown on demand
  size_t b_cap = 0;
  double t_sc = 0, t_rb = 0, t_ex = 0;
  typedef std::chrono::steady_clock clk;
  auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  if (rc == DM_OK && (hipMemcpyAsync(d_code, item_code, (size_t)n_items * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
                      hipMemsetAsync(d_proj, 0, (size_t)n_items * 4, h->stream) != hipSuccess))          // first all assigned to the root (:23-26)
    rc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: upload failed");
  rc = comm_agree(h, c, rc, "dm_jtm_optimize_cached");          // every rank enters the gap steps, or none does
  int64_t lo = 0, hi = n_items;
  std::vector<uint64_t> woff;
  for (int old_level = 0; old_level < max_level && rc == DM_OK; old_level += gap) {
    const int level = std::min(max_level, old_level + gap);
    const int C = 1 << (level - old_level);
    const int max_assign = 1 << (max_level - level);             // TreeLearning.scala:56
    rc = LAUNCH(h, jtm_ancestor_kernel, dim3(2048), dim3(256), 0, d_code, n_items, level, d_old);      // (a failure reaches the agreement below)
    // ---- (a) scoring: this rank's contiguous item range, into its slice of the weight matrix
    if (W > 1) jtm_shard_range(n_items, rank, W, &lo, &hi);
    const auto t0 = clk::now();
    if (rc == DM_OK && hi > lo)
      rc = jtm_child_weights_impl(h, scorer, h->jtm_off.data() + lo, nullptr, true, lo, nullptr, hi - lo, h->jtm_L, old_level, level, hierarchical, min_level,
                                  use_mask, nullptr, d_proj + lo, d_w + lo * C);
    const auto t1 = clk::now();
    t_sc += secs(t0, t1);
    st.items_scored += (uint64_t)(hi - lo);
    if ((rc = comm_agree(h, c, rc, "dm_jtm_optimize_cached")) != DM_OK) break;       // every rank reaches the all-gather, or none does
    // ---- (b) the slices, all-gathered in place
    if (W > 1) {
      woff.assign(W + 1, 0);
      for (int r = 0; r < W; r++) { int64_t a, b; jtm_shard_range(n_items, r, W, &a, &b); woff[r] = (uint64_t)a * C * 4; woff[r + 1] = (uint64_t)b * C * 4; }
      rc = jtm_all_gather_inplace(h, (char *)d_w, woff);
      if (rc == DM_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: weight exchange failed");
      st.weight_bytes += woff[W];
      if (rc != DM_OK) break;
    }
    const auto t2 = clk::now();
    t_ex += secs(t1, t2);
    // ---- (c) re-balance
    const int64_t P = (int64_t)1 << old_level;
    const bool node_sharded = W > 1 && P >= W && jtm_rebalance_on_device(h, n_items, old_level, level);    // the same decision on every rank
    if (!node_sharded) {
      rc = jtm_rebalance_step(h, d_w, d_old, d_proj, n_items, old_level, level, max_assign, d_next);
      t_rb += secs(t2, clk::now());
      st.steps_replicated++;
    } else {
      int64_t p_lo, p_hi;
      jtm_shard_range(P, rank, W, &p_lo, &p_hi);
      // (rank-local failures up to the projection exchange are collected in lrc: the peers are told before anybody enters the all-gather)
      int lrc = LAUNCH(h, jtm_owner_flag_kernel, dim3(2048), dim3(256), 0, d_proj, n_items, (int32_t)(P - 1), p_lo, p_hi, d_flag);
      unsigned long long hm = 0;
      if (lrc == DM_OK &&
          (dev_select_flagged<int32_t>(h->stream, (const int32_t *)nullptr, (const char *)nullptr, (const uint8_t *)d_flag, d_pack, (char *)nullptr, d_cnt, n_items,
                                       (uint32_t *)d_tmp) != hipSuccess ||      // the item indices themselves, in order
           hipMemcpyAsync(&hm, d_cnt, 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess))
        lrc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: item selection failed");
      const int64_t m = lrc == DM_OK ? (int64_t)hm : 0;
      if (lrc == DM_OK && m > 0) {
        const size_t need = DevArena::up((size_t)m * C * 4) + 2 * DevArena::up((size_t)m * 4);
        if (need > b_cap) { t.drop(B); b_cap = 0; if ((lrc = t.alloc(B, need + need / 4)) == DM_OK) b_cap = need + need / 4; }
        if (lrc == DM_OK) {
          float *c_w = (float *)B;
          int32_t *c_old = (int32_t *)(B + DevArena::up((size_t)m * C * 4)), *c_node = (int32_t *)(B + DevArena::up((size_t)m * C * 4) + DevArena::up((size_t)m * 4));
          lrc = LAUNCH(h, jtm_compact_kernel, dim3(2048), dim3(256), 0, d_pack, m, C, d_w, d_old, d_proj, c_w, c_old, c_node);
          if (lrc == DM_OK) lrc = jtm_rebalance_all_dev(h, c_w, c_old, c_node, m, old_level, level, max_assign, d_pack + m);
          if (lrc == DM_ERR_UNSUPPORTED) lrc = fail(h, DM_ERR_STATE, "dm_jtm_optimize_cached: device re-balance refused a shape it was planned for");
        }
      }
      const auto t3 = clk::now();
      t_rb += secs(t2, t3);
      // every rank's (item, new node) pairs; items outside the level keep their entry
      std::vector<uint64_t> sizes;
      if (lrc == DM_OK && hipMemcpyAsync(d_next, d_proj, (size_t)n_items * 4, hipMemcpyDeviceToDevice, h->stream) != hipSuccess) lrc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: copy failed");
      if ((rc = comm_agree(h, c, lrc, "dm_jtm_optimize_cached")) != DM_OK) break;
      rc = jtm_all_gather_v(h, (const char *)d_pack, (size_t)m * 8, (char *)d_all, (size_t)n_items * 8, sizes);
      if (rc != DM_OK) break;
      uint64_t o = 0;
      for (int r = 0; r < W; r++) {
        const int64_t mr = (int64_t)(sizes[r] / 8);
        if (mr && (rc = LAUNCH(h, jtm_scatter_kernel, dim3(1024), dim3(256), 0, d_all + o, d_all + o + mr, mr, d_next)) != DM_OK) break;
        o += 2 * (uint64_t)mr;
        st.proj_bytes += sizes[r];
      }
      if (rc != DM_OK) break;
      if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: projection exchange failed"); break; }
      t_ex += secs(t3, clk::now());
      st.steps_node_sharded++;
      st.items_rebalanced += (uint64_t)m;
    }
    std::swap(d_proj, d_next);
  }
  if (rc == DM_OK && hipMemcpy(out_proj, d_proj, (size_t)n_items * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, DM_ERR_HIP, "dm_jtm_optimize_cached: download failed");
  (void)hipStreamSynchronize(h->stream);
  h->jtm_score_s = t_sc; h->jtm_rebal_s = t_rb;
  st.scoring_s = t_sc; st.rebalance_s = t_rb; st.exchange_s = t_ex;
  if (step_seconds) { step_seconds[0] = t_sc; step_seconds[1] = t_rb; }
  return rc;
}

int dm_jtm_optimize_cached(dm_handle_t h, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical, int min_level,
                           int use_mask, int32_t *out_proj, double *step_seconds) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  DM_DIN_ONLY(h, "dm_jtm_optimize_cached");
  try { return jtm_optimize_impl(h, DM_KIND_DIN, item_code, n_items, max_level, gap, hierarchical, min_level, use_mask, out_proj, step_seconds); }
  catch (const std::exception &e) { return fail(h, DM_ERR_INVALID, std::string("dm_jtm_optimize_cached: ") + e.what()); }
}

// The DeepFM twin: one rank (dfm_jtm_enter refuses an attached communicator of more), so none of the collectives above is entered
int dm_deepfm_jtm_optimize_cached(dm_handle_t h, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical, int min_level,
                                  int use_mask, int32_t *out_proj, double *step_seconds) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  const int rc = dfm_jtm_enter(h, "dm_deepfm_jtm_optimize_cached", use_mask, h->jtm_off.empty() ? -1 : h->jtm_L);
  if (rc != DM_OK) return rc;
  try { return jtm_optimize_impl(h, DM_KIND_DEEPFM, item_code, n_items, max_level, gap, hierarchical, min_level, 0, out_proj, step_seconds); }
  catch (const std::exception &e) { return fail(h, DM_ERR_INVALID, std::string("dm_deepfm_jtm_optimize_cached: ") + e.what()); }
}

// The same for ONE process driving every rank of a dm_comm_create_all clique (the reference's shape: one JVM, N workers): hs[i] carries
// rank i and holds the cached catalogue; each rank runs on its own host thread (the collectives meet inside RCCL).  Every rank ends with
// the same projection — checked — and out_proj receives it.
int dm_jtm_optimize_all(dm_handle_t *hs, int n, const int32_t *item_code, int64_t n_items, int max_level, int gap, int hierarchical,
                        int min_level, int use_mask, int32_t *out_proj, double *step_seconds) {
  if (!hs || n < 1 || !hs[0]) return DM_ERR_INVALID;
  if (n == 1) return dm_jtm_optimize_cached(hs[0], item_code, n_items, max_level, gap, hierarchical, min_level, use_mask, out_proj, step_seconds);
  for (int i = 0; i < n; i++) {
    if (!hs[i]) return DM_ERR_INVALID;
    if (!hs[i]->comm || hs[i]->comm->nranks != n || hs[i]->comm->rank != i)
      return fail(hs[0], DM_ERR_INVALID, "dm_jtm_optimize_all: handle i must carry rank i of one communicator clique");
  }
  if (!out_proj || n_items < 0) return fail(hs[0], DM_ERR_INVALID, "dm_jtm_optimize_all: bad arguments");
  std::vector<std::vector<int32_t>> outs((size_t)n);
  std::vector<int> rcs((size_t)n, DM_OK);
  std::vector<std::array<double, 2>> ss((size_t)n);
  std::vector<std::thread> pool;
  for (int i = 0; i < n; i++)
    pool.emplace_back([&, i]() {
      outs[(size_t)i].resize((size_t)(n_items > 0 ? n_items : 1));
      rcs[(size_t)i] = dm_jtm_optimize_cached(hs[i], item_code, n_items, max_level, gap, hierarchical, min_level, use_mask, outs[(size_t)i].data(), ss[(size_t)i].data());
    });
  for (auto &t : pool) t.join();
  for (int i = 0; i < n; i++)
    if (rcs[(size_t)i] != DM_OK) { if (i) hs[0]->err = hs[i]->err; return rcs[(size_t)i]; }
  for (int i = 1; i < n; i++)
    if (memcmp(outs[0].data(), outs[(size_t)i].data(), (size_t)n_items * 4) != 0)
      return fail(hs[0], DM_ERR_STATE, "dm_jtm_optimize_all: rank " + std::to_string(i) + " ended with a different projection than rank 0");
  memcpy(out_proj, outs[0].data(), (size_t)n_items * 4);
  if (step_seconds) { step_seconds[0] = ss[0][0]; step_seconds[1] = ss[0][1]; }
  return DM_OK;
}

// what the last dm_jtm_optimize_cached on this handle did: out[0..9] = nranks, transport (-1: no communicator), items this rank
// scored (summed over the gap steps), items it re-balanced in node-sharded steps, steps with a replicated re-balance, node-sharded
// steps, weight bytes all-gathered, projection bytes all-gathered, 0, 0; secs[0..2] = scoring, re-balance, exchange seconds
int dm_jtm_optimize_stats(dm_handle_t h, uint64_t *out10, double *secs3) {
  if (!h || !out10 || !secs3) return DM_ERR_INVALID;
  const dm_jtm_stats &s = h->jtm_stats;
  out10[0] = (uint64_t)s.nranks; out10[1] = (uint64_t)(int64_t)s.transport; out10[2] = s.items_scored; out10[3] = s.items_rebalanced;
  out10[4] = (uint64_t)s.steps_replicated; out10[5] = (uint64_t)s.steps_node_sharded; out10[6] = s.weight_bytes; out10[7] = s.proj_bytes;
  out10[8] = out10[9] = 0;
  secs3[0] = s.scoring_s; secs3[1] = s.rebalance_s; secs3[2] = s.exchange_s;
  return DM_OK;
}
