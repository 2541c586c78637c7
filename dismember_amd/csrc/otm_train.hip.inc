// One OTM training iteration behind the C ABI (SURVEY.md §8 rows A11 + A12 for OTM): LocalOptimizer.optimize's body for one batch
// (otm/src/main/scala/com/mass/otm/optim/LocalOptimizer.scala:55-109) —
//   targetNodes     = OTMTree.optimalPseudoTargets (otm/.../tree/OTMTree.scala:27-46, computeTargets :104-129, computeChildrenScores
//                     :131-165) or normalTargets (:50-63),
//   beamSearchNodes = OTMTree.beamSearchNodes (:67-91) with the weights fixed,
//   per level       : MiniBatch.batchTransform (otm/.../dataset/MiniBatch.scala:17-40) -> trainBatch (:111-131) -> syncGradients
//                     (:133-141; here dm_train_sync_gradients over the attached communicator) -> Adam.optimize —
// with every list on the device.  A user's target list at a level holds at most as many nodes as the user has target items (parents
// never outnumber children), so all levels share ONE CSR layout [target_off[u], target_off[u+1]) with a per-level count; the
// reference's List.find / groupMapReduce become linear scans over those few entries by the user's thread (first match, first
// appearance: the orders the reference's list operations produce; its HashMap-ordered `toList` is the one order that cannot be
// reproduced — the oracle and this file both keep first appearance, DESIGN.md).  computeTargets' quirk is kept: the fold walks the
// users from the right while `offset` counts from 0, so user u reads the predictions stored for the MIRRORED positions (:115-128).

struct OtmTgtParams {
  const int32_t *seq;        // [U][L] node ids, -1 = padding
  const unsigned *umask;     // [U] bit j: history position j is padding
  const int64_t *toff;       // [U + 1] CSR of the target lists (capacity per user)
  int64_t U;
  int L, use_mask;
  // children level (in)
  const int32_t *cnode; const double *clab; const int32_t *ccnt; const int64_t *coff;    // coff [U + 1]: exclusive scan of ccnt
  // rows of the two forwards (pos block, then neg block) and their results
  int32_t *codes, *rseq; unsigned *rmask; double *negl;
  const void *pred;          // [2 * total] in the model's element type
  // parent level (out)
  int32_t *pnode; double *plab; int32_t *pcnt;
};

__global__ void otm_umask_kernel(const int32_t *seq, int64_t U, int L, int use_mask, unsigned *umask) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  unsigned m = 0;
  if (use_mask) for (int j = 0; j < L; j++) if (seq[u * L + j] == -1) m |= 1u << j;      // sequenceBatchLabels: masks = paddingIdx positions
  umask[u] = m;
}

// leaf level: batchData.map(_.targetItems.map(Node(_, 1.0)))  (OTMTree.scala:38)
__global__ void otm_tgt_leaf_kernel(const int64_t *toff, const int32_t *targets, int64_t U, int32_t *node, double *lab, int32_t *cnt) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t b = toff[u], n = toff[u + 1] - b;
  for (int64_t i = 0; i < n; i++) { node[b + i] = targets[b + i]; lab[b + i] = 1.0; }
  cnt[u] = (int32_t)n;
}
// normalTargets (:50-63): every level holds the ancestors of the target items, label 1 (no grouping)
__global__ void otm_tgt_normal_kernel(const int64_t *toff, int64_t U, const int32_t *cnode, const int32_t *ccnt, int32_t *pnode, double *plab, int32_t *pcnt) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t b = toff[u];
  const int n = ccnt[u];
  for (int i = 0; i < n; i++) { pnode[b + i] = (cnode[b + i] - 1) >> 1; plab[b + i] = 1.0; }
  pcnt[u] = n;
}

// exclusive scan of the per-user counts (one wave; a level has U counts)
__global__ void otm_scan_kernel(const int32_t *cnt, int64_t U, int64_t *off) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (U + 63) / 64, lo = lane * chunk, hi = lo + chunk < U ? lo + chunk : U;
  int64_t s = 0;
  for (int64_t i = lo; i < hi; i++) s += cnt[i];
  int64_t incl = s;
  for (int o = 1; o < 64; o <<= 1) { const int64_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  int64_t run = incl - s;
  for (int64_t i = lo; i < hi; i++) { off[i] = run; run += cnt[i]; }
  if (lane == 63) off[U] = incl;
}

// computeChildrenScores (:131-165), the part before the two forwards: positive rows, sibling rows, sibling labels
__global__ void otm_tgt_rows_kernel(OtmTgtParams p) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= p.U) return;
  const int64_t b = p.toff[u], c0 = p.coff[u], total = p.coff[p.U];
  const int n = p.ccnt[u];
  const unsigned m = p.use_mask ? p.umask[u] : 0u;
  for (int i = 0; i < n; i++) {
    const int32_t node = p.cnode[b + i];
    const int32_t sib = (node % 2 == 0) ? node - 1 : node + 1;
    double nl = 0.0;
    for (int j = 0; j < n; j++) if (p.cnode[b + j] == sib) { nl = p.clab[b + j]; break; }       // nodes.find(_.id == nn)
    const int64_t e = c0 + i;
    p.codes[e] = p.use_mask ? node : sib;      // without a mask the reference feeds negTensor to BOTH forwards (:155-157)
    p.codes[total + e] = sib;
    p.negl[e] = nl;
    for (int j = 0; j < p.L; j++) { const int32_t s = p.seq[u * p.L + j]; p.rseq[e * p.L + j] = s; p.rseq[(total + e) * p.L + j] = s; }
    p.rmask[e] = m; p.rmask[total + e] = m;
  }
}

// computeTargets' fold (:113-128): labels from the MIRRORED prediction positions, parents grouped in first-appearance order,
// sums clipped to [0, 1]
template <typename T>
__global__ void otm_tgt_reduce_kernel(OtmTgtParams p) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= p.U) return;
  const int64_t b = p.toff[u], total = p.coff[p.U];
  const int64_t offset = total - p.coff[u + 1];           // nodes of the users to the RIGHT of u: the fold's running offset
  const int n = p.ccnt[u];
  const T *pred = (const T *)p.pred;
  int m = 0;
  for (int i = 0; i < n; i++) {
    const int64_t idx = offset + i;
    const double label = pred[idx] >= pred[total + idx] ? p.clab[b + i] : p.negl[idx];
    const int32_t par = (p.cnode[b + i] - 1) >> 1;
    int j = 0;
    for (; j < m; j++) if (p.pnode[b + j] == par) break;
    if (j == m) { p.pnode[b + m] = par; p.plab[b + m] = label; m++; }
    else p.plab[b + j] = p.plab[b + j] + label;                                   // groupMapReduce(...)(_ + _)
  }
  for (int j = 0; j < m; j++) { const double v = p.plab[b + j]; p.plab[b + j] = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }   // clipValue
  p.pcnt[u] = m;
}

// MiniBatch.batchTransform (MiniBatch.scala:17-40): the level's candidates of every user in user order, label = the first target
// with that id, else 0
__global__ void otm_batch_kernel(const int32_t *seq, const unsigned *umask, const int64_t *toff, int64_t U, int L, const int32_t *tc,
                                 const int32_t *tn, int levels, int cap, int it, int n_lv, const int32_t *tnode, const double *tlab,
                                 const int32_t *tcnt, int32_t *codes, int32_t *rseq, unsigned *rmask, float *lab) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < U * n_lv; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = r / n_lv;
    const int slot = (int)(r - u * n_lv);
    const int32_t node = slot < tn[u * levels + it] ? tc[(u * levels + it) * cap + slot] : -1;
    codes[r] = node;
    if (rseq) {          // (null for the user-grouped training step: it reads the histories per user)
      for (int j = 0; j < L; j++) rseq[r * L + j] = seq[u * L + j];
      rmask[r] = umask[u];
    }
    double l = 0.0;
    const int64_t b = toff[u];
    const int n = tcnt[u];
    for (int j = 0; j < n; j++) if (tnode[b + j] == node) { l = tlab[b + j]; break; }
    lab[r] = (float)l;
  }
}

// device arena of the target lists and of computeTargets' scratch (shared by the training iteration and dm_otm_pseudo_targets)
struct OtmTgtArena {
  size_t o_seq, o_umask, o_toff, o_tin, o_tnode, o_tlab, o_tcnt, o_coff, o_ccodes, o_cseq, o_cmask, o_negl, o_pred, end, NTc;
  int levels;
  int64_t U;
  int32_t *tnode(char *A, int li) const { return (int32_t *)(A + o_tnode) + (size_t)li * NTc; }
  double *tlab(char *A, int li) const { return (double *)(A + o_tlab) + (size_t)li * NTc; }
  int32_t *tcnt(char *A, int li) const { return (int32_t *)(A + o_tcnt) + (size_t)li * (size_t)U; }
};
static OtmTgtArena otm_tgt_arena(int64_t U, int L, int64_t NT, int levels) {
  OtmTgtArena a{};
  a.NTc = (size_t)(NT > 0 ? NT : 1); a.levels = levels; a.U = U;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o_ = off; off += (bytes + 255) & ~(size_t)255; return o_; };
  a.o_seq = take((size_t)U * L * 4); a.o_umask = take((size_t)U * 4); a.o_toff = take((size_t)(U + 1) * 8); a.o_tin = take(a.NTc * 4);
  a.o_tnode = take((size_t)levels * a.NTc * 4); a.o_tlab = take((size_t)levels * a.NTc * 8); a.o_tcnt = take((size_t)levels * U * 4);
  a.o_coff = take((size_t)(U + 1) * 8); a.o_ccodes = take(2 * a.NTc * 4); a.o_cseq = take(2 * a.NTc * L * 4); a.o_cmask = take(2 * a.NTc * 4);
  a.o_negl = take(a.NTc * 8); a.o_pred = take(2 * a.NTc * 8);
  a.end = off;
  return a;
}

// uploads the batch and builds every level's target list bottom up (list index li <-> tree level start_level + 1 + li)
static int otm_targets_dev(dm_ctx *h, char *A, const OtmTgtArena &a, const int32_t *seq_codes, int L, const int64_t *target_off,
                           const int32_t *target_nodes, const dm_otm_train_opts *o, uint64_t *fwd_rows) {
  const int64_t U = a.U, NT = target_off[U];
  const int levels = a.levels;
  const bool f64 = h->dtype == DM_F64;
  int32_t *d_seq = (int32_t *)(A + a.o_seq), *d_tin = (int32_t *)(A + a.o_tin);
  unsigned *d_umask = (unsigned *)(A + a.o_umask);
  int64_t *d_toff = (int64_t *)(A + a.o_toff), *d_coff = (int64_t *)(A + a.o_coff);
  const unsigned GU = (unsigned)((U + 255) / 256);
  HIPCHK(h, hipMemsetAsync(A + a.o_tnode, 0xFF, (size_t)levels * a.NTc * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(A + a.o_tlab, 0, (size_t)levels * a.NTc * 8, h->stream));
  // DeepFM has no mask, and without one the reference feeds the sibling tensor to BOTH forwards (OTMTree.scala:156-161): posPreds(i) >=
  // negPreds(i) compares a value with itself, so every node keeps its own label unless the logit is NaN.  No forward is run: the fold
  // reads a zeroed prediction buffer
  const bool dfm = h->scorer_kind == DM_KIND_DEEPFM;
  if (dfm) HIPCHK(h, hipMemsetAsync(A + a.o_pred, 0, 2 * a.NTc * 8, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_seq, seq_codes, (size_t)U * L * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_toff, target_off, (size_t)(U + 1) * 8, hipMemcpyHostToDevice, h->stream));
  if (NT > 0) HIPCHK(h, hipMemcpyAsync(d_tin, target_nodes, (size_t)NT * 4, hipMemcpyHostToDevice, h->stream));
  LAUNCHCHK(h, otm_umask_kernel, dim3(GU), dim3(256), 0, d_seq, U, L, o->use_mask, d_umask);
  LAUNCHCHK(h, otm_tgt_leaf_kernel, dim3(GU), dim3(256), 0, d_toff, d_tin, U, a.tnode(A, levels - 1), a.tlab(A, levels - 1), a.tcnt(A, levels - 1));
  for (int li = levels - 1; li >= 1; li--) {
    if (o->target_mode == 1) {
      LAUNCHCHK(h, otm_tgt_normal_kernel, dim3(GU), dim3(256), 0, d_toff, U, a.tnode(A, li), a.tcnt(A, li), a.tnode(A, li - 1), a.tlab(A, li - 1), a.tcnt(A, li - 1));
      continue;
    }
    LAUNCHCHK(h, otm_scan_kernel, dim3(1), dim3(64), 0, a.tcnt(A, li), U, d_coff);
    int64_t total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, d_coff + U, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    OtmTgtParams p{};
    p.seq = d_seq; p.umask = d_umask; p.toff = d_toff; p.U = U; p.L = L; p.use_mask = o->use_mask;
    p.cnode = a.tnode(A, li); p.clab = a.tlab(A, li); p.ccnt = a.tcnt(A, li); p.coff = d_coff;
    p.codes = (int32_t *)(A + a.o_ccodes); p.rseq = (int32_t *)(A + a.o_cseq); p.rmask = (unsigned *)(A + a.o_cmask); p.negl = (double *)(A + a.o_negl);
    p.pred = A + a.o_pred; p.pnode = a.tnode(A, li - 1); p.plab = a.tlab(A, li - 1); p.pcnt = a.tcnt(A, li - 1);
    if (total > 0 && !dfm) {
      LAUNCHCHK(h, otm_tgt_rows_kernel, dim3(GU), dim3(256), 0, p);
      // computePreds (:167-172): posPreds and negPreds as one launch (a row's value does not depend on its batch)
      // (f32 histories of 17 .. 32 positions: the general forward — the MFMA rows kernel holds one 16-position score tile)
      const int rc = f64 ? (rows_fwd64_available(h, L) ? rows_fwd64(h, p.codes, p.rseq, p.rmask, 2 * total, L, (double *)(A + a.o_pred))      // (the matrix-pipe forward while training state exists)
                                                        : din_forward_t<double>(h, p.codes, p.rseq, p.rmask, 2 * total, L, (double *)(A + a.o_pred)))
                         : L > DM_MAXL ? din_forward_t<float>(h, p.codes, p.rseq, p.rmask, 2 * total, L, (float *)(A + a.o_pred))
                                       : din_rows_dev(h, p.codes, p.rseq, p.rmask, 2 * total, L, (float *)(A + a.o_pred));
      if (rc != DM_OK) return rc;
      if (fwd_rows) *fwd_rows += (uint64_t)(2 * total);
    }
    if (f64) LAUNCHCHK(h, otm_tgt_reduce_kernel<double>, dim3(GU), dim3(256), 0, p);
    else LAUNCHCHK(h, otm_tgt_reduce_kernel<float>, dim3(GU), dim3(256), 0, p);
  }
  return DM_OK;
}

// *agreed = level agreements this rank has taken part in (the caller completes the protocol when the call fails between two of them)
// dfm: the DeepFM scorer (dm_deepfm_otm_train_batch) — targets without a forward, the fused search of dfm_otm.hip.inc, the row step of
// dfm_train.hip.inc per level; one rank
static int otm_train_batch_impl(dm_ctx *h, bool dfm, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                                const dm_otm_train_opts *o, double *level_losses, int *n_levels, int *agreed, int *agree_total) {
  const std::string who = dfm ? "dm_deepfm_otm_train_batch" : "dm_otm_train_batch";
  int rc = dfm ? dfm_train_check(h, who.c_str(), false) : train_check(h, who.c_str());
  if (rc != DM_OK) return rc;
  if (!seq_codes || !target_off || !o || !level_losses || U <= 0 || L <= 0 || L > DM_PIPE_MAXL)
    return fail(h, DM_ERR_INVALID, who + ": bad arguments");
  if (dfm) {
    if ((rc = dfm_otm_check(h, who.c_str(), U, L, o->beam, o->leaf_level, o->use_mask)) != DM_OK) return rc;
    if (h->comm && h->comm->nranks > 1)
      return fail(h, DM_ERR_UNSUPPORTED, who + ": a communicator with " + std::to_string(h->comm->nranks) + " ranks is attached; the gradient exchange for DeepFM is not built");
    if ((rc = dfm_train_check(h, who.c_str(), true)) != DM_OK) return rc;
    // the row step's limits (dfm_train_fb_dev), before anything runs
    if (U * 2 * o->beam > (int64_t)DRT_MAX_ROWS || U * 2 * o->beam * (int64_t)(L + 1) >= ((int64_t)1 << 31))
      return fail(h, DM_ERR_UNSUPPORTED, who + ": a level's batch of U * 2 beam rows is too large for the DeepFM row step (at most 4 194 240 rows, and rows (L + 1) below 2^31): split the users");
  } else if ((rc = otm_check(h, U, L, o->beam, o->leaf_level, who.c_str())) != DM_OK) return rc;
  int start, start_level;
  level_start_int(o->beam, &start, &start_level);
  const int levels = o->leaf_level - start_level;
  if (levels < 1) return fail(h, DM_ERR_INVALID, who + ": the leaf level must lie below the beam's start level");
  *agree_total = levels;
  if (target_off[0] != 0) return fail(h, DM_ERR_INVALID, who + ": target_off[0] must be 0");
  for (int64_t u = 0; u < U; u++)
    if (target_off[u + 1] < target_off[u]) return fail(h, DM_ERR_INVALID, who + ": target_off must be non-decreasing");
  const int64_t NT = target_off[U];
  if (NT > 0 && !target_nodes) return fail(h, DM_ERR_INVALID, who + ": target_nodes is NULL");
  const int64_t leaf_lo = ((int64_t)1 << o->leaf_level) - 1, leaf_hi = ((int64_t)2 << o->leaf_level) - 2;
  for (int64_t i = 0; i < NT; i++)
    if (target_nodes[i] < leaf_lo || target_nodes[i] > leaf_hi) return fail(h, DM_ERR_INDEX, who + ": a target is not a node of the leaf level");
  if ((rc = check_table_ids(h, who.c_str(), "history code", seq_codes, U * L, -1)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_otm_stats &st = h->otm_stats;
  st = dm_otm_stats{};
  typedef std::chrono::steady_clock clk;
  auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  const bool f64 = h->dtype == DM_F64;
  const bool f64_search = use_f64_beam(h);
  // the fused f32 kernels hold one 16-position score tile: longer histories take the per-level pipeline, like dm_otm_beam_search*
  const bool pipe_search = f64_search || L > DM_MAXL;
  int cap = ((2 * o->beam + 15) / 16) * 16;
  if (cap < 32) cap = 32;
  SearchPlan pl{};
  if (!pipe_search && !dfm) {
    if ((rc = plan_search(h, o->beam, U, L, levels, false, &pl)) != DM_OK) return rc;
    cap = pl.cap;
  }
  // candidates per user and level: 2 (start + 1) at the beam's start, then 2 min(beam, previous) — a complete tree (OTMTree.scala:12-22)
  std::vector<int> n_lv((size_t)levels);
  int nprev = start + 1, n_max = 0;
  for (int it = 0; it < levels; it++) { const int nb = it == 0 ? nprev : std::min(o->beam, nprev); n_lv[(size_t)it] = 2 * nb; nprev = 2 * nb; n_max = std::max(n_max, 2 * nb); }
  const size_t tsz = f64_search ? 8 : 4;
  const OtmTgtArena ar = otm_tgt_arena(U, L, NT, levels);
  size_t off = ar.end;
  auto take = [&](size_t bytes) { size_t o_ = off; off += DevArena::up(bytes); return o_; };
  const size_t o_tc = take((size_t)U * levels * cap * 4), o_ts = take((size_t)U * levels * cap * tsz), o_tn = take((size_t)U * levels * 4),
               o_ids = take((size_t)U * 2 * o->beam * 4), o_sc = take((size_t)U * 2 * o->beam * 8), o_cnt = take((size_t)U * 4),
               o_bcodes = take((size_t)U * n_max * 4), o_bseq = take((size_t)U * n_max * L * 4), o_bmask = take((size_t)U * n_max * 4),
               o_blab = take((size_t)U * n_max * 4);
  char *A = nullptr;
  DevTemps t(h);
  if ((rc = t.alloc(A, off)) != DM_OK) return rc;
  int32_t *d_seq = (int32_t *)(A + ar.o_seq);
  unsigned *d_umask = (unsigned *)(A + ar.o_umask);
  int64_t *d_toff = (int64_t *)(A + ar.o_toff);
  auto tn_ = [&](int li) { return ar.tnode(A, li); };
  auto tl_ = [&](int li) { return ar.tlab(A, li); };
  auto tc_ = [&](int li) { return ar.tcnt(A, li); };
  // ---- targets, bottom up
  const auto t0 = clk::now();
  if ((rc = otm_targets_dev(h, A, ar, seq_codes, L, target_off, target_nodes, o, &st.target_rows)) != DM_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const auto t1 = clk::now();
  st.targets_s = secs(t0, t1);
  // ---- beam nodes with the weights fixed: the search's per-level trace IS beamSearchNodes
  int32_t *d_tc = (int32_t *)(A + o_tc), *d_tnn = (int32_t *)(A + o_tn), *d_ids = (int32_t *)(A + o_ids), *d_cnt = (int32_t *)(A + o_cnt);
  HIPCHK(h, hipMemsetAsync(d_tnn, 0, (size_t)U * levels * 4, h->stream));
  if (dfm) rc = dfm_otm_search_dev(h, d_seq, U, L, o->beam, o->leaf_level, d_ids, (float *)(A + o_sc), d_cnt, levels, cap, d_tc, (float *)(A + o_ts), d_tnn);
  else if (pipe_search) rc = otm64_search_dev(h, d_seq, U, L, o->beam, o->leaf_level, d_ids, f64_search ? (double *)(A + o_sc) : nullptr,
                                         f64_search ? nullptr : (float *)(A + o_sc), d_cnt, levels, cap, d_tc,
                                         f64_search ? (double *)(A + o_ts) : nullptr, f64_search ? nullptr : (float *)(A + o_ts), d_tnn);
  else rc = otm_search_dev(h, d_seq, U, L, o->beam, o->leaf_level, d_ids, (float *)(A + o_sc), d_cnt, levels, d_tc, (float *)(A + o_ts), d_tnn, pl, false);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const auto t2 = clk::now();
  st.beam_s = secs(t1, t2);
  // ---- per level: batch, forward / backward, exchange, Adam
  dm_comm *c = h->comm;
  const int W = c ? c->nranks : 1;
  int32_t *b_codes = (int32_t *)(A + o_bcodes), *b_seq = (int32_t *)(A + o_bseq);
  unsigned *b_mask = (unsigned *)(A + o_bmask);
  float *b_lab = (float *)(A + o_blab);
  // the level batch replicates a user's history over the user's candidates: the fp64 model trains on it user by user (train_grouped_f64.hip.inc)
  // ... and a DeepFM model under DM_DFM_TRAIN_GROUPED=1 (read per call; dfm_train_grouped.hip.inc).  The row step stays the default
  const bool grouped = dfm ? dfm_train_grouped_enabled() : f64 && L <= DM_MAXL && tg_enabled();
  for (int it = 0; it < levels; it++) {
    const int nl = n_lv[(size_t)it];
    const int64_t B = U * nl;
    const auto ta = clk::now();
    LAUNCHCHK(h, otm_batch_kernel, dim3((unsigned)std::min<int64_t>((B + 255) / 256, 8192)), dim3(256), 0, d_seq, d_umask, d_toff, U, L, d_tc, d_tnn, levels, cap, it, nl, tn_(it),
              tl_(it), tc_(it), b_codes, grouped ? (int32_t *)nullptr : b_seq, grouped ? (unsigned *)nullptr : b_mask, b_lab);
    float lf = 0.f;
    double ld = 0.0;
    if (dfm && grouped) rc = dfm_train_fb_grouped_dev(h, d_seq, nullptr, b_codes, b_lab, U, nl, 0, &ld);
    else if (dfm) rc = dfm_train_fb_dev(h, b_codes, b_seq, b_lab, B, &ld);      // (the row mask is unused: the graph has no mask input)
    else if (grouped) rc = train_fb_grouped_dev(h, d_seq, d_umask, b_codes, b_lab, U, nl, L, &lf);
    else rc = train_fb_dev(h, b_codes, b_seq, b_mask, b_lab, B, L, &lf);
    const auto tb = clk::now();
    double loss = dfm ? ld : h->last_loss;
    if (W > 1) {
      // one small all-reduce carries the ranks' status and their losses: a rank whose forward/backward failed tells the others BEFORE
      // anybody enters the gradient exchange (they would wait in it forever)
      double sl[2] = {rc != DM_OK ? 1.0 : 0.0, rc == DM_OK ? loss : 0.0};
      const int rc2 = dm_comm_allreduce_f64(c, sl, 2, 0);
      *agreed = it + 1;
      if (rc != DM_OK || rc2 != DM_OK || sl[0] > 0) *agreed = -1;          // everybody leaves here: no further agreement is owed
      if (rc != DM_OK) return rc;
      if (rc2 != DM_OK) return fail(h, rc2, c->err);
      if (sl[0] > 0) return fail(h, DM_ERR_STATE, "dm_otm_train_batch: a peer rank failed in its forward/backward; this rank left the level with it");
      if ((rc = dm_train_sync_gradients(h)) != DM_OK) { *agreed = -1; return rc; }
      loss = sl[1] / W;                             // totalLoss.sum / miniBatches.length (:130)
    } else if (rc != DM_OK) return rc;
    const auto tc2 = clk::now();
    if ((rc = dfm ? dm_deepfm_adam_step(h, 1.0f) : dm_adam_step(h, 1.0f / (float)W)) != DM_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const auto td = clk::now();
    level_losses[it] = loss;
    st.train_rows += (uint64_t)B;
    st.fwdbwd_s += secs(ta, tb); st.exchange_s += secs(tb, tc2); st.adam_s += secs(tc2, td);
  }
  if (n_levels) *n_levels = levels;
  st.levels = levels; st.users = (uint64_t)U;
  return DM_OK;
}

int dm_otm_train_batch(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                       const dm_otm_train_opts *opts, double *level_losses, int *n_levels) {
  if (!h) return DM_ERR_INVALID;
  int agreed = 0, total = 1, rc;
  try { rc = otm_train_batch_impl(h, false, seq_codes, U, L, target_off, target_nodes, opts, level_losses, n_levels, &agreed, &total); }
  catch (const std::exception &e) { rc = fail(h, DM_ERR_INVALID, std::string("dm_otm_train_batch: ") + e.what()); }
  // a data-parallel worker that failed OUTSIDE a level's agreement (validation, allocation, the beam search, the Adam step) still owes its
  // peers the next one: they are waiting in it.  (agreed == -1: everybody already left at an agreement; agreed == total: the peers are done.)
  if (rc != DM_OK && h->comm && h->comm->nranks > 1 && agreed >= 0 && agreed < total) {
    double sl[2] = {1.0, 0.0};
    (void)dm_comm_allreduce_f64(h->comm, sl, 2, 0);
  }
  return rc;
}

// the same iteration with a DeepFM model (OTMTrainDeepModel.scala:41-47 with deep_model DeepFM): needs dm_deepfm_train_init; one rank
int dm_deepfm_otm_train_batch(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                              const dm_otm_train_opts *opts, double *level_losses, int *n_levels) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_otm_train_batch");
  int agreed = 0, total = 1;
  try { return otm_train_batch_impl(h, true, seq_codes, U, L, target_off, target_nodes, opts, level_losses, n_levels, &agreed, &total); }
  catch (const std::exception &e) { return fail(h, DM_ERR_INVALID, std::string("dm_deepfm_otm_train_batch: ") + e.what()); }
}

// parity instrumentation: the target lists alone, downloaded — OTMTree.optimalPseudoTargets / normalTargets for a batch: out_nodes / out_labels [levels][NT] in the CSR of target_off,
// out_counts [levels][U]; level index li <-> tree level start_level + 1 + li.
static int otm_pseudo_targets_impl(dm_ctx *h, bool dfm, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                                   const dm_otm_train_opts *o, int32_t *out_nodes, double *out_labels, int32_t *out_counts) {
  const std::string who = dfm ? "dm_deepfm_otm_pseudo_targets" : "dm_otm_pseudo_targets";
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, who + ": weights not loaded");
  if (dfm) { const int rc_ = dfm_train_check(h, who.c_str(), false); if (rc_ != DM_OK) return rc_; }
  else DM_DIN_ONLY(h, who);
  if (!seq_codes || !target_off || !o || !out_nodes || !out_labels || !out_counts || U <= 0 || L <= 0 || L > DM_PIPE_MAXL)
    return fail(h, DM_ERR_INVALID, who + ": bad arguments");
  int rc = dfm ? dfm_otm_check(h, who.c_str(), U, L, o->beam, o->leaf_level, o->use_mask) : otm_check(h, U, L, o->beam, o->leaf_level, who.c_str());
  if (rc != DM_OK) return rc;
  int start, start_level;
  level_start_int(o->beam, &start, &start_level);
  const int levels = o->leaf_level - start_level;
  if (levels < 1 || target_off[0] != 0) return fail(h, DM_ERR_INVALID, who + ": bad levels / target_off");
  const int64_t NT = target_off[U];
  if ((rc = check_table_ids(h, who.c_str(), "target", target_nodes, NT, 1)) != DM_OK ||
      (rc = check_table_ids(h, who.c_str(), "history code", seq_codes, U * L, -1)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const OtmTgtArena ar = otm_tgt_arena(U, L, NT, levels);
  char *A = nullptr;
  DevTemps t(h);
  if ((rc = t.alloc(A, ar.end)) != DM_OK) return rc;
  if ((rc = otm_targets_dev(h, A, ar, seq_codes, L, target_off, target_nodes, o, nullptr)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(out_nodes, A + ar.o_tnode, (size_t)levels * ar.NTc * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out_labels, A + ar.o_tlab, (size_t)levels * ar.NTc * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out_counts, A + ar.o_tcnt, (size_t)levels * U * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_otm_pseudo_targets(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                          const dm_otm_train_opts *o, int32_t *out_nodes, double *out_labels, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  return otm_pseudo_targets_impl(h, false, seq_codes, U, L, target_off, target_nodes, o, out_nodes, out_labels, out_counts);
}
// with a DeepFM model: no forward runs (otm_targets_dev says why); every label of target_mode 0 is clip(sum of child labels, 0, 1)
int dm_deepfm_otm_pseudo_targets(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, const int64_t *target_off, const int32_t *target_nodes,
                                 const dm_otm_train_opts *o, int32_t *out_nodes, double *out_labels, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  return otm_pseudo_targets_impl(h, true, seq_codes, U, L, target_off, target_nodes, o, out_nodes, out_labels, out_counts);
}

// what the last dm_otm_train_batch / dm_deepfm_otm_train_batch on this handle did: out6 = users, levels, rows of the pseudo-target forwards, rows trained,
// 0, 0; secs5 = pseudo targets, beam search (fixed weights), forward / backward (incl. the batch kernel), exchange, Adam
int dm_otm_train_stats(dm_handle_t h, uint64_t *out6, double *secs5) {
  if (!h || !out6 || !secs5) return DM_ERR_INVALID;
  const dm_otm_stats &s = h->otm_stats;
  out6[0] = s.users; out6[1] = (uint64_t)s.levels; out6[2] = s.target_rows; out6[3] = s.train_rows; out6[4] = out6[5] = 0;
  secs5[0] = s.targets_s; secs5[1] = s.beam_s; secs5[2] = s.fwdbwd_s; secs5[3] = s.exchange_s; secs5[4] = s.adam_s;
  return DM_OK;
}
