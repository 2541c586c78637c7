// TDM beam search level by level: the level fold as a short pipeline of kernels over a batch of users, with the scorer as a parameter
// (TdmPlScorer below).  Two scorers use it: DIN for history lengths 17 .. 32 (this file) and DeepFM for every length (deepfm.hip.inc).
//
// The fused beam kernels (beam_kernel*.hip.inc) hold ONE 16-position score tile per candidate tile (DM_MAXL = 16); the reference has no
// such limit (scalann/.../nn/Attention.scala:34-53 takes any sequence length).  Longer histories therefore take this path: the same fold
// (Recommender._recommend, tdm/src/main/scala/com/mass/tdm/model/Recommender.scala:40-107; TDM.recommend, TDM.scala:17-22) level by level,
// scored with the per-user restructured DIN of DESIGN.md §3 in plain fp32 —
//   setup   history ids -> codes (TDMTree.idToCode, tdm/.../tree/TDMTree.scala:35-56), T1 = K att.W^T, G = T1 W1b^T + b1   (two GEMMs)
//   level   step: leaves of the frontier -> the user's leaf list (in order), stable sortBy(-pred).take(beam) when the non-leaves
//           outnumber the beam (else input order, Recommender.scala:74-87), existing children in beam order        (tdm_pl_step_kernel)
//           H1 = Q W1a^T over the children (gather GEMM), attention + epilogue per row (otm64_attn_kernel<float>)
//   final   leaf list, latest level first, consumed ids dropped, stable sortBy(-pred).take(topk)                   (tdm_pl_final_kernel)
// The sorts are rank-by-counting on unique 64-bit keys (descending score key, list position): exact, and cheap at frontier sizes.
// Integer logic and tie order are the fused kernels' (and the oracle's); scores meet the same fp32 tolerance.

struct TdmPlTree {
  const uint32_t *exists_bits, *leaf_bits;
  const int32_t *node_id, *id_to_code;
  int64_t n_slots, num_index;
  int32_t non_leaf_offset, max_code;
};

// TDMTree.idToCode for the history (Recommender.duplicateSequence, Recommender.scala:171,181): 0 / unknown -> -1 = a zero key row
__global__ void tdm_pl_keys_kernel(const int32_t *seq, int64_t n, TdmPlTree t, int32_t *kcode) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t id = seq[i];
    int32_t code;
    if (id == 0) code = -1;
    else if (id < t.non_leaf_offset && id >= 0 && t.id_to_code[id] >= 0) code = t.id_to_code[id];
    else {
      const int32_t d = (int32_t)((uint32_t)id - (uint32_t)t.non_leaf_offset);
      code = (d > t.max_code) ? -1 : d;
    }
    if (code < -1 || code >= t.num_index) code = -1;
    kcode[i] = code;
  }
}

struct TdmPlStep {
  TdmPlTree t;
  const int32_t *cur; const float *sc; const int32_t *cnt;     // frontier [U][stride], [U]
  int32_t *next; int32_t *next_cnt;                            // children [U][stride] (unused slots = code 0), [U]
  int32_t *lf_code; float *lf_score; int32_t *lf_pos; int32_t *lf_n;   // leaf list [U][lcap] (+ order key), [U]
  const int64_t *consumed_off;                                 // widened beams (Recommender.recommendItems, Recommender.scala:28-33) or null
  int stride, lcap, beam, topk, widen, it, n_iter, start, init;
  int64_t U;
  unsigned long long *scored_rows;                             // += children handed to the scorer (dm_last_scored_rows)
};

// ordered compaction helper of ONE wave: lanes with flag set get consecutive slots from *running (advanced by the wave's count)
__device__ __forceinline__ int tdm_pl_slot(bool flag, int &running) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63;
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  const int s = running + before;
  running += __popcll(m);
  return s;
}

// one workgroup (256 threads) per user; dynamic LDS: keys u64 [stride] | codes i32 [stride] | kept i32 [stride]
__global__ __launch_bounds__(256) void tdm_pl_step_kernel(TdmPlStep p) {
  extern __shared__ __attribute__((aligned(16))) char smem_t[];
  unsigned long long *key = (unsigned long long *)smem_t;
  int32_t *nlc = (int32_t *)(key + p.stride);
  int32_t *kept = nlc + p.stride;
  __shared__ int s_nl, s_nc;
  const int64_t u = blockIdx.x;
  const int tid = threadIdx.x;
  int32_t *next = p.next + u * p.stride;
  if (p.init) {
    // the first frontier: the existing codes of level floor(log2 beam), preds 0 (Recommender.scala:53-56)
    if (tid < 64) {
      int running = 0;
      for (int b = 0; b <= p.start; b += 64) {
        const int i = b + tid;
        const int64_t c = (int64_t)p.start + i;
        const bool ok = i <= p.start && p.n_iter > 0 && c < p.t.n_slots && dm_bit(p.t.exists_bits, c);
        const int s = tdm_pl_slot(ok, running);
        if (ok) next[s] = (int32_t)c;
      }
      if (tid == 0) { s_nc = running; p.next_cnt[u] = running; p.lf_n[u] = 0; }
    }
    __syncthreads();
    for (int i = s_nc + tid; i < p.stride; i += 256) next[i] = 0;
    return;
  }
  const int n = p.cnt[u];
  if (n == 0) {       // (a user whose fold has ended keeps an empty frontier)
    if (tid == 0) p.next_cnt[u] = 0;
    for (int i = tid; i < p.stride; i += 256) next[i] = 0;
    return;
  }
  int beam = p.beam;
  if (p.widen && p.consumed_off) {
    const int64_t w = ((p.consumed_off[u + 1] - p.consumed_off[u]) + p.topk) / 2;      // Recommender.scala:31
    if (w > beam) beam = (int)w;
  }
  const int32_t *cur = p.cur + u * p.stride;
  const float *sc = p.sc + u * p.stride;
  // (1) partition(isLeaf), both sides in candidate order (Recommender.scala:62-70)
  if (tid < 64) {
    int nl = 0, nleaf = p.lf_n[u];
    const int leaf0 = nleaf;
    for (int b = 0; b < n; b += 64) {
      const int i = b + tid;
      const bool valid = i < n;
      const int32_t c = valid ? cur[i] : 0;
      const float s = valid ? sc[i] : 0.0f;
      const bool leaf = valid && dm_bit(p.t.leaf_bits, c);
      const int sl = tdm_pl_slot(leaf, nleaf);
      const int sn = tdm_pl_slot(valid && !leaf, nl);
      if (leaf && sl < p.lcap) {
        const int64_t q = u * p.lcap + sl;
        p.lf_code[q] = c; p.lf_score[q] = s;
        // the reference's list has the LATEST level block first (leafNodes ++: levelInfo.leafNodes): order key = (blocks from the end, index)
        p.lf_pos[q] = (p.n_iter - 1 - p.it) * p.stride + (sl - leaf0);
      }
      if (valid && !leaf) { nlc[sn] = c; key[sn] = ((unsigned long long)dm_desc_key(s) << 32) | (unsigned)sn; }
    }
    if (tid == 0) { s_nl = nl; p.lf_n[u] = nleaf < p.lcap ? nleaf : p.lcap; }
  }
  __syncthreads();
  const int nl = s_nl;
  const int nb = nl < beam ? nl : beam;
  // (2) more non-leaves than the beam: stable sortBy(-pred).take(beam) (:74-84); otherwise the input order (:85-87)
  if (nl > beam) {
    for (int j = tid; j < nl; j += 256) {
      const unsigned long long kj = key[j];
      int rank = 0;
      for (int k = 0; k < nl; k++) rank += key[k] < kj ? 1 : 0;
      if (rank < nb) kept[rank] = nlc[j];
    }
  } else {
    for (int j = tid; j < nl; j += 256) kept[j] = nlc[j];
  }
  __syncthreads();
  // (3) children of the kept nodes in beam order, filtered by existence (:88-92)
  if (tid < 64) {
    int nc = 0;
    for (int b = 0; b < 2 * nb; b += 64) {
      const int k = b + tid;
      const bool valid = k < 2 * nb;
      const int64_t c = valid ? (int64_t)kept[k >> 1] * 2 + 1 + (k & 1) : 0;
      const bool ok = valid && c < p.t.n_slots && c < p.t.num_index && dm_bit(p.t.exists_bits, c);
      const int s = tdm_pl_slot(ok, nc);
      if (ok && s < p.stride) next[s] = (int32_t)c;
    }
    if (tid == 0) {
      s_nc = nc < p.stride ? nc : p.stride; p.next_cnt[u] = s_nc;
      if (s_nc) atomicAdd(p.scored_rows, (unsigned long long)s_nc);
    }
  }
  __syncthreads();
  for (int i = s_nc + tid; i < p.stride; i += 256) next[i] = 0;
}

// per-level trace of the scored children (dm_tdm_beam_search_trace): [U][levels][cap]
__global__ void tdm_pl_trace_kernel(const int32_t *codes, const float *sc, const int32_t *cnt, int stride, int64_t U, int64_t u0, int it,
                                    int levels, int cap, int32_t *tc, float *ts, int32_t *tn) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < U * stride; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = t / stride;
    const int i = (int)(t % stride);
    const int n = cnt[u];
    const int64_t tb = (u0 + u) * levels + it;
    if (i == 0) tn[tb] = n;
    if (i < n && i < cap) { tc[tb * cap + i] = codes[t]; ts[tb * cap + i] = sc[t]; }
  }
}

struct TdmPlFinal {
  const int32_t *node_id;
  const int32_t *lf_code; const float *lf_score; const int32_t *lf_pos; const int32_t *lf_n;
  unsigned long long *lf_key;           // [U][lcap] scratch
  const int64_t *consumed_off; const int32_t *consumed_ids;
  int32_t *out_ids; float *out_scores; int32_t *out_counts;
  int lcap, topk;
  int64_t U, u0;
};

// Recommender.scala:103-106 (drop consumed ids) then TDM.recommend's stable sortBy(-pred).take(topk) (TDM.scala:21)
__global__ __launch_bounds__(256) void tdm_pl_final_kernel(TdmPlFinal p) {
  __shared__ int s_kept;
  const int64_t u = blockIdx.x, gu = p.u0 + u;
  const int tid = threadIdx.x;
  const int n = p.lf_n[u];
  unsigned long long *key = p.lf_key + u * p.lcap;
  if (tid == 0) s_kept = 0;
  __syncthreads();
  const int64_t c0 = p.consumed_off ? p.consumed_off[gu] : 0, c1 = p.consumed_off ? p.consumed_off[gu + 1] : 0;
  int kept_local = 0;
  for (int i = tid; i < n; i += 256) {
    const int64_t q = u * p.lcap + i;
    const int32_t id = p.node_id[p.lf_code[q]];
    bool drop = false;
    for (int64_t c = c0; c < c1; c++) drop |= p.consumed_ids[c] == id;
    key[i] = drop ? ~0ull : (((unsigned long long)dm_desc_key(p.lf_score[q]) << 32) | (unsigned)p.lf_pos[q]);
    kept_local += drop ? 0 : 1;
  }
  if (kept_local) atomicAdd(&s_kept, kept_local);
  __syncthreads();
  const int kept = s_kept;
  const int nout = kept < p.topk ? kept : p.topk;
  for (int i = tid; i < n; i += 256) {
    const unsigned long long ki = key[i];
    if (ki == ~0ull) continue;
    int rank = 0;
    for (int k = 0; k < n; k++) rank += key[k] < ki ? 1 : 0;
    if (rank < nout) {
      const int64_t q = u * p.lcap + i;
      p.out_ids[gu * p.topk + rank] = p.node_id[p.lf_code[q]];
      p.out_scores[gu * p.topk + rank] = p.lf_score[q];
    }
  }
  if (tid == 0) p.out_counts[gu] = nout;
}

// ------------------------------------------------------------------------------------------------ host
// The scorer of the level fold: everything between "the users' history codes are known" and "sc[U][stride] holds the scores of
// cur[U][stride] (ncur[U] rows per user)".  Two hooks — setup once per pass of users, score once per level — plus the scorer's share of
// the pass's workspace.  The fold below owns the integer logic and never looks inside.
struct TdmPlScorer {
  virtual ~TdmPlScorer() {}
  virtual void layout(DevArena &ar, int64_t Uc, int stride, int L) = 0;            // add() the scorer's arrays to the pass's workspace
  virtual int attach(dm_ctx *h, const DevArena &ar) = 0;                           // after commit(); once per call, before any pass
  virtual int setup(dm_ctx *h, const int32_t *kcode, int64_t Un) = 0;              // kcode [Un][L]: history codes, -1 = a zero row
  virtual int score(dm_ctx *h, const int32_t *cur, const int32_t *ncur, float *sc, int64_t Un) = 0;
};

// The per-user restructured DIN of DESIGN.md §3 in plain fp32 (histories of 17 .. 32 positions): T1 = K att.W^T, G = T1 W1b^T + b1 per
// user; per level H1 = Q W1a^T over the children (gather GEMM), then attention + epilogue per row (otm64_attn_kernel<float>)
struct TdmPlDin : TdmPlScorer {
  int use_mask, E, L = 0, stride = 0;
  const float *base = nullptr, *att_w = nullptr, *l1_w = nullptr, *l1_b = nullptr, *l2_w = nullptr;
  const int32_t *kcode = nullptr;
  float *H1 = nullptr, *T1 = nullptr, *G = nullptr, *zero = nullptr;
  size_t o_h1 = 0, o_t1 = 0, o_g = 0, o_zero = 0;
  TdmPlDin(const dm_ctx *h, int use_mask_) : use_mask(use_mask_), E(h->embed) {}
  void layout(DevArena &ar, int64_t Uc, int stride_, int L_) override {
    L = L_; stride = stride_;
    o_h1 = ar.add((size_t)Uc * stride * E * 4); o_t1 = ar.add((size_t)Uc * L * E * 4); o_g = ar.add((size_t)Uc * L * E * 4); o_zero = ar.add(256);
  }
  int attach(dm_ctx *h, const DevArena &ar) override {
    base = (const float *)h->d_compact;
    att_w = base + h->num_index * E; l1_w = att_w + (int64_t)E * E; l1_b = l1_w + (int64_t)2 * E * E; l2_w = l1_b + E;
    H1 = ar.ptr<float>(o_h1); T1 = ar.ptr<float>(o_t1); G = ar.ptr<float>(o_g); zero = ar.ptr<float>(o_zero);
    HIPCHK(h, hipMemsetAsync(zero, 0, 256, h->stream));
    return DM_OK;
  }
  int setup(dm_ctx *h, const int32_t *kcode_, int64_t Un) override {
    kcode = kcode_;
    int rc;
    DrGemmParams<float> g{};
    g.A = base; g.lda = E; g.gidx = kcode; g.Lg = 1; g.E = E; g.B = att_w; g.ldb = E; g.bias = nullptr; g.zero = zero;
    g.C = T1; g.ldc = E; g.M = Un * L; g.N = E; g.Kd = E;
    if ((rc = dr_launch_gemm<float>(h, g)) != DM_OK) return rc;
    g.A = T1; g.gidx = nullptr; g.B = l1_w + E; g.ldb = 2 * E; g.bias = l1_b; g.C = G;
    return dr_launch_gemm<float>(h, g);
  }
  int score(dm_ctx *h, const int32_t *cur, const int32_t *ncur, float *sc, int64_t Un) override {
    int rc;
    DrGemmParams<float> q{};
    q.A = base; q.lda = E; q.gidx = cur; q.Lg = 1; q.E = E; q.B = l1_w; q.ldb = 2 * E; q.bias = nullptr; q.zero = zero;
    q.C = H1; q.ldc = E; q.M = Un * stride; q.N = E; q.Kd = E;
    if ((rc = dr_launch_gemm<float>(h, q)) != DM_OK) return rc;
    Otm64Attn<float> a{};
    a.emb = base; a.H1 = H1; a.G = G; a.w2 = l2_w; a.b2 = h->b2; a.scale = sm_scale32(h); a.codes = cur; a.seq = kcode; a.scores = sc;
    a.n = stride; a.stride = stride; a.L = L; a.E = E; a.U = Un; a.counts = ncur; a.use_mask = use_mask;
    return otm_pl_launch_attn<float>(h, a);
  }
};

// The level fold (Recommender._recommend + TDM.recommend) over passes of users, scored by `scorer`.
// d_seq [U][L] item ids on the device; outputs pre-filled by the caller (ids -1, scores 0, counts 0); trace [U][trace_levels][cap] or null
static int tdm_pl_fold(dm_ctx *h, TdmPlScorer &scorer, const int32_t *d_seq, int64_t U, int L, const dm_tdm_search_opts *o, int max_beam,
                       const int64_t *d_coff, const int32_t *d_cids, int32_t *d_ids, float *d_scores, int32_t *d_counts,
                       int trace_levels, int cap, int32_t *d_tc, float *d_ts, int32_t *d_tn) {
  const int E = h->embed;
  int start, level0;
  level_start_int(o->beam, &start, &level0);
  int n_iter = h->max_level - level0 + 1;
  if (n_iter < 0) n_iter = 0;
  int stride = 2 * (max_beam > start + 1 ? max_beam : start + 1);
  stride = (stride + 15) / 16 * 16;
  if ((size_t)stride * 16 > 128 * 1024) return fail(h, DM_ERR_UNSUPPORTED, "tdm beam search (level pipeline): beam too large for the level pipeline");
  const int lcap = h->leaves_at_max_only ? stride : stride * (n_iter > 0 ? n_iter : 1);
  int64_t Uc = ((int64_t)1 << 30) / ((int64_t)stride * E * 4);
  if (Uc < 1) Uc = 1;
  if (Uc > U) Uc = U;
  const size_t b_k = (size_t)Uc * L * 4, b_codes = (size_t)Uc * stride * 4, b_cnt = (size_t)Uc * 4, b_lf = (size_t)Uc * lcap * 4;
  DevArena ar(h->ws);
  const size_t o_k = ar.add(b_k), o_c0 = ar.add(b_codes), o_c1 = ar.add(b_codes), o_sc = ar.add(b_codes), o_n0 = ar.add(b_cnt), o_n1 = ar.add(b_cnt),
               o_lfn = ar.add(b_cnt), o_lfc = ar.add(b_lf), o_lfs = ar.add(b_lf), o_lfp = ar.add(b_lf), o_lfk = ar.add(2 * DevArena::up(b_lf));
  scorer.layout(ar, Uc, stride, L);
  int rc = ar.commit(h);
  if (rc != DM_OK) return rc;
  int32_t *kcode = ar.ptr<int32_t>(o_k), *c0 = ar.ptr<int32_t>(o_c0), *c1 = ar.ptr<int32_t>(o_c1), *n0 = ar.ptr<int32_t>(o_n0), *n1 = ar.ptr<int32_t>(o_n1);
  int32_t *lf_n = ar.ptr<int32_t>(o_lfn), *lf_code = ar.ptr<int32_t>(o_lfc), *lf_pos = ar.ptr<int32_t>(o_lfp);
  float *sc = ar.ptr<float>(o_sc), *lf_score = ar.ptr<float>(o_lfs);
  unsigned long long *lf_key = ar.ptr<unsigned long long>(o_lfk);
  if ((rc = scorer.attach(h, ar)) != DM_OK) return rc;
  HIPCHK(h, reset_search_counters(h, false));
  const size_t lds_step = (size_t)stride * 16;
  HIPCHK(h, lds_opt_in(tdm_pl_step_kernel, lds_step));          // once for the launches of every level below
  TdmPlTree t{h->d_exists, h->d_leaf, h->d_node_id, h->d_id_to_code, h->n_slots, h->num_index, h->non_leaf_offset, h->max_code};
  for (int64_t u0 = 0; u0 < U; u0 += Uc) {
    const int64_t Un = U - u0 < Uc ? U - u0 : Uc;
    LAUNCHCHK(h, tdm_pl_keys_kernel, dim3(256), dim3(256), 0, d_seq + u0 * L, Un * L, t, kcode);
    if ((rc = scorer.setup(h, kcode, Un)) != DM_OK) return rc;
    TdmPlStep sp{};
    sp.t = t; sp.lf_code = lf_code; sp.lf_score = lf_score; sp.lf_pos = lf_pos; sp.lf_n = lf_n;
    sp.consumed_off = d_coff ? d_coff + u0 : nullptr; sp.stride = stride; sp.lcap = lcap; sp.beam = o->beam; sp.topk = o->topk;
    sp.widen = (o->widen_consumed && d_coff) ? 1 : 0; sp.n_iter = n_iter; sp.start = start; sp.U = Un;
    sp.scored_rows = &h->d_ctr->rows;
    int32_t *cur = c0, *nxt = c1, *ncur = n0, *nnxt = n1;
    sp.init = 1; sp.next = cur; sp.next_cnt = ncur; sp.sc = sc;
    LAUNCHCHK(h, tdm_pl_step_kernel, dim3((unsigned)Un), dim3(256), lds_step, sp);
    HIPCHK(h, hipMemsetAsync(sc, 0, (size_t)Un * stride * 4, h->stream));
    sp.init = 0;
    for (int it = 0; it < n_iter; it++) {
      sp.it = it; sp.cur = cur; sp.cnt = ncur; sp.next = nxt; sp.next_cnt = nnxt;
      LAUNCHCHK(h, tdm_pl_step_kernel, dim3((unsigned)Un), dim3(256), lds_step, sp);
      std::swap(cur, nxt); std::swap(ncur, nnxt);
      if ((rc = scorer.score(h, cur, ncur, sc, Un)) != DM_OK) return rc;
      if (d_tn && it < trace_levels) {
        LAUNCHCHK(h, tdm_pl_trace_kernel, dim3(512), dim3(256), 0, cur, sc, ncur, stride, Un, u0, it, trace_levels, cap, d_tc, d_ts, d_tn);
      }
    }
    TdmPlFinal f{};
    f.node_id = h->d_node_id; f.lf_code = lf_code; f.lf_score = lf_score; f.lf_pos = lf_pos; f.lf_n = lf_n; f.lf_key = lf_key;
    f.consumed_off = d_coff; f.consumed_ids = d_cids; f.out_ids = d_ids; f.out_scores = d_scores; f.out_counts = d_counts;
    f.lcap = lcap; f.topk = o->topk; f.U = Un; f.u0 = u0;
    LAUNCHCHK(h, tdm_pl_final_kernel, dim3((unsigned)Un), dim3(256), 0, f);
    HIPCHK(h, hipStreamSynchronize(h->stream));      // the workspace is reused by the next pass
  }
  return DM_OK;
}

// the DIN route: histories of 17 .. 32 positions whose frontier does not fit the fused kernel's LDS
static int tdm_pipeline_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, const dm_tdm_search_opts *o, int max_beam,
                            const int64_t *d_coff, const int32_t *d_cids, int32_t *d_ids, float *d_scores, int32_t *d_counts,
                            int trace_levels, int cap, int32_t *d_tc, float *d_ts, int32_t *d_tn) {
  if (h->dtype != DM_F32)
    return fail(h, DM_ERR_UNSUPPORTED, "tdm beam search: history lengths 17..32 run in fp32 on an f32 model (an f64 model serves OTM searches of that length in fp64)");
  snprintf(h->last_kernel, sizeof(h->last_kernel), "tdm level pipeline (L > 16)");
  TdmPlDin din(h, o->use_mask ? 1 : 0);
  return tdm_pl_fold(h, din, d_seq, U, L, o, max_beam, d_coff, d_cids, d_ids, d_scores, d_counts, trace_levels, cap, d_tc, d_ts, d_tn);
}
