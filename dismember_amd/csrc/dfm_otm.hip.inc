// OTM beam search with the DeepFM scorer (examples/.../otm/OTMTrainDeepModel.scala:41-47 builds otm/.../model/DeepFM.scala:10-49;
// otm/.../model/OTM.scala:14-22,32,58 serves it with useMask = false): CandidateSearcher.beamSearch (otm/.../model/CandidateSearcher.scala:
// 58-80, buildBeamNodes :109-122) / OTMTree.beamSearchNodes (otm/.../tree/OTMTree.scala:67-91,174-212) as ONE launch.  fp32, like the loader.
//
// An OTM tree is complete: no existence test, no id -> code step, the same candidate count for every user on every level.  A scored row
// costs E (T + 1) MACs and one row gather (deepfm.hip.inc: logit(e) = e.s + c + sum_t l2.W[t] relu(W1a[t].e + a[t])), so a whole user —
// set-up, every level's prune / expand / score, the results — fits in one workgroup.  One workgroup per user, grid-stride over the users
// (they cost the same: a static assignment), no communication between workgroups; the only seams are __syncthreads.
//
// Per workgroup : W1a's B fragments (d_dfm_frag, [0 ; W1a ; 0]) and w2p staged in LDS (dfm_stage_frag).
// Per user      : dfm_user_setup (history rows into LDS, S[E], aux[0] = c, aux[1 .. T] = W1s vec(K) + b1), results kept in LDS; a -1 code
//                 and a code outside the table are zero rows.
// Frontier      : nodes 2^s - 1 .. 2^(s+1) - 2 with score 0, s = floor(log2 beam) (OTMTree.initializeBeam).
// Per level     : prune (first level: keep all; then otm64_sort_positions — the stable (Double.compare descending, position) order — and
//                 take min(beam, n)), expand (children 2c+1, 2c+2 in kept order), score (a wave takes the 16-row tiles wave, wave + nwaves, ..;
//                 dfm_tile_gather and dfm_tile_score with the user's S / aux and w2p in LDS; scores to LDS), emit (trace slot and,
//                 on the last level, the outputs, in expansion order: what the reference returns before OTM.recommend sorts).
// A user's scores depend on the user alone: not on batch mates, the grid, or which wave took which tile (a tile's arithmetic is a
// function of its 16 rows and the user's S / aux).  No atomics.
//
// LDS: fragments NCT E 64 | w2p | S | aux | red | codes A, codes B, scores (2 beam each) | max(history rows L E 4, sort pcap 12) bytes:
// the history rows are dead once S and aux exist, the sort starts after them.  beam <= 512 (pcap 1024): 61 KB at E = 128, L = 32.

#define DFM_OTM_MAX_BEAM 512

struct DfmOtm {
  const float *emb, *l1_w, *l1_b;      // l1_w [T][T E]
  float b2;
  const f32x4 *frag;                   // [NCT][E / 16][64]
  const float *w2p;                    // [NCT * 16]
  const int32_t *seq;                  // [U][L], -1 (or outside the table) = zero row
  int L, beam, leaf_level, start, level0, cap2;      // cap2 = 2 beam rounded up to 4: slots of the code / score arrays
  int64_t U, num_index;
  int32_t *out_ids; float *out_sc; int32_t *out_cnt;                               // [U][2 beam], [U]
  int32_t *tr_codes; float *tr_sc; int32_t *tr_cnt; int tr_levels, tr_cap;         // [U][tr_levels][tr_cap], [U][tr_levels] or null
  unsigned long long *rows; unsigned long long rows_total;                         // dm_last_scored_rows
};

static inline size_t dfm_otm_lds(int E, int NCT, int L, int cap2, int pcap) {
  const size_t un = std::max((size_t)L * E * 4, (size_t)pcap * 12);
  return dfm_frag_bytes(E, NCT) + (size_t)NCT * 16 * 4 * 2 + (size_t)E * 4 + 16 + (size_t)cap2 * 12 + ((un + 15) & ~(size_t)15);
}

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_otm_beam_kernel(DfmOtm p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem_dfo[];
  const int nthr = blockDim.x, nw = nthr >> 6;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int cap2 = p.cap2;
  f32x4 *wl = (f32x4 *)smem_dfo;
  float *w2l = (float *)(wl + NCT * NJ * 64);
  float *Sl = w2l + NC, *auxl = Sl + E, *red = auxl + NC;
  int32_t *cA = (int32_t *)(red + 4), *cB = cA + cap2;
  float *scl = (float *)(cB + cap2);
  char *un = (char *)(scl + cap2);
  float *K = (float *)un;
  unsigned long long *key = (unsigned long long *)un;
  const f32x4 *Sl4 = (const f32x4 *)Sl;
  dfm_stage_frag<E, NCT>(p.frag, wl, p.w2p, w2l, nthr);
  if (blockIdx.x == 0 && tid == 0) *p.rows = p.rows_total;
  for (int64_t u = blockIdx.x; u < p.U; u += gridDim.x) {
    __syncthreads();                   // the staging above; the last user's emit has read its codes and scores
    // ---- the user; the frontier goes in before the set-up's second barrier (the history rows are dead behind it: the sort takes their place)
    int n = p.start + 1;
    dfm_user_setup(p.emb, p.l1_w, p.l1_b, p.b2, p.num_index, E, p.L, NC, p.seq + u * p.L, K, nthr, Sl, auxl, red, [&] {
      for (int i = tid; i < n; i += nthr) { cA[i] = p.start + i; scl[i] = 0.0f; }
    });
    int32_t *cur = cA, *nxt = cB;
    for (int level = p.level0; level < p.leaf_level; level++) {
      // ---- prune + expand
      int nb = n;
      if (level == p.level0) {
        for (int i = tid; i < n; i += nthr) { const int32_t c = cur[i]; nxt[2 * i] = 2 * c + 1; nxt[2 * i + 1] = 2 * c + 2; }
      } else {
        nb = n < p.beam ? n : p.beam;
        int pc = 2;
        while (pc < n) pc <<= 1;
        unsigned *pos = (unsigned *)(key + pc);
        otm64_sort_positions<float>(key, pos, scl, n, pc);
        for (int i = tid; i < nb; i += nthr) { const int32_t c = cur[pos[i]]; nxt[2 * i] = 2 * c + 1; nxt[2 * i + 1] = 2 * c + 2; }
      }
      __syncthreads();                 // (also: aux[0] = c on the first level)
      { int32_t *t_ = cur; cur = nxt; nxt = t_; }
      n = 2 * nb;
      // ---- score: column 0 of tile 0 is the user's s, read from LDS by the lanes r = 0 (feature 16 jc + 4 g + t)
      for (int row0 = 16 * wave; row0 < n; row0 += 16 * nw) {
        f32x4 qa[NJ];
        dfm_tile_gather<E>(p.emb, row0 + r < n ? cur[row0 + r] : -1, p.num_index, g, qa);       // rows at or past the count are neither gathered nor stored
        float tot[4];
        dfm_tile_score<E, NCT>(qa, wl, w2l, lane, [&](int jc, const f32x4 *staged) { return *(r == 0 ? Sl4 + 4 * jc + g : staged); },
                               [&](int, int col) { return auxl[col]; }, tot);
        if (r == 0) {
#pragma unroll
          for (int rr = 0; rr < 4; rr++)
            if (row0 + 4 * g + rr < n) scl[row0 + 4 * g + rr] = tot[rr];
        }
      }
      __syncthreads();
      // ---- emit
      const int it = level - p.level0;
      if (p.tr_cnt && it < p.tr_levels) {
        const int64_t tb = u * p.tr_levels + it;
        for (int i = tid; i < n && i < p.tr_cap; i += nthr) { p.tr_codes[tb * p.tr_cap + i] = cur[i]; p.tr_sc[tb * p.tr_cap + i] = scl[i]; }
        if (tid == 0) p.tr_cnt[tb] = n;
      }
      if (level == p.leaf_level - 1) {
        for (int i = tid; i < 2 * p.beam; i += nthr) {
          p.out_ids[u * 2 * p.beam + i] = i < n ? cur[i] : -1;
          p.out_sc[u * 2 * p.beam + i] = i < n ? scl[i] : 0.0f;
        }
        if (tid == 0) p.out_cnt[u] = n;
      }
    }
    if (p.leaf_level <= p.level0) {      // no level to score: the frontier itself is the answer, scores 0 (as in the reference)
      for (int i = tid; i < 2 * p.beam; i += nthr) {
        p.out_ids[u * 2 * p.beam + i] = i < n ? cA[i] : -1;
        p.out_sc[u * 2 * p.beam + i] = 0.0f;
      }
      if (tid == 0) p.out_cnt[u] = n;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
template <int E, int NCT>
static int dfm_otm_launch(dm_ctx *h, const DfmOtm &p, int nthr, size_t lds) {
  HIPCHK(h, lds_opt_in(dfm_otm_beam_kernel<E, NCT>, lds));      // before the occupancy query, which is asked about the same LDS
  int occ = 0;
  HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)dfm_otm_beam_kernel<E, NCT>, nthr, lds));
  if (occ < 1) occ = 1;
  int64_t grid = std::min<int64_t>(p.U, (int64_t)h->n_cu * occ);      // every workgroup resident: equal users, equal shares
  if (const long long g_ = env_int("DM_DFM_OTM_GRID")) grid = std::min<int64_t>(g_, 65535);      // (tests: a second, partial round of the user loop)
  snprintf(h->last_kernel, sizeof(h->last_kernel), "dfm_otm_beam_kernel<%d, %d>", E, NCT);
  return timed(h, EV_DFM_OTM, true, [&] { return LAUNCH(h, (dfm_otm_beam_kernel<E, NCT>), dim3((unsigned)grid), dim3((unsigned)nthr), lds, p); });
}

// what every DeepFM OTM entry point checks first (after the NULL check and, for the searches, DM_CLONE_ENTER): dfm_enter, then the search's shape
static int dfm_otm_check(dm_ctx *h, const char *who, int64_t U, int L, int beam, int leaf_level, int use_mask) {
  const int rc = dfm_enter(h, who, &L, use_mask);
  if (rc != DM_OK) return rc;
  if (U < 0 || L <= 0 || L > DFM_MAXL || beam <= 0 || leaf_level <= 0 || leaf_level > 30)
    return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments (L must be 1..32)");
  if ((((int64_t)1) << (leaf_level + 1)) - 1 > h->num_index) return fail(h, DM_ERR_INDEX, std::string(who) + ": leaf level exceeds the embedding table");
  if (beam > DFM_OTM_MAX_BEAM) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": beam too large for the LDS sort (at most 512 with a DeepFM model)");
  return DM_OK;
}

// candidates of a user summed over the scored levels: 2 (start + 1) at the beam's start, then 2 min(beam, previous)
static int64_t dfm_otm_rows_per_user(int beam, int leaf_level) {
  int start, level0;
  level_start_int(beam, &start, &level0);
  int64_t rows = 0;
  int n = start + 1;
  for (int level = level0; level < leaf_level; level++) { const int nb = level == level0 ? n : std::min(beam, n); n = 2 * nb; rows += n; }
  return rows;
}

// d_seq [U][L] on the device; outputs on the device ([U][2 beam] ids / scores, [U] counts, every slot written); trace [U][max_levels][cap]
// (live slots only) when d_tn is given.  The arguments have passed dfm_otm_check.
static int dfm_otm_search_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, int beam, int leaf_level, int32_t *d_ids, float *d_sc,
                              int32_t *d_cnt, int max_levels, int cap, int32_t *d_tc, float *d_ts, int32_t *d_tn) {
  const int E = h->embed, NCT = dfm_col_tiles(L);
  const DfmBlocks b = dfm_blocks(h);
  DfmOtm p{};
  level_start_int(beam, &p.start, &p.level0);
  p.emb = h->d_emb32; p.l1_w = b.l1_w; p.l1_b = b.l1_b; p.b2 = h->b2; p.frag = (const f32x4 *)h->d_dfm_frag; p.w2p = h->d_dfm_w2p;
  p.seq = d_seq; p.L = L; p.beam = beam; p.leaf_level = leaf_level; p.cap2 = (2 * beam + 3) & ~3; p.U = U; p.num_index = h->num_index;
  p.out_ids = d_ids; p.out_sc = d_sc; p.out_cnt = d_cnt;
  p.tr_codes = d_tc; p.tr_sc = d_ts; p.tr_cnt = d_tn; p.tr_levels = d_tn ? max_levels : 0; p.tr_cap = cap;
  p.rows = &h->d_ctr->rows; p.rows_total = (unsigned long long)(U * dfm_otm_rows_per_user(beam, leaf_level));
  int pcap = 2;
  while (pcap < 2 * beam) pcap <<= 1;
  const size_t lds = dfm_otm_lds(E, NCT, L, p.cap2, pcap);
  const int tiles = (2 * beam + 15) / 16;
  const int nthr = tiles <= 1 ? 64 : tiles == 2 ? 128 : 256;      // 1, 2 or 4 waves
  return dispatch_E_NCT(h, E, NCT, "unsupported embed size", [&](auto e, auto n) { return dfm_otm_launch<decltype(e)::value, decltype(n)::value>(h, p, nthr, lds); });
}

// host-buffer front end of dm_deepfm_otm_beam_search[_trace]
static int dfm_otm_search_host(dm_ctx *h, const char *who, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level, int32_t *out_node_ids,
                               float *out_scores, int32_t *out_counts, int max_levels, int32_t *tc, float *ts, int32_t *tn) {
  int rc = dfm_otm_check(h, who, U, L, beam, leaf_level, 0);
  if (rc != DM_OK) return rc;
  if (U == 0) return DM_OK;          // an empty batch is not an error
  if (!seq_codes || !out_node_ids || !out_scores || !out_counts) return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  if ((rc = check_table_ids(h, who, "history code", seq_codes, U * L, -1)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  int cap;
  frontier_caps(beam, &cap, nullptr);
  ReqLayout lay(h, h->req, 2, U, (size_t)L * 4, (size_t)2 * beam, 4);
  if (tn) lay.trace(max_levels, cap, 4);
  if ((rc = lay.commit(out_node_ids, out_scores, out_counts, tc, ts, tn)) != DM_OK) return rc;
  HIPCHK(h, lay.upload(seq_codes));
  if (tn) HIPCHK(h, lay.clear_trace());
  if ((rc = dfm_otm_search_dev(h, lay.d<int32_t>(lay.SEQ), U, L, beam, leaf_level, lay.d<int32_t>(lay.IDS), lay.d<float>(lay.SCORES), lay.d<int32_t>(lay.COUNTS),
                               max_levels, cap, lay.d<int32_t>(lay.TC), lay.d<float>(lay.TS), lay.d<int32_t>(lay.TN))) != DM_OK) return rc;
  HIPCHK(h, lay.finish());
  return DM_OK;
}

int dm_deepfm_otm_beam_search(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level, int32_t *out_node_ids,
                              float *out_scores, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  return dfm_otm_search_host(h, "dm_deepfm_otm_beam_search", seq_codes, U, L, beam, leaf_level, out_node_ids, out_scores, out_counts, 0, nullptr, nullptr, nullptr);
}

int dm_deepfm_otm_beam_search_trace(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level, int32_t *out_node_ids,
                                    float *out_scores, int32_t *out_counts, int max_levels, int32_t *trace_codes, float *trace_scores,
                                    int32_t *trace_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (max_levels <= 0 || !trace_codes || !trace_scores || !trace_counts) return fail(h, DM_ERR_INVALID, "dm_deepfm_otm_beam_search_trace: bad trace arguments");
  return dfm_otm_search_host(h, "dm_deepfm_otm_beam_search_trace", seq_codes, U, L, beam, leaf_level, out_node_ids, out_scores, out_counts, max_levels,
                             trace_codes, trace_scores, trace_counts);
}

// device-resident request: history codes outside the table are treated as padding by the kernel (the host entry points reject them)
int dm_deepfm_otm_beam_search_dev(dm_handle_t h, const int32_t *d_seq_codes, int64_t U, int L, int beam, int leaf_level, int32_t *d_out_node_ids,
                                  float *d_out_scores, int32_t *d_out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  int rc = dfm_otm_check(h, "dm_deepfm_otm_beam_search_dev", U, L, beam, leaf_level, 0);
  if (rc != DM_OK) return rc;
  if (U == 0) return DM_OK;
  if (!d_seq_codes || !d_out_node_ids || !d_out_scores || !d_out_counts) return fail(h, DM_ERR_INVALID, "dm_deepfm_otm_beam_search_dev: NULL argument");
  HIPCHK(h, hipSetDevice(h->device));
  return dfm_otm_search_dev(h, d_seq_codes, U, L, beam, leaf_level, d_out_node_ids, d_out_scores, d_out_counts, 0, 0, nullptr, nullptr, nullptr);
}
