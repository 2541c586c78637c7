// DeepFM scorer of (training row, chain node) pairs: JTM tree learning with a DeepFM model (TreeLearning.aggregateWeights,
// jtm/src/main/scala/com/mass/jtm/optim/TreeLearning.scala:152-174, calls dlModel.forward on whatever graph the model file holds).
// fp32 only.  The algebra is deepfm.hip.inc's per-user form with one difference: the pairs of a 16-pair tile belong to several
// histories, so nothing per history can ride in the B operand.
//   per history (dfm_jtm_rows_kernel):  s = sum_j k_j      c = (|s|^2 - sum_j |k_j|^2) / 2 + l2.b      a = W1s vec(K) + l1.b
//   per pair    (dfm_jtm_pairs_kernel): logit = e.s + c + sum_t l2.W[t] relu(W1a[t].e + a[t])
// S [H][E] and aux [H][NCT 16] (aux[0] = c, aux[1 .. T] = a, 0 beyond) have dfm_user_kernel's layout.  history(pair) = pair / seq_div,
// as in din_rows_dev.  The pair kernel stages W1a's fragments and gathers its rows through deepfm.hip.inc (dfm_stage_frag,
// dfm_tile_gather) and keeps a product and epilogue of its own, a restatement of dfm_tile_score's with its orders: through
// dfm_tile_score itself the kernel measured 1.4 % slower (DESIGN.md section 15).  The per-history set-up is its own algorithm (MFMA
// over 16 histories), not dfm_user_setup.  The set-up results live for one slice of histories
// (DFM_JTM_SLICE), never for a catalogue.
//
// Summation orders (fixed; no atomics; a history's (s, c, a) depends on its L codes only and a pair's logit on its (code, history) only:
// neither on the tile mates, nor on the position in the tile, nor on seq_div or the slicing):
//   s[e], sum_j k_j[e]^2   history order j = 0 .. L-1, in the lane that holds feature e of the history
//   c                      d[e] = s[e]^2 - sum_j k_j[e]^2 per feature, added over the lane's 4 E/16 features in (jc, t) order, then lane
//                          groups g: xor 16, xor 32
//   a[t]                   v_mfma_f32_16x16x4_f32 over k = (j, jc, t) ascending: an exact fp32 fma chain per output; + l1.b[t] last
//   e.s                    fma chain over the lane's features in (jc, t) order, then xor 16, xor 32
//   W1a[t].e               v_mfma_f32_16x16x4_f32 over k = 0 .. E-1 in steps of 4
//   logit                  per column w2 relu(. + a) (column 0: c), column tiles added in order, the xor tree over the 16 lanes that hold a
//                          pair's columns (dfm_tile_score's orders, deepfm.hip.inc), + e.s last

#define DFM_JTM_SLICE ((int64_t)1 << 18)      // histories per set-up pass: 144 MB of s and aux at E = 128, L <= 14
// DM_DFM_JTM_SLICE=<positive integer>: histories per set-up pass, read per call like DM_JTM_MAX_PAIRS (tests: slice edges at sizes a test
// can afford); unset or invalid: DFM_JTM_SLICE
static int64_t dfm_jtm_slice() {
  const char *e = env_str("DM_DFM_JTM_SLICE");
  if (!e || !*e) return DFM_JTM_SLICE;
  char *end = nullptr;
  const long long v = strtoll(e, &end, 10);
  return (*end == 0 && v > 0 && v <= DFM_JTM_SLICE) ? (int64_t)v : DFM_JTM_SLICE;
}

// ---- per history: one wave per tile of 16 histories.  The history rows go HBM -> VGPR in A-fragment layout (lane (g, r): history r of
// the tile, features 16 jc + 4 g .. + 3 as one float4), one history position j at a time; W1s' fragments of position j come from L2
// (every wave reads the same NCT E 64 bytes per j; the whole copy is NCT L E 64 bytes and fits no LDS at L = 32).
struct DfmJtmRows {
  const float *emb;
  const f32x4 *fragS;                  // [NCT][L][E / 16][64]
  const float *l1_b;
  float b2;
  const int32_t *hcode;                // [H][L], -1 (or anything outside the table) = zero row
  int L;
  int64_t H, num_index;
  float *S, *aux;                      // [H][E], [H][NCT * 16]
};

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_jtm_rows_kernel(DfmJtmRows p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int L = p.L, T = L + 1;
  const int64_t tiles = (p.H + 15) / 16;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < tiles; w += (int64_t)gridDim.x * 4) {
    const int64_t hh = w * 16 + r;
    const bool live = hh < p.H;          // histories at or past H are neither gathered nor stored
    f32x4 s[NJ], q[NJ], acc[NCT];
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) { s[jc] = (f32x4){0.f, 0.f, 0.f, 0.f}; q[jc] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < L; j++) {
      int32_t code = live ? p.hcode[hh * L + j] : -1;
      if (code >= p.num_index) code = -1;
      const f32x4 *bj = p.fragS + (int64_t)j * NJ * 64 + lane;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 k = code >= 0 ? *(const f32x4 *)(p.emb + (int64_t)code * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; t++) { s[jc][t] += k[t]; q[jc][t] = fmaf(k[t], k[t], q[jc][t]); }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
          const f32x4 b = bj[((int64_t)ct * L * NJ + jc) * 64];
#pragma unroll
          for (int t = 0; t < 4; t++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(k[t], b[t], acc[ct], 0, 0, 0);
        }
      }
    }
    float d = 0.0f;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
#pragma unroll
      for (int t = 0; t < 4; t++) d += fmaf(s[jc][t], s[jc][t], -q[jc][t]);
    }
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    if (live) {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) *(f32x4 *)(p.S + hh * E + 16 * jc + 4 * g) = s[jc];
      if (g == 0) p.aux[hh * NC] = 0.5f * d + p.b2;
    }
    // C layout: lane (g, r) holds histories 4 g .. 4 g + 3 of column 16 ct + r; column 0 is c's (written above)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      const int col = 16 * ct + r;
      const float bias = (col >= 1 && col <= T) ? p.l1_b[col - 1] : 0.0f;
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int64_t h2 = w * 16 + 4 * g + rr;
        if (col != 0 && h2 < p.H) p.aux[h2 * NC + col] = acc[ct][rr] + bias;      // (columns past T: W1s' fragment is zero there)
      }
    }
  }
}

// ---- per pair: one wave per 16 consecutive pairs.  e.s is a VALU dot against S[history(pair)] (column 0 of the
// product is W1a's zero column here: tile mates have different histories); aux is read per C-layout row, aux[history(row)][column].
struct DfmJtmPairs {
  const float *emb;
  const f32x4 *frag;                   // [NCT][E / 16][64] (d_dfm_frag: column 0 zero, columns 1 .. T = W1a)
  const float *w2p;                    // [NCT * 16]
  const float *S, *aux;                // [ceil(P / seq_div)][E], [..][NCT * 16]
  const int32_t *codes;                // [P]
  float *out;                          // [P]
  int64_t P, num_index;
  int seq_div;
};

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_jtm_pairs_kernel(DfmJtmPairs p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem_dfj[];
  f32x4 *wl = (f32x4 *)smem_dfj;
  dfm_stage_frag<E, NCT>(p.frag, wl, nullptr, nullptr, 256);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int64_t tiles = (p.P + 15) / 16;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < tiles; w += (int64_t)gridDim.x * 4) {
    const int64_t pr = w * 16 + r;
    const bool live = pr < p.P;          // pairs at or past P are neither gathered nor stored
    const int32_t code = live ? p.codes[pr] : -1;
    const int64_t hh = live ? pr / p.seq_div : 0;
    f32x4 qa[NJ];
    float es = 0.0f;
    dfm_tile_gather<E>(p.emb, code, p.num_index, g, qa, [&](int jc, bool row) {
      if (!row) return;      // (a zero row: e.s = 0, S is not read)
      const f32x4 sv = *(const f32x4 *)(p.S + hh * E + 16 * jc + 4 * g);
#pragma unroll
      for (int t = 0; t < 4; t++) es = fmaf(qa[jc][t], sv[t], es);
    });
    es += __shfl_xor(es, 16);
    es += __shfl_xor(es, 32);            // e.s of pair r, in all four lane groups
    float tot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 b = wl[(ct * NJ + jc) * 64 + lane];
#pragma unroll
        for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[jc][t], b[t], acc, 0, 0, 0);
      }
      const int col = 16 * ct + r;
      const float wv = p.w2p[col];
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int64_t p2 = w * 16 + 4 * g + rr;
        const float av = p2 < p.P ? p.aux[(p2 / p.seq_div) * NC + col] : 0.0f;
        const float x = acc[rr] + av;
        tot[rr] += col == 0 ? x : wv * fmaxf(x, 0.0f);
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) tot[rr] += __shfl_xor(tot[rr], o);
      tot[rr] += __shfl(es, 4 * g + rr);         // lane 4 g + rr (group 0) holds e.s of pair 4 g + rr
    }
    if (r == 0) {
#pragma unroll
      for (int rr = 0; rr < 4; rr++)
        if (w * 16 + 4 * g + rr < p.P) p.out[w * 16 + 4 * g + rr] = tot[rr];
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// the two launches of the pair scorer: the per-history set-up (OTM tree construction, dfm_otm_tree.hip.inc, runs it on its own) and the pairs
template <int E, int NCT>
static int dfm_jtm_launch_rows(dm_ctx *h, const DfmJtmRows &r) {
  int64_t blocks = ((r.H + 15) / 16 + 3) / 4;
  if (blocks > (int64_t)h->n_cu * 8) blocks = (int64_t)h->n_cu * 8;
  return timed(h, EV_DFM_JTM_ROWS, true, [&] { return LAUNCH(h, (dfm_jtm_rows_kernel<E, NCT>), dim3((unsigned)blocks), dim3(256), 0, r); });
}
template <int E, int NCT>
static int dfm_jtm_launch_pairs(dm_ctx *h, const DfmJtmPairs &p) {
  int64_t blocks = ((p.P + 15) / 16 + 3) / 4;
  if (blocks > (int64_t)h->n_cu * 4) blocks = (int64_t)h->n_cu * 4;
  return timed(h, EV_DFM_JTM_PAIRS, true, [&] { return LAUNCH(h, (dfm_jtm_pairs_kernel<E, NCT>), dim3((unsigned)blocks), dim3(256), dfm_frag_bytes(E, NCT), p); });
}

// logits of P pairs on device buffers, asynchronous on the handle's stream: d_seqs holds ceil(P / seq_div) histories of CODES
static int dfm_pairs_dev(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, int64_t P, int L, float *d_out, int seq_div) {
  if (P <= 0) return DM_OK;
  if (h->scorer_kind != DM_KIND_DEEPFM || L != h->dfm_L || seq_div < 1) return fail(h, DM_ERR_STATE, "dfm_pairs_dev: no DeepFM model of this history length");
  const int E = h->embed, NCT = dfm_col_tiles(L), NC = NCT * 16;
  const int64_t H = (P + seq_div - 1) / seq_div, Hs = std::min<int64_t>(H, dfm_jtm_slice());
  const size_t o_aux = DevArena::up((size_t)Hs * E * 4);
  int rc = h->dfm_jtm_ws.reserve(h, o_aux + (size_t)Hs * NC * 4);
  if (rc != DM_OK) return rc;
  const DfmBlocks b = dfm_blocks(h);
  DfmJtmRows r;
  r.emb = h->d_emb32; r.fragS = (const f32x4 *)h->d_dfm_fragS; r.l1_b = b.l1_b; r.b2 = h->b2; r.L = L; r.num_index = h->num_index;
  r.S = (float *)h->dfm_jtm_ws.p; r.aux = (float *)((char *)h->dfm_jtm_ws.p + o_aux);
  DfmJtmPairs p;
  p.emb = h->d_emb32; p.frag = (const f32x4 *)h->d_dfm_frag; p.w2p = h->d_dfm_w2p; p.S = r.S; p.aux = r.aux; p.num_index = h->num_index;
  p.seq_div = seq_div;
  for (int64_t h0 = 0; h0 < H; h0 += Hs) {       // slices start on a history: a pair's tile mates change with the slicing, its logit does not
    const int64_t p0 = h0 * seq_div;
    r.hcode = d_seqs + h0 * L; r.H = std::min(Hs, H - h0);
    p.codes = d_codes + p0; p.out = d_out + p0; p.P = std::min(P - p0, r.H * seq_div);
    rc = dispatch_E_NCT(h, E, NCT, "unsupported embed size", [&](auto e, auto n) {
      const int r_ = dfm_jtm_launch_rows<decltype(e)::value, decltype(n)::value>(h, r);
      return r_ != DM_OK ? r_ : dfm_jtm_launch_pairs<decltype(e)::value, decltype(n)::value>(h, p);
    });
    if (rc != DM_OK) return rc;
  }
  return DM_OK;
}

// what every DeepFM tree-learning entry point checks first (after the NULL check and DM_CLONE_ENTER): dfm_enter (L < 0: not known yet), one rank
static int dfm_jtm_enter(dm_ctx *h, const char *who, int use_mask, int L) {
  const int rc = dfm_enter(h, who, L < 0 ? nullptr : &L, use_mask);
  if (rc != DM_OK) return rc;
  if (h->comm && h->comm->nranks > 1)
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": a communicator with " + std::to_string(h->comm->nranks) + " ranks is attached; DeepFM tree learning runs on one rank");
  return DM_OK;
}

int dm_deepfm_pairs_forward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, int64_t P, int L, int seq_div, float *logits) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  int rc = dfm_enter(h, "dm_deepfm_pairs_forward", &L, 0);
  if (rc != DM_OK) return rc;
  if (!codes || !seqs || !logits || P < 0 || seq_div < 1) return fail(h, DM_ERR_INVALID, "dm_deepfm_pairs_forward: bad arguments");
  if (P == 0) return DM_OK;
  const int64_t H = (P + seq_div - 1) / seq_div;
  if ((rc = check_lookup_ids(h, codes, P, 1, "pair")) != DM_OK || (rc = check_lookup_ids(h, seqs, H * L, L, "history")) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ReqArena ar(h);
  const size_t o_codes = ar.add((size_t)P * 4), o_seqs = ar.add((size_t)H * L * 4), o_out = ar.add((size_t)P * 4);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(ar.ptr<int32_t>(o_codes), codes, (size_t)P * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(ar.ptr<int32_t>(o_seqs), seqs, (size_t)H * L * 4, hipMemcpyHostToDevice, h->stream));
  if ((rc = dfm_pairs_dev(h, ar.ptr<int32_t>(o_codes), ar.ptr<int32_t>(o_seqs), P, L, ar.ptr<float>(o_out), seq_div)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(logits, ar.ptr<float>(o_out), (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}
