// DeepFM node scorer (tdm/src/main/scala/com/mass/tdm/model/DeepFM.scala:11-45), serving half: the row forward and the scorer of the
// TDM level pipeline (tdm_pipeline.hip.inc).  fp32 only; the training step is not here.
//
// Model (T = L + 1 features of E values: the item row e, then the history rows k_1 .. k_L; -1 / padding = a zero row):
//   x      = [e ; k_1 ; .. ; k_L]                                            Concat(itemFlatten, seqFlatten), DeepFM.scala:26-34
//   fm     = (|sum_i x_i|^2 - sum_i |x_i|^2) / 2                              scalann/.../nn/FM.scala:24-37
//   logit  = fm + l2.W relu(l1.W x + l1.b) + l2.b                             Linear(T E, T), ReLU, Linear(T, 1), Add; DeepFM.scala:35-42
// Compact vector in Graph.parameters order (scalann/.../nn/graphnn/Graph.scala:37-48 walks the nodes in forward order: EmbeddingShare,
// DeepFM.scala:18; Linear, :35; Linear, :39 — FM, Reshape, Concat, ReLU and Add hold no parameters):
//   [emb num_index x E ; l1.W T x (T E) ; l1.b T ; l2.W 1 x T ; l2.b 1]       n = num_index E + T T E + 2 T + 1
// On the device every E-wide block (the table's rows, the T column blocks of every l1.W row) is zero-padded to Ep = 16 / 32 / 64 / 128
// like the DIN loader's: zero columns add nothing to a dot product, to |s|^2 or to sum |k|^2.
//
// Per user (shared by every row scored for that user): W1a = l1.W[:, :E], W1s = l1.W[:, E:]
//   s = sum_j k_j          c = (|s|^2 - sum_j |k_j|^2) / 2 + l2.b          a = W1s vec(K) + l1.b   (T values)
//   logit(e) = e.s + c + sum_t l2.W[t] relu(W1a[t].e + a[t])
// since |e + s|^2 - |e|^2 - sum |k_j|^2 = 2 e.s + |s|^2 - sum |k_j|^2.  A level of the search is therefore ONE product per user,
// [children x E] . [E x (T + 1)]: column 0 is the user's s, columns 1 .. T are W1a (shared by all users), padded to 16 / 32 / 48.
//
// Every kernel that evaluates this form calls the same device functions, defined here once:
//   dfm_user_setup         (s, c, a) of one user by one workgroup of 1, 2 or 4 waves: dfm_user_kernel, dfm_otm_beam_kernel (dfm_otm.hip.inc)
//   dfm_stage_frag         W1a's B fragments (and w2p) into LDS, once per workgroup; dfm_frag_bytes: their size, in HBM and in LDS
//   dfm_tile_gather        16 node rows HBM -> VGPR in A-fragment layout
//   dfm_tile_score         the product, the epilogue and the row sums of a 16-row tile: dfm_level_kernel, dfm_otm_beam_kernel
// (dfm_jtm_pairs_kernel, dfm_jtm.hip.inc, shares the staging and the gather and restates the product: see there)
// so a (row, user) pair gets the same bytes from each of them (tests/test_gpu_deepfm_shared_tile.py).
//
// Summation orders (fixed; no atomics on floats; two runs give the same bits):
//   s[e], sum_j k_j[e]^2   history order j = 0 .. L-1, one thread per feature
//   c                      d[e] = s[e]^2 - sum_j k_j[e]^2 per feature (the cancellation happens per feature, on small numbers), then the
//                          xor-shuffle tree over the 64 lanes: features 0 .. 63 and 64 .. 127 each through one wave-sum, whichever wave
//                          executes it; c = 0.5 (red0 + red1) + b2
//   a[t]                   lane-strided partial sums over vec(K) in index order, then the xor-shuffle tree
//   tile score             v_mfma_f32_16x16x4_f32 over k = 0 .. Ep-1 in steps of 4 (exact fp32 fma chain per output), the epilogue per column,
//                          column tiles added in order, then the xor-shuffle tree over the 16 lanes that hold a row's columns

#define DFM_MAXL 32

static int64_t deepfm_len_for(int64_t num_index, int64_t E, int64_t L) { const int64_t T = L + 1; return num_index * E + T * T * E + 2 * T + 1; }
static int dfm_col_tiles(int L) { return (L + 2 + 15) / 16; }      // ceil((T + 1) / 16): 1 for L <= 14, 2 for L <= 30, 3 up to 32

// ---- derived copies, from the compact vector on the device: W1a (and the zero column 0 / padding columns) as MFMA B fragments
// frag[ct][jc][lane = (g, r)][t] = M[col 16 ct + r][feature 16 jc + 4 g + t], M[0] = 0 (the user's s goes there), M[n] = W1a[n - 1] for
// n = 1 .. T, 0 beyond; w2p[n] = l2.W[n - 1] for n = 1 .. T, 0 elsewhere.
__global__ void dfm_derive_kernel(const float *l1_w, const float *l2_w, int E, int T, int NCT, float *frag, float *w2p) {
  const int NJ = E / 16, n = NCT * NJ * 256;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int t = i & 3, lane = (i >> 2) & 63, jc = (i >> 8) % NJ, ct = (i >> 8) / NJ;
    const int col = 16 * ct + (lane & 15), e = 16 * jc + 4 * (lane >> 4) + t;
    frag[i] = (col >= 1 && col <= T) ? l1_w[(int64_t)(col - 1) * T * E + e] : 0.0f;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < NCT * 16; i += gridDim.x * blockDim.x) w2p[i] = (i >= 1 && i <= T) ? l2_w[i - 1] : 0.0f;
}

// ---- W1s (the L history blocks of every l1.W row) as MFMA B fragments, for the per-history set-up of dfm_jtm.hip.inc:
// fragS[ct][j][jc][lane = (g, r)][t] = W1s[col 16 ct + r - 1][history position j][feature 16 jc + 4 g + t] for col = 1 .. T, 0 for column 0
// (c goes there) and beyond T: the column numbering of aux.  NCT L E 64 bytes.
__global__ void dfm_jtm_derive_kernel(const float *l1_w, int E, int L, int NCT, float *fragS) {
  const int NJ = E / 16, T = L + 1;
  const int64_t n = (int64_t)NCT * L * NJ * 256;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i & 3), lane = (int)(i >> 2) & 63;
    const int64_t blk = i >> 8;
    const int jc = (int)(blk % NJ), j = (int)((blk / NJ) % L), ct = (int)(blk / ((int64_t)NJ * L));
    const int col = 16 * ct + (lane & 15), e = 16 * jc + 4 * (lane >> 4) + t;
    fragS[i] = (col >= 1 && col <= T) ? l1_w[((int64_t)(col - 1) * T + 1 + j) * E + e] : 0.0f;
  }
}

// ---- per user: s [E], aux [NC]: aux[0] = c, aux[n] = a[n - 1] for n = 1 .. T, 0 beyond.  Called by every thread of a workgroup of nthr = 64,
// 128 or 256 threads for ONE user's L history codes (-1 or outside the table = a zero row).  K: LDS, L E floats, written before the first
// of the two barriers in here and read between them: dead only after the second, so between(), which runs just before it, must not
// touch K (the OTM kernel fills its frontier there and lets its sort overlap K afterwards).  S, aux, red (2 floats): global or LDS, the
// caller's choice; c is written after the second barrier.  No sum's order depends on nthr.
template <typename F>
__device__ __forceinline__ void dfm_user_setup(const float *emb, const float *l1_w, const float *l1_b, float b2, int64_t num_index, int E, int L, int NC,
                                               const int32_t *kcode, float *K, int nthr, float *S, float *aux, float *red, F between) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int T = L + 1, n = L * E;
  for (int i = tid; i < n; i += nthr) {
    const int32_t c = kcode[i / E];
    K[i] = (c >= 0 && c < num_index) ? emb[(int64_t)c * E + i % E] : 0.0f;
  }
  __syncthreads();
  for (int hf = wave; hf < 2; hf += nw) {      // features 0 .. 63, 64 .. 127 (E <= 128)
    const int e = 64 * hf + lane;
    float d = 0.0f;
    if (e < E) {
      float s = 0.0f, q = 0.0f;
      for (int j = 0; j < L; j++) { const float v = K[j * E + e]; s += v; q = fmaf(v, v, q); }
      S[e] = s;
      d = fmaf(s, s, -q);
    }
    d = dm_wave_sum(d);
    if (lane == 0) red[hf] = d;
  }
  for (int t = wave; t < T; t += nw) {
    const float *w = l1_w + (int64_t)t * T * E + E;      // W1s[t]: the L history blocks of row t
    float part = 0.0f;
    for (int i = lane; i < n; i += 64) part = fmaf(w[i], K[i], part);
    part = dm_wave_sum(part);
    if (lane == 0) aux[1 + t] = part + l1_b[t];
  }
  for (int i = T + 1 + tid; i < NC; i += nthr) aux[i] = 0.0f;
  between();
  __syncthreads();
  if (tid == 0) aux[0] = 0.5f * (red[0] + red[1]) + b2;
}

// One workgroup of 256 per user: S [U][E], aux [U][NC].
struct DfmUser {
  const float *emb, *l1_w, *l1_b;      // l1_w [T][T E]
  float b2;
  const int32_t *kcode;                // [U][L], -1 = zero row
  int E, L, NC;
  int64_t num_index;
  float *S, *aux;
};

__global__ __launch_bounds__(256) void dfm_user_kernel(DfmUser p) {
  __shared__ float K[DFM_MAXL * 128];
  __shared__ float red[2];
  const int64_t u = blockIdx.x;
  dfm_user_setup(p.emb, p.l1_w, p.l1_b, p.b2, p.num_index, p.E, p.L, p.NC, p.kcode + u * p.L, K, 256, p.S + u * p.E, p.aux + u * p.NC, red, [] {});
}

// ---- the 16-row tile.  One wave scores 16 rows against [s ; W1a] (T + 1 columns, padded to NCT tiles of 16).  The rows go HBM -> VGPR
// straight into A-fragment layout (lane (g, r): row r, features 16 jc + 4 g .. + 3 as one float4 per jc: k-step (jc, t) of the MFMA takes
// feature 16 jc + 4 g + t from lane group g — the B fragments above follow the same map); W1a's fragments are staged once per workgroup
// in LDS (NCT E 64 bytes: 24 KB at E = 128, L = 32) and read back as one conflict-free ds_read_b128 per lane and (ct, jc).
// C layout: lane (g, r) holds rows 4 g .. 4 g + 3 of column 16 ct + r.
static size_t dfm_frag_bytes(int E, int NCT) { return (size_t)NCT * E * 64; }

// frag [NCT][E / 16][64] -> wl, and w2p [NCT * 16] -> w2l where the caller keeps it in LDS (else null); the caller's barrier follows
template <int E, int NCT>
__device__ __forceinline__ void dfm_stage_frag(const f32x4 *frag, f32x4 *wl, const float *w2p, float *w2l, int nthr) {
  for (int i = threadIdx.x; i < NCT * (E / 16) * 64; i += nthr) wl[i] = frag[i];
  if (w2l)
    for (int i = threadIdx.x; i < NCT * 16; i += nthr) w2l[i] = w2p[i];
}

// row `code` of the table for lane (g, .); a code < 0 or >= num_index is a zero row.  next(jc, row) runs behind the load of qa[jc], row =
// "not a zero row": what a caller reads per feature block beside the row (the level kernel's s, the pair kernel's e.s) keeps its place
// between the gathers.
struct DfmNothing { __device__ __forceinline__ void operator()(int, bool) const {} };

template <int E, typename F = DfmNothing>
__device__ __forceinline__ void dfm_tile_gather(const float *emb, int32_t code, int64_t num_index, int g, f32x4 (&qa)[E / 16], F next = F{}) {
  if (code >= num_index) code = -1;
#pragma unroll
  for (int jc = 0; jc < E / 16; jc++) {
    qa[jc] = code >= 0 ? *(const f32x4 *)(emb + (int64_t)code * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
    next(jc, code >= 0);
  }
}

// tot[rr] = sum over the columns of  col == 0 ? x : w2[col] relu(x),  x = (row . column) + aux(rr, col),  for rows 4 g + rr of the tile, in
// every lane (g, .).  b0(jc, staged) is the B fragment of column tile 0: *staged (DfmStagedB0) where column 0 is W1a's zero column, and
// with the lanes r = 0 holding the user's s (features 16 jc + 4 g ..) where it is the user's.  aux(rr, col): aux[user of row 4 g + rr][col].
struct DfmStagedB0 { __device__ __forceinline__ f32x4 operator()(int, const f32x4 *staged) const { return *staged; } };

template <int E, int NCT, typename B0, typename Aux>
__device__ __forceinline__ void dfm_tile_score(const f32x4 (&qa)[E / 16], const f32x4 *wl, const float *w2, int lane, B0 b0, Aux aux, float (&tot)[4]) {
  constexpr int NJ = E / 16;
  const int r = lane & 15;
#pragma unroll
  for (int rr = 0; rr < 4; rr++) tot[rr] = 0.0f;
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      const f32x4 *staged = wl + (ct * NJ + jc) * 64 + lane;
      const f32x4 b = ct == 0 ? b0(jc, staged) : *staged;
#pragma unroll
      for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[jc][t], b[t], acc, 0, 0, 0);
    }
    const int col = 16 * ct + r;
    const float wv = w2[col];
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const float x = acc[rr] + aux(rr, col);
      tot[rr] += col == 0 ? x : wv * fmaxf(x, 0.0f);
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) tot[rr] += __shfl_xor(tot[rr], o);
  }
}

// ---- one level: sc[u][row] for the rows < counts[u] of cur[u][stride].  One wave per (user, 16-row tile); column 0 of tile 0 is the
// user's s, held by the lanes r = 0.
struct DfmLevel {
  const float *emb;
  const f32x4 *frag;                   // [NCT][E / 16][64]
  const float *w2p;                    // [NCT * 16]
  const float *S, *aux;                // [U][E], [U][NCT * 16]
  const int32_t *codes, *counts;       // [U][stride], [U]
  float *sc;                           // [U][stride]
  int stride;
  int64_t U, num_index;
};

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_level_kernel(DfmLevel p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem_dfm[];
  f32x4 *wl = (f32x4 *)smem_dfm;
  dfm_stage_frag<E, NCT>(p.frag, wl, nullptr, nullptr, 256);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int tpu = p.stride / 16;
  const int64_t total = p.U * tpu;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < total; w += (int64_t)gridDim.x * 4) {
    const int64_t u = w / tpu;
    const int row0 = (int)(w % tpu) * 16;
    const int n = min(p.counts[u], p.stride);
    if (row0 >= n) continue;           // (wave-uniform) rows at or past counts[u] are neither gathered nor stored
    f32x4 qa[NJ], sf[NJ];
    dfm_tile_gather<E>(p.emb, row0 + r < n ? p.codes[u * p.stride + row0 + r] : -1, p.num_index, g, qa, [&](int jc, bool) {
      sf[jc] = r == 0 ? *(const f32x4 *)(p.S + u * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
    });
    // (the select per component: given a whole-vector select the compiler sinks the LDS read under it, behind a branch of its own per jc,
    // and the MFMAs wait for every read; the parent's ISA, which this form reproduces, reads ahead in pairs)
    const auto b0 = [&](int jc, const f32x4 *staged) {
      const f32x4 b = *staged;
      return (f32x4){r == 0 ? sf[jc][0] : b[0], r == 0 ? sf[jc][1] : b[1], r == 0 ? sf[jc][2] : b[2], r == 0 ? sf[jc][3] : b[3]};
    };
    float tot[4];
    dfm_tile_score<E, NCT>(qa, wl, p.w2p, lane, b0, [&](int, int col) { return p.aux[u * NC + col]; }, tot);
    if (r == 0) {
#pragma unroll
      for (int rr = 0; rr < 4; rr++)
        if (row0 + 4 * g + rr < n) p.sc[u * p.stride + row0 + 4 * g + rr] = tot[rr];
    }
  }
}

// ---- Module.forward(Table(item, seq)) for rows that each carry their own history: one wave per row, the direct formulation
// (FM over the T rows, then the two Linears), every sum lane-strided in index order + the xor-shuffle tree.
struct DfmFwd {
  const float *emb, *l1_w, *l1_b, *l2_w;
  float b2;
  const int32_t *codes, *seqs;
  int E, L;
  int64_t B;
  float *out;
};

__global__ __launch_bounds__(256) void dfm_forward_kernel(DfmFwd p) {
  extern __shared__ __attribute__((aligned(16))) char smem_dff[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = p.E, T = p.L + 1, n = T * E;
  float *x = (float *)smem_dff + (size_t)wave * n;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < p.B; row += (int64_t)gridDim.x * 4) {
    for (int i = lane; i < n; i += 64) {
      const int f = i / E;
      const int32_t c = f == 0 ? p.codes[row] : p.seqs[row * p.L + f - 1];
      x[i] = c >= 0 ? p.emb[(int64_t)c * E + i % E] : 0.0f;
    }
    __builtin_amdgcn_wave_barrier();
    float d = 0.0f;
    for (int e = lane; e < E; e += 64) {
      float s = 0.0f, q = 0.0f;
      for (int f = 0; f < T; f++) { const float v = x[f * E + e]; s += v; q = fmaf(v, v, q); }
      d += fmaf(s, s, -q);
    }
    float logit = 0.5f * dm_wave_sum(d) + p.b2;
    for (int t = 0; t < T; t++) {
      const float *w = p.l1_w + (int64_t)t * n;
      float part = 0.0f;
      for (int i = lane; i < n; i += 64) part = fmaf(w[i], x[i], part);
      const float hsum = dm_wave_sum(part) + p.l1_b[t];
      logit += p.l2_w[t] * fmaxf(hsum, 0.0f);
    }
    if (lane == 0) p.out[row] = logit;
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------ host
// device layout of the small blocks behind the table (padded E)
struct DfmBlocks { const float *l1_w, *l1_b, *l2_w, *l2_b; };
static DfmBlocks dfm_blocks(const dm_ctx *h) {
  const int64_t E = h->embed, T = h->dfm_L + 1;
  DfmBlocks b;
  b.l1_w = (const float *)h->d_compact + h->num_index * E; b.l1_b = b.l1_w + T * T * E; b.l2_w = b.l1_b + T; b.l2_b = b.l2_w + T;
  return b;
}

// model layout (E) <-> device layout (Ep): the table's rows and the T column blocks of every l1.W row
static void dfm_repad(const float *src, int E_src, int E_dst, int64_t NI, int L, float *dst) {
  const int64_t T = L + 1;
  const int Ec = E_src < E_dst ? E_src : E_dst;
  memset(dst, 0, (size_t)deepfm_len_for(NI, E_dst, L) * 4);
  for (int64_t r = 0; r < NI; r++) memcpy(dst + r * E_dst, src + r * E_src, (size_t)Ec * 4);
  const float *s_w = src + NI * E_src;
  float *d_w = dst + NI * E_dst;
  for (int64_t b = 0; b < T * T; b++) memcpy(d_w + b * E_dst, s_w + b * E_src, (size_t)Ec * 4);
  memcpy(d_w + T * T * E_dst, s_w + T * T * E_src, (size_t)(2 * T + 1) * 4);
}

int dm_load_weights_deepfm(dm_handle_t h, int dtype, int E, int L, int64_t num_index, const void *compact, int64_t n_elems) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_weights_deepfm");
  if (dtype == DM_F64) return fail(h, DM_ERR_UNSUPPORTED, "dm_load_weights_deepfm: DM_F32 only (the reference's DeepFM[Double] belongs to OTM, which this library serves with DIN)");
  if (dtype != DM_F32) return fail(h, DM_ERR_INVALID, "dm_load_weights_deepfm: dtype");
  if (!compact || num_index <= 0 || E < 1 || E > 128 || L < 1 || L > DFM_MAXL)
    return fail(h, DM_ERR_INVALID, "dm_load_weights_deepfm: bad arguments (E must be 1..128, L 1..32)");
  if (n_elems != deepfm_len_for(num_index, E, L))
    return fail(h, DM_ERR_INVALID, "dm_load_weights_deepfm: n_elems does not match the DeepFM layout for (E, L, num_index)");
  HIPCHK(h, hipSetDevice(h->device));
  const int Ep = native_embed(E);
  const float *w = (const float *)compact;
  std::vector<float> padded;
  if (Ep != E) {
    padded.resize((size_t)deepfm_len_for(num_index, Ep, L));
    dfm_repad(w, E, Ep, num_index, L, padded.data());
    w = padded.data();
  }
  const size_t bytes = (size_t)deepfm_len_for(num_index, Ep, L) * 4;
  free_weights(h);      // (also switches the handle back to "no scorer": a failed load leaves no half-DIN, half-DeepFM state)
  void *d = nullptr;
  ALLOC(h, d, bytes);
  if (hipMemcpy(d, w, bytes, hipMemcpyHostToDevice) != hipSuccess) { dm_release(d); return fail(h, DM_ERR_HIP, "dm_load_weights_deepfm: upload failed"); }
  h->d_compact = d; h->d_emb32 = (float *)d; h->dtype = DM_F32; h->embed = Ep; h->embed_log = E; h->num_index = num_index;
  h->scorer_kind = DM_KIND_DEEPFM; h->dfm_L = L;
  const int NCT = dfm_col_tiles(L);
  ALLOC(h, h->d_dfm_frag, dfm_frag_bytes(Ep, NCT));
  ALLOC(h, h->d_dfm_w2p, (size_t)NCT * 16 * 4);
  ALLOC(h, h->d_dfm_fragS, (size_t)NCT * L * Ep * 64);
  const DfmBlocks b = dfm_blocks(h);
  {
    int rc = LAUNCH(h, dfm_derive_kernel, dim3(32), dim3(256), 0, b.l1_w, b.l2_w, Ep, L + 1, NCT, h->d_dfm_frag, h->d_dfm_w2p);
    if (rc == DM_OK) rc = LAUNCH(h, dfm_jtm_derive_kernel, dim3(256), dim3(256), 0, b.l1_w, Ep, L, NCT, h->d_dfm_fragS);
    if (rc != DM_OK) return rc;
  }
  HIPCHK(h, hipMemcpyAsync(&h->b2, b.l2_b, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->w_loaded = true;
  return DM_OK;
}

int dm_get_scorer_kind(dm_handle_t h, int *kind, int *seq_len) {
  if (!h || !kind) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  *kind = h->scorer_kind;
  if (seq_len) *seq_len = h->scorer_kind == DM_KIND_DEEPFM ? h->dfm_L : 0;
  return DM_OK;
}

// the model's own layout (unpadded E) on the host: the checkpoint's payload
static int dfm_download_model(dm_ctx *h, std::vector<float> &out) {
  const int64_t NI = h->num_index;
  std::vector<float> dev((size_t)deepfm_len_for(NI, h->embed, h->dfm_L));
  HIPCHK(h, hipMemcpy(dev.data(), h->d_compact, dev.size() * 4, hipMemcpyDeviceToHost));
  out.resize((size_t)deepfm_len_for(NI, h->embed_log, h->dfm_L));
  dfm_repad(dev.data(), h->embed, h->embed_log, NI, h->dfm_L, out.data());
  return DM_OK;
}

// What every DeepFM entry point checks first (after the NULL check and its DM_CLONE_ENTER / DM_OWNER_ONLY): a DeepFM model is loaded, the
// caller asks for no mask (the graph has no mask input) and *L is the model's (L == nullptr: not known yet).  The one wording of these
// refusals.
static int dfm_check_L(dm_ctx *h, const char *who, int L) {
  if (L == h->dfm_L) return DM_OK;
  return fail(h, DM_ERR_INVALID, std::string(who) + ": L = " + std::to_string(L) + " but the model was built for seq_len " + std::to_string(h->dfm_L) + " (l1.W is sized by it)");
}
static int dfm_enter(dm_ctx *h, const char *who, const int *L, int use_mask) {
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": weights not loaded");
  if (h->scorer_kind != DM_KIND_DEEPFM)
    return fail(h, DM_ERR_STATE, std::string(who) + ": the loaded scorer is DIN (dm_load_weights_deepfm loads a DeepFM model; DIN trains through dm_train_*)");
  if (use_mask != 0) return fail(h, DM_ERR_INVALID, std::string(who) + ": the DeepFM graph has no mask input (use_mask must be 0; OTM.scala:14-22 serves it with useMask = false)");
  return L ? dfm_check_L(h, who, *L) : DM_OK;
}

int dm_deepfm_forward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, int64_t B, int L, float *logits) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  int rc = dfm_enter(h, "dm_deepfm_forward", &L, 0);
  if (rc != DM_OK) return rc;
  if (!codes || !seqs || !logits || B < 0) return fail(h, DM_ERR_INVALID, "dm_deepfm_forward: bad arguments");
  if (B == 0) return DM_OK;
  if ((rc = check_lookup_ids(h, codes, B, 1, "row")) != DM_OK || (rc = check_lookup_ids(h, seqs, B * L, L, "row")) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ReqArena ar(h);
  const size_t o_codes = ar.add((size_t)B * 4), o_seqs = ar.add((size_t)B * L * 4), o_out = ar.add((size_t)B * 4);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(ar.ptr<int32_t>(o_codes), codes, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(ar.ptr<int32_t>(o_seqs), seqs, (size_t)B * L * 4, hipMemcpyHostToDevice, h->stream));
  const DfmBlocks b = dfm_blocks(h);
  DfmFwd p;
  p.emb = h->d_emb32; p.l1_w = b.l1_w; p.l1_b = b.l1_b; p.l2_w = b.l2_w; p.b2 = h->b2;
  p.codes = ar.ptr<int32_t>(o_codes); p.seqs = ar.ptr<int32_t>(o_seqs); p.E = h->embed; p.L = L; p.B = B; p.out = ar.ptr<float>(o_out);
  const size_t lds = (size_t)4 * (L + 1) * h->embed * 4;      // at most 4 x 33 x 128 floats = 66 KB
  int64_t blocks = (B + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  if ((rc = LAUNCH_LDS(h, dfm_forward_kernel, dim3((unsigned)blocks), dim3(256), lds, p)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(logits, p.out, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

// ---- the level pipeline's scorer
template <int E, int NCT>
static int dfm_launch_level(dm_ctx *h, const DfmLevel &p) {
  const size_t lds = dfm_frag_bytes(E, NCT);
  const int64_t waves = p.U * (p.stride / 16);
  int64_t blocks = (waves + 3) / 4;
  if (blocks > (int64_t)h->n_cu * 4) blocks = (int64_t)h->n_cu * 4;
  if (blocks < 1) blocks = 1;
  return timed(h, EV_DFM_LEVEL, true, [&] { return LAUNCH(h, (dfm_level_kernel<E, NCT>), dim3((unsigned)blocks), dim3(256), lds, p); });
}

struct TdmPlDeepFM : TdmPlScorer {
  int E, L, NCT, stride = 0;
  float *S = nullptr, *aux = nullptr;
  explicit TdmPlDeepFM(const dm_ctx *h) : E(h->embed), L(h->dfm_L), NCT(dfm_col_tiles(h->dfm_L)) {}
  size_t o_s = 0, o_aux = 0;
  void layout(DevArena &ar, int64_t Uc, int stride_, int) override {
    stride = stride_;
    o_s = ar.add((size_t)Uc * E * 4); o_aux = ar.add((size_t)Uc * NCT * 16 * 4);
  }
  int attach(dm_ctx *, const DevArena &ar) override {
    S = ar.ptr<float>(o_s); aux = ar.ptr<float>(o_aux);
    return DM_OK;
  }
  int setup(dm_ctx *h, const int32_t *kcode, int64_t Un) override {
    const DfmBlocks b = dfm_blocks(h);
    DfmUser p;
    p.emb = h->d_emb32; p.l1_w = b.l1_w; p.l1_b = b.l1_b; p.b2 = h->b2; p.kcode = kcode; p.E = E; p.L = L; p.NC = NCT * 16;
    p.num_index = h->num_index; p.S = S; p.aux = aux;
    return timed(h, EV_DFM_USER, true, [&] { return LAUNCH(h, dfm_user_kernel, dim3((unsigned)Un), dim3(256), 0, p); });
  }
  int score(dm_ctx *h, const int32_t *cur, const int32_t *ncur, float *sc, int64_t Un) override {
    DfmLevel p;
    p.emb = h->d_emb32; p.frag = (const f32x4 *)h->d_dfm_frag; p.w2p = h->d_dfm_w2p; p.S = S; p.aux = aux; p.codes = cur; p.counts = ncur;
    p.sc = sc; p.stride = stride; p.U = Un; p.num_index = h->num_index;
    return dispatch_E_NCT(h, E, NCT, "unsupported embed size", [&](auto e, auto n) { return dfm_launch_level<decltype(e)::value, decltype(n)::value>(h, p); });
  }
};

// TDM beam search with a DeepFM model: every history length takes the level pipeline
static int dfm_pipeline_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, const dm_tdm_search_opts *o, int max_beam,
                            const int64_t *d_coff, const int32_t *d_cids, int32_t *d_ids, float *d_scores, int32_t *d_counts,
                            int trace_levels, int cap, int32_t *d_tc, float *d_ts, int32_t *d_tn) {
  snprintf(h->last_kernel, sizeof(h->last_kernel), "tdm level pipeline: dfm_level_kernel<%d, %d>", h->embed, dfm_col_tiles(h->dfm_L));
  TdmPlDeepFM dfm(h);
  return tdm_pl_fold(h, dfm, d_seq, U, L, o, max_beam, d_coff, d_cids, d_ids, d_scores, d_counts, trace_levels, cap, d_tc, d_ts, d_tn);
}
