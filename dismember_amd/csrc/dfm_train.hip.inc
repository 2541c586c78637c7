// DeepFM node scorer, training half: one step of LocalOptimizer.trainBatch with the DeepFM graph (dm_deepfm_train_*, dm_deepfm_adam_step;
// DESIGN.md §12).  Reference: tdm/src/main/scala/com/mass/tdm/model/DeepFM.scala:11-45 (the graph), tdm/.../optim/LocalOptimizer.scala:139-162
// (trainBatch, useMask = false), scalann nn/{FM,Linear,ReLU,BCECriterionWithLogits}, scalann optim/Adam.scala:19-73.  fp32 only, as the loader.
//
// A batch is B rows (code[r], seq[r][0..L), y[r]), -1 = a zero row that receives no gradient, T = L + 1:
//   X[r]   = [emb[code] ; emb[seq_0] ; .. ; emb[seq_{L-1}]]          x_i = feature block i, i < T
//   buf    = sum_i x_i          fm = (|buf|^2 - sum_i |x_i|^2) / 2
//   zpre   = l1.W vec(X) + l1.b     h = relu(zpre)     z = fm + (l2.W.h + l2.b)
//   loss   = mean_r( max(z,0) - z y + log1p(exp(-|z|)) )              g_r = (sigmoid(z_r) - y_r) / B
//   dh     = g_r l2.W [zpre > 0]
//   g_l2b  = sum_r g_r     g_l2W = sum_r g_r h[r]     g_l1b = sum_r dh[r]     g_l1W = sum_r dh[r] (x) vec(X[r])
//   dX_i[r]= (dh[r] l1.W)_block i + g_r (buf[r] - x_i[r])             (FM.updateGradInput, scalann/.../nn/FM.scala:43-71)
//   g_emb[row] += dX_i[r] for every slot (r, i) that read `row`
//
// Kernels:
//   dfm_train_idx_kernel    [code ; seq] side by side as one [B x T] index array; an id outside [0, num_index) becomes -1
//   dfm_train_rows_kernel   one wave per 16-row tile, v_mfma_f32_16x16x4_f32.  Pass 1 gathers x_i straight into the A-fragment layout of
//                           dfm_level_kernel and adds x_i W1_i^T into H, buf and sum |x_i|^2 in the same loop; the epilogue (C layout) makes
//                           h, z, the loss, g and dh.  Pass 2 re-gathers x_i and computes dX_i^T = W1_i^T dH^T: its C layout IS the gather's
//                           layout (lane (g, r): row r, features 16 jn + 4 g ..), so g_r (buf - x_i) is added per lane and dX is stored as
//                           float4.  dH crosses from the C layout of pass 1 to the B operand of pass 2 through 3 KB of LDS per wave.
//                           Both fragment orders of l1.W are read through L2 (not staged in LDS) at every L.
//   dfm_train_sum_kernel    loss (double), g_l2b and g_l2W: per-workgroup partials added in workgroup order
//   drt_gemm_kernel<float>  g_l1W and g_l1b (the ones column): A = dH^T, B gathered through the index array, slabs of DRT_SLAB rows added in
//                           slab order by drt_slab_sum_kernel
//   drt_sort_slots + dfm_seg_chunks_kernel + dfm_seg_heads_kernel   g_emb: the sorted slots of a destination row are added in batch order, in
//                           chunks of at most 64 and then chunk by chunk (drt_seg_rows_kernel<float, true> clears the previous batch's rows)
// No floating-point atomics; every sum has a fixed order: the same state and batch give the same bytes.

struct dm_dfm_train {
  TrainVec vec;                              // over d_compact in its padded layout: rows = num_index, E = embed
  float *fragF = nullptr, *fragB = nullptr;  // l1.W in the two fragment orders of dfm_train_rows_kernel (dfm_train_derive_kernel)
  DevGrow ws, io;
  DevGrow sync;                              // staging of dm_deepfm_train_sync_gradients (dfm_train_sync.hip.inc): all ranks' blocks, their tails
  bool exchanged = false;                    // vec.grad holds the sum over ranks: until the next forward/backward or Adam step
};

static void dfm_train_release(dm_ctx *h) {
  dm_dfm_train *t = h->dfm_tr;
  if (!t) return;
  t->vec.release();
  dm_release(t->fragF, t->fragB);
  for (DevGrow *g : {&t->ws, &t->io, &t->sync}) g->release();
  delete t;
  h->dfm_tr = nullptr;
}

static int dfm_train_col_tiles(int L) { return (L + 1 + 15) / 16; }      // ceil(T / 16): 1 for L <= 15, 2 for L <= 31, 3 at 32
static inline bool dfm_time_launches() { return env_on("DM_DFM_TIME_LAUNCHES"); }

// ---------------------------------------------------------------------------------------------------------------- kernels
// The one statement of both fragment orders of l1.W [T][T E] (columns t >= T are zero), NJ = E / 16, lane = (g, r):
//   fragF[i][ct][jc][lane][c] = l1.W[16 ct + r][i E + 16 jc + 4 g + c]          B operand of  H   += x_i W1_i^T     (k = feature)
//   fragB[i][jn][kq][lane][c] = l1.W[4 (4 kq + c) + g][i E + 16 jn + r]         A operand of  dX_i^T = W1_i^T dH^T  (k = unit t)
__global__ void dfm_train_derive_kernel(const float *l1_w, int E, int T, int NCT, float *fragF, float *fragB) {
  const int NJ = E / 16;
  const int64_t n = (int64_t)T * NCT * NJ * 256;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i & 3), lane = (int)((i >> 2) & 63), r = lane & 15, g = lane >> 4;
    const int64_t q = i >> 8;
    {
      const int jc = (int)(q % NJ), ct = (int)((q / NJ) % NCT), blk = (int)(q / ((int64_t)NJ * NCT));
      const int col = 16 * ct + r, e = 16 * jc + 4 * g + c;
      fragF[i] = col < T ? l1_w[(int64_t)col * T * E + (int64_t)blk * E + e] : 0.0f;
    }
    {
      const int kq = (int)(q % NCT), jn = (int)((q / NCT) % NJ), blk = (int)(q / ((int64_t)NJ * NCT));
      const int t = 4 * (4 * kq + c) + g, f = 16 * jn + r;
      fragB[i] = t < T ? l1_w[(int64_t)t * T * E + (int64_t)blk * E + f] : 0.0f;
    }
  }
}

// idx[r][0] = codes[r], idx[r][1 + j] = seqs[r][j]; anything outside [0, num_index) is padding
__global__ void dfm_train_idx_kernel(const int32_t *codes, const int32_t *seqs, int64_t B, int L, int64_t num_index, int32_t *idx) {
  const int T = L + 1;
  const int64_t n = B * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / T;
    const int j = (int)(i % T);
    const int32_t id = j == 0 ? codes[r] : seqs[r * L + j - 1];
    idx[i] = (id >= 0 && id < num_index) ? id : -1;
  }
}

struct DfmTrainRows {
  const float *emb, *l1_b, *l2_w, *l2_b;
  const f32x4 *fragF, *fragB;
  const int32_t *idx;                  // [B][T]
  const float *labels;                 // [B]
  int64_t B;
  int T;
  float *dH, *dX;                      // [B][NC] (columns >= T: 0), [B][T][E]
  double *ploss;                       // [gridDim.x]
  float *pg;                           // [gridDim.x][1 + NC]: g_l2b, g_l2W
};

#define DFM_WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// ---- what dfm_train_rows_kernel and the user-grouped dfm_tg_rows_kernel (dfm_train_grouped.hip.inc) share: a tile's epilogue and the
// workgroup's partials.  acc: H of the tile in the C layout; fm: of row r in every lane (., r); dhl: the wave's 16 x (16 NCT + 1) floats of
// LDS.  Adds the tile to lsum / gsum / pw2, stores dH (and g, where the caller keeps it), returns pass 2's operands grow and dhb
struct DfmTrainEpi { const float *l1_b, *l2_w, *labels; float *dH, *g /* [B], or NULL */; int64_t B; int T; float fB, b2; };
template <int NCT>
__device__ __forceinline__ void dfm_train_epilogue(const DfmTrainEpi &q, const f32x4 (&acc)[NCT], float fm, int64_t row0, int r, int g, float *dhl, double &lsum,
                                                   float &gsum, float (&pw2)[NCT], float &grow, float (&dhb)[4 * NCT]) {
  constexpr int NC = NCT * 16, LDH = NC + 1;
  // ---- epilogue in the C layout: lane (g, r) holds rows 4 g .. 4 g + 3 of column 16 ct + r
  float zl[4] = {0.f, 0.f, 0.f, 0.f}, hv[NCT][4], aw[NCT][4], gr[4];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    const int col = 16 * ct + r;
    const float b1 = col < q.T ? q.l1_b[col] : 0.0f, w2 = col < q.T ? q.l2_w[col] : 0.0f;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const float zp = acc[ct][rr] + b1;
      hv[ct][rr] = fmaxf(zp, 0.0f);
      aw[ct][rr] = zp > 0.0f ? w2 : 0.0f;
      zl[rr] = fmaf(w2, hv[ct][rr], zl[rr]);
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) zl[rr] += __shfl_xor(zl[rr], o);
    const int64_t row = row0 + 4 * g + rr;
    const float z = __shfl(fm, 4 * g + rr) + (zl[rr] + q.b2);
    float loss = 0.0f, gz = 0.0f;
    if (row < q.B) {
      const float y = q.labels[row], e = expf(-fabsf(z));
      loss = (fmaxf(z, 0.0f) - z * y) + log1pf(e);
      gz = ((z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e)) - y) / q.fB;
      if (q.g && r == 0) q.g[row] = gz;
    }
    gr[rr] = gz;
    if (r == 0) { lsum += (double)loss; gsum += gz; }
  }
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    const int col = 16 * ct + r;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const float dh = gr[rr] * aw[ct][rr];
      dhl[(4 * g + rr) * LDH + col] = dh;
      if (row0 + 4 * g + rr < q.B) q.dH[(row0 + 4 * g + rr) * NC + col] = dh;
      pw2[ct] = fmaf(gr[rr], hv[ct][rr], pw2[ct]);
    }
  }
  DFM_WAVE_LDS_SYNC();
  // ---- pass 2: dX_i^T = W1_i^T dH^T; lane (g, r) supplies dH[row r][unit 4 ks + g] and receives row r, features 16 jn + 4 g ..
  grow = 0.0f;
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
    const float t = __shfl(gr[rr], (r >> 2) * 16);
    if ((r & 3) == rr) grow = t;
  }
#pragma unroll
  for (int ks = 0; ks < 4 * NCT; ks++) dhb[ks] = dhl[r * LDH + 4 * ks + g];
}
template <int NCT>
__device__ __forceinline__ void dfm_train_partials(double lsum, float gsum, float (&pw2)[NCT], double *wloss, float (*wpg)[1 + 16 * NCT], double *ploss, float *pg) {
  constexpr int NC = NCT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  // ---- the workgroup's partials: lanes (g, 0) hold the loss and g of their rows, lanes (g, r) the g_l2W part of column 16 ct + r
  lsum += __shfl_xor(lsum, 16); lsum += __shfl_xor(lsum, 32);
  gsum += __shfl_xor(gsum, 16); gsum += __shfl_xor(gsum, 32);
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    pw2[ct] += __shfl_xor(pw2[ct], 16); pw2[ct] += __shfl_xor(pw2[ct], 32);
    if (g == 0) wpg[wave][1 + 16 * ct + r] = pw2[ct];
  }
  if (lane == 0) { wloss[wave] = lsum; wpg[wave][0] = gsum; }
  __syncthreads();
  if (threadIdx.x < 1 + NC) pg[(int64_t)blockIdx.x * (1 + NC) + threadIdx.x] = ((wpg[0][threadIdx.x] + wpg[1][threadIdx.x]) + wpg[2][threadIdx.x]) + wpg[3][threadIdx.x];
  if (threadIdx.x == 0) ploss[blockIdx.x] = ((wloss[0] + wloss[1]) + wloss[2]) + wloss[3];
}

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_train_rows_kernel(DfmTrainRows p) {
  constexpr int NJ = E / 16, NC = NCT * 16, LDH = NC + 1;
  __shared__ float dhl[4][16 * LDH];
  __shared__ double wloss[4];
  __shared__ float wpg[4][1 + NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int T = p.T;
  const int64_t tiles = (p.B + 15) / 16;
  const DfmTrainEpi q{p.l1_b, p.l2_w, p.labels, p.dH, nullptr, p.B, p.T, (float)p.B, p.l2_b[0]};
  double lsum = 0.0;
  float gsum = 0.0f, pw2[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) pw2[ct] = 0.0f;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 16, myrow = row0 + r;
    const bool in = myrow < p.B;
    const int32_t *ids = p.idx + myrow * T;
    // ---- pass 1: H = X W1^T, buf = sum_i x_i, sq = sum_i |x_i|^2 (this lane's features of row r)
    f32x4 buf[NJ], acc[NCT];
    float sq = 0.0f;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) buf[jc] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < T; i++) {
      const int32_t id = in ? ids[i] : -1;
      f32x4 x[NJ];
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        x[jc] = id >= 0 ? *(const f32x4 *)(p.emb + (int64_t)id * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
        buf[jc] += x[jc];
#pragma unroll
        for (int c = 0; c < 4; c++) sq = fmaf(x[jc][c], x[jc][c], sq);
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) {
          const f32x4 b = p.fragF[(((int64_t)i * NCT + ct) * NJ + jc) * 64 + lane];
#pragma unroll
          for (int c = 0; c < 4; c++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[jc][c], b[c], acc[ct], 0, 0, 0);
        }
    }
    float ss = 0.0f;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++)
#pragma unroll
      for (int c = 0; c < 4; c++) ss = fmaf(buf[jc][c], buf[jc][c], ss);
    ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);
    sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
    const float fm = 0.5f * (ss - sq);                 // of row r, in every lane (., r)
    // ---- epilogue in the C layout, then pass 2: dX_i^T = W1_i^T dH^T; lane (g, r) supplies dH[row r][unit 4 ks + g] and receives row r,
    // features 16 jn + 4 g ..
    float grow, dhb[4 * NCT];
    dfm_train_epilogue<NCT>(q, acc, fm, row0, r, g, dhl[wave], lsum, gsum, pw2, grow, dhb);
    for (int i = 0; i < T; i++) {
      const int32_t id = in ? ids[i] : -1;
      float *dst = p.dX + (myrow * T + i) * E + 4 * g;
#pragma unroll
      for (int jn = 0; jn < NJ; jn++) {
        const f32x4 x = id >= 0 ? *(const f32x4 *)(p.emb + (int64_t)id * E + 16 * jn + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kq = 0; kq < NCT; kq++) {
          const f32x4 a = p.fragB[(((int64_t)i * NJ + jn) * NCT + kq) * 64 + lane];
#pragma unroll
          for (int c = 0; c < 4; c++) c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], dhb[4 * kq + c], c4, 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) c4[c] = fmaf(grow, buf[jn][c] - x[c], c4[c]);
        if (in) *(f32x4 *)(dst + 16 * jn) = c4;
      }
    }
    DFM_WAVE_LDS_SYNC();               // the next tile overwrites dhl
  }
  dfm_train_partials<NCT>(lsum, gsum, pw2, wloss, wpg, p.ploss, p.pg);
}

// workgroup partials -> loss (mean, double), g_l2b, g_l2W, workgroup 0 first; one block of 64 threads (1 + NC <= 49)
__global__ void dfm_train_sum_kernel(const double *ploss, const float *pg, int nb, int NC, int T, int64_t B, double *loss, float *g_l2w, float *g_l2b) {
  const int c = threadIdx.x;
  if (c < 1 + NC) {
    float s = 0.0f;
    for (int b = 0; b < nb; b++) s += pg[(int64_t)b * (1 + NC) + c];
    if (c == 0) g_l2b[0] = s;
    else if (c - 1 < T) g_l2w[c - 1] = s;
  }
  if (c == 0) {
    double s = 0.0;
    for (int b = 0; b < nb; b++) s += ploss[b];
    loss[0] = s / (double)B;
  }
}

// g_emb from the sorted (destination, slot) pairs, in two levels.  The sampler repeats one history over all the rows of a target and
// histories are Zipf-distributed: a batch of 16 384 rows holds destinations with thousands of slots, and one wave adding them one after
// the other (drt_seg_rows_kernel) is the whole step's time.  Here the sorted positions are cut into CHUNKS at every multiple of
// DFM_SEG_CHUNK and at every change of destination.  Level 1: one wave per chunk adds the chunk's slots in sorted (= batch) order into
// the chunk's first slot of dX, in place (a chunk is read and written by its own wave only).  Level 2: one wave per destination adds
// its chunk heads in order.  The cuts are a function of the sorted order alone: a fixed order, the same bytes every run.
#define DFM_SEG_CHUNK 64
__global__ __launch_bounds__(256) void dfm_seg_chunks_kernel(const unsigned long long *keys, const int32_t *vals, int64_t m, int64_t NR, float *dX, int E) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < m; i += (int64_t)gridDim.x * 4) {
    const unsigned long long key = keys[i];
    if (key >= (unsigned long long)NR || ((i % DFM_SEG_CHUNK) != 0 && keys[i - 1] == key)) continue;       // padding, or not a chunk's first position
    const int64_t limit = std::min<int64_t>((i / DFM_SEG_CHUNK + 1) * DFM_SEG_CHUNK, m);
    const int n = (int)(limit - i);                                                                       // 1 .. 64 positions up to the next cut
    const bool differs = lane >= n - 1 || keys[i + 1 + lane] != key;
    const int len = __builtin_ctzll(__ballot(differs)) + 1;
    if (len == 1) continue;
    float *dst = dX + (int64_t)vals[i] * E;
    for (int e = lane; e < E; e += 64) {
      float acc = 0.0f;
      int q = 0;
      for (; q + 4 <= len; q += 4) {                        // four loads in flight, added in order
        const float x0 = dX[(int64_t)vals[i + q] * E + e], x1 = dX[(int64_t)vals[i + q + 1] * E + e], x2 = dX[(int64_t)vals[i + q + 2] * E + e], x3 = dX[(int64_t)vals[i + q + 3] * E + e];
        acc += x0; acc += x1; acc += x2; acc += x3;
      }
      for (; q < len; q++) acc += dX[(int64_t)vals[i + q] * E + e];
      dst[e] = acc;
    }
  }
}
__global__ __launch_bounds__(256) void dfm_seg_heads_kernel(const unsigned long long *keys, const int32_t *vals, int64_t m, int64_t NR, const float *dX, int E, float *grad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < m; i += (int64_t)gridDim.x * 4) {
    const unsigned long long key = keys[i];
    if (key >= (unsigned long long)NR || (i > 0 && keys[i - 1] == key)) continue;
    const int64_t qe = drt_segment_end(keys, i, m, key, lane);
    const int64_t next = (i / DFM_SEG_CHUNK + 1) * DFM_SEG_CHUNK;      // the destination's second chunk, if it reaches that far
    float *dst = grad + (int64_t)key * E;
    for (int e = lane; e < E; e += 64) {
      float acc = dX[(int64_t)vals[i] * E + e];
      for (int64_t q = next; q < qe; q += DFM_SEG_CHUNK) acc += dX[(int64_t)vals[q] * E + e];
      dst[e] = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// (launch kinds under DM_DFM_TIME_LAUNCHES=1: EV_DFT_* in host_request.hip.inc)
static int dfm_train_check(dm_ctx *h, const char *who, bool need_init) {
  const int rc = dfm_enter(h, who, nullptr, 0);
  if (rc != DM_OK) return rc;
  if (need_init && !h->dfm_tr) return fail(h, DM_ERR_STATE, std::string(who) + ": call dm_deepfm_train_init first");
  return DM_OK;
}

// every copy computed from the compact vector: the serving fragments, l2.b on the host and, while training, both orders of l1.W
static int dfm_rederive(dm_ctx *h) {
  const DfmBlocks b = dfm_blocks(h);
  const int E = h->embed, T = h->dfm_L + 1;
  int rc = LAUNCH(h, dfm_derive_kernel, dim3(32), dim3(256), 0, b.l1_w, b.l2_w, E, T, dfm_col_tiles(h->dfm_L), h->d_dfm_frag, h->d_dfm_w2p);
  if (rc == DM_OK) rc = LAUNCH(h, dfm_jtm_derive_kernel, dim3(256), dim3(256), 0, b.l1_w, E, h->dfm_L, dfm_col_tiles(h->dfm_L), h->d_dfm_fragS);
  if (rc == DM_OK && h->dfm_tr)
    rc = LAUNCH(h, dfm_train_derive_kernel, dim3(256), dim3(256), 0, b.l1_w, E, T, dfm_train_col_tiles(h->dfm_L), h->dfm_tr->fragF, h->dfm_tr->fragB);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(&h->b2, b.l2_b, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_deepfm_train_init(dm_handle_t h, const dm_adam_opts *o) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_init");
  int rc = dfm_train_check(h, "dm_deepfm_train_init", false);
  if (rc != DM_OK) return rc;
  if (!o || !(o->lr > 0)) return fail(h, DM_ERR_INVALID, "dm_deepfm_train_init: bad optimizer options");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfm_train_release(h);
  dm_dfm_train *t = new dm_dfm_train();
  h->dfm_tr = t;
  const int E = h->embed, L = h->dfm_L;
  const size_t frag_bytes = (size_t)(L + 1) * dfm_train_col_tiles(L) * E * 64;
  rc = t->vec.init(h, h->num_index, E, deepfm_len_for(h->num_index, E, L), 4, *o);
  if (rc == DM_OK) rc = dm_alloc(h, (void **)&t->fragF, frag_bytes);
  if (rc == DM_OK) rc = dm_alloc(h, (void **)&t->fragB, frag_bytes);
  if (rc == DM_OK) rc = dfm_rederive(h);
  if (rc != DM_OK) dfm_train_release(h);
  return rc;
}

int dm_deepfm_train_free(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_free");
  if (!h->dfm_tr) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfm_train_release(h);
  return DM_OK;
}

// ---- what the row step and the user-grouped step (dfm_train_grouped.hip.inc) share on the host
// zeroGradParameters for the table: the rows the last batch reached, of either step (the dense blocks are overwritten by every step).
// After a gradient exchange `prev` is the concatenation of every rank's rows, not sorted and with repeats: the kernel clears at every
// change of key, so a row may be cleared more than once, which changes nothing
static int dfm_train_clear_prev(dm_ctx *h, dm_dfm_train *t) {
  t->exchanged = false;
  if (t->vec.prev_m <= 0) return DM_OK;
  const int rc = LAUNCH(h, (drt_seg_rows_kernel<float, true>), dim3(drt_blocks(h, t->vec.prev_m, 4)), dim3(256), 0, (const unsigned long long *)t->vec.prev.p, nullptr,
                        t->vec.prev_m, h->num_index, nullptr, h->embed, (float *)t->vec.grad);
  if (rc == DM_OK) t->vec.forget();
  return rc;
}
// g_emb: the m slots idx[i] -> dX[i] sorted by destination row, chunk sums, one wave per destination; the rows are remembered and marked active
static int dfm_train_emb_grad(dm_ctx *h, dm_dfm_train *t, const int32_t *idx, int64_t m, float *dX, const DrtSortBufs &sb, bool detail) {
  const int E = h->embed;
  const int64_t NI = h->num_index;
  return timed(h, EV_DFT_EMB, detail, [&] {
    const unsigned long long *ks;
    const int32_t *vs;
    int rc;
    if ((rc = drt_sort_slots(h, idx, m, NI, sb, ks, vs)) != DM_OK) return rc;
    if ((rc = LAUNCH(h, dfm_seg_chunks_kernel, dim3(drt_blocks(h, m, 4)), dim3(256), 0, ks, vs, m, NI, dX, E)) != DM_OK) return rc;
    if ((rc = LAUNCH(h, dfm_seg_heads_kernel, dim3(drt_blocks(h, m, 4)), dim3(256), 0, ks, vs, m, NI, dX, E, (float *)t->vec.grad)) != DM_OK) return rc;
    if ((rc = t->vec.remember(h, ks, m)) != DM_OK) return rc;
    return t->vec.mark_active(h, drt_blocks(h, m, 256), idx, m);
  });
}

template <int E, int NCT>
static int dfm_launch_train_rows(dm_ctx *h, const DfmTrainRows &p, int nb, bool on) {
  return timed(h, EV_DFT_ROWS, on, [&] { return LAUNCH(h, (dfm_train_rows_kernel<E, NCT>), dim3((unsigned)nb), dim3(256), 0, p); });
}

static int dfm_train_fb_dev(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const float *d_labels, int64_t B, double *out_loss) {
  dm_dfm_train *t = h->dfm_tr;
  const int E = h->embed, L = h->dfm_L, T = L + 1, NCT = dfm_train_col_tiles(L), NC = 16 * NCT;
  const int64_t NI = h->num_index, m = B * T;
  // B T slots are sorted with 32-bit values; the slabs of the l1.W product are a grid's z
  if (m >= ((int64_t)1 << 31) || B > (int64_t)DRT_MAX_ROWS)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_deepfm_train_forward_backward: batch too large (at most 4 194 240 rows, and B (L + 1) below 2^31): split it and accumulate on the host");
  const bool detail = dfm_time_launches();
  const int64_t slabs = (B + DRT_SLAB - 1) / DRT_SLAB;
  int nb = (int)std::min<int64_t>(((B + 15) / 16 + 3) / 4, 1024);            // workgroups of the rows kernel: a function of B alone
  if (const long long g_ = env_int("DM_DFM_TRAIN_GRID")) nb = (int)std::min<long long>(g_, 65535);      // (tests: a second, partial round of the grid-stride loop)
  int rc;
  DevArena ar(t->ws, 8);
  const size_t o_idx = ar.add((size_t)m * 4), o_dh = ar.add((size_t)B * NC * 4), o_dx = ar.add((size_t)m * E * 4);
  const size_t o_k0 = ar.add((size_t)m * 8), o_k1 = ar.add((size_t)m * 8), o_v0 = ar.add((size_t)m * 4), o_v1 = ar.add((size_t)m * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_part = ar.add((size_t)slabs * T * ((size_t)T * E + 1) * 4);
  const size_t o_pl = ar.add((size_t)nb * 8), o_pg = ar.add((size_t)nb * (1 + NC) * 4), o_loss = ar.add(8);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  int32_t *idx = ar.ptr<int32_t>(o_idx);
  float *dH = ar.ptr<float>(o_dh), *dX = ar.ptr<float>(o_dx), *part = ar.ptr<float>(o_part);
  float *grad = (float *)t->vec.grad;
  float *g_l1w = grad + NI * E, *g_l1b = g_l1w + (int64_t)T * T * E, *g_l2w = g_l1b + T, *g_l2b = g_l2w + T;
  // ---- zeroGradParameters: the rows the last batch reached (the dense blocks are overwritten below)
  if ((rc = dfm_train_clear_prev(h, t)) != DM_OK) return rc;
  if ((rc = LAUNCH(h, dfm_train_idx_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, d_codes, d_seqs, B, L, NI, idx)) != DM_OK) return rc;
  // ---- forward, loss, dH, dX
  {
    const DfmBlocks b = dfm_blocks(h);
    DfmTrainRows p;
    p.emb = h->d_emb32; p.l1_b = b.l1_b; p.l2_w = b.l2_w; p.l2_b = b.l2_b; p.fragF = (const f32x4 *)t->fragF; p.fragB = (const f32x4 *)t->fragB;
    p.idx = idx; p.labels = d_labels; p.B = B; p.T = T; p.dH = dH; p.dX = dX; p.ploss = ar.ptr<double>(o_pl); p.pg = ar.ptr<float>(o_pg);
    rc = dispatch_E_NCT(h, E, NCT, "unsupported embed size", [&](auto e, auto n) { return dfm_launch_train_rows<decltype(e)::value, decltype(n)::value>(h, p, nb, detail); });
    if (rc != DM_OK) return rc;
    if ((rc = LAUNCH(h, dfm_train_sum_kernel, dim3(1), dim3(64), 0, p.ploss, p.pg, nb, NC, T, B, ar.ptr<double>(o_loss), g_l2w, g_l2b)) != DM_OK) return rc;
  }
  // ---- g_l1W, g_l1b: dH^T [T x B] . [X | 1] [B x (T E + 1)] in slabs of the batch, added in slab order
  {
    const int cols = T * E;
    DrtGemmParams<float> g{};
    g.A = dH; g.a_rs = 1; g.a_cs = NC;
    g.B = h->d_emb32; g.gidx = idx; g.Lg = T; g.E = E; g.gcols = cols;
    g.C = part; g.ldc = cols + 1; g.c_slab = (int64_t)T * (cols + 1); g.M = T; g.N = cols + 1; g.Kd = B; g.slab = DRT_SLAB;
    if ((rc = drt_launch_gemm<float>(h, g, EV_DFT_DW, detail)) != DM_OK) return rc;
    rc = timed(h, EV_DFT_DW, detail, [&] {
      return LAUNCH(h, drt_slab_sum_kernel<float>, dim3(drt_blocks(h, (int64_t)T * (cols + 1), 256)), dim3(256), 0, part, (int)slabs, T, cols, g_l1w, g_l1b, cols);
    });
    if (rc != DM_OK) return rc;
  }
  // ---- g_emb: sort the B T slots by destination row, chunk sums, one wave per destination
  {
    const DrtSortBufs sb{ar.ptr<unsigned long long>(o_k0), ar.ptr<unsigned long long>(o_k1), ar.ptr<int32_t>(o_v0), ar.ptr<int32_t>(o_v1), ar.ptr<uint32_t>(o_tmp)};
    if ((rc = dfm_train_emb_grad(h, t, idx, m, dX, sb, detail)) != DM_OK) return rc;
  }
  if (out_loss) HIPCHK(h, hipMemcpyAsync(out_loss, ar.ptr<double>(o_loss), 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

static int dfm_train_fb_args(dm_ctx *h, const void *codes, const void *seqs, const void *labels, int64_t B, int L) {
  if (B <= 0 || !codes || !seqs || !labels) return fail(h, DM_ERR_INVALID, "dm_deepfm_train_forward_backward: B must be positive and the arrays non-null");
  return dfm_check_L(h, "dm_deepfm_train_forward_backward", L);
}

int dm_deepfm_train_forward_backward_dev(dm_handle_t h, const int32_t *d_codes, const int32_t *d_seqs, const float *d_labels, int64_t B, int L, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_forward_backward");
  int rc = dfm_train_check(h, "dm_deepfm_train_forward_backward", true);
  if (rc != DM_OK) return rc;
  if ((rc = dfm_train_fb_args(h, d_codes, d_seqs, d_labels, B, L)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return dfm_train_fb_dev(h, d_codes, d_seqs, d_labels, B, out_loss);
}

int dm_deepfm_train_forward_backward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, const float *labels, int64_t B, int L, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_forward_backward");
  int rc = dfm_train_check(h, "dm_deepfm_train_forward_backward", true);
  if (rc != DM_OK) return rc;
  if ((rc = dfm_train_fb_args(h, codes, seqs, labels, B, L)) != DM_OK) return rc;
  if (B * (int64_t)(L + 1) >= ((int64_t)1 << 31) || B > (int64_t)DRT_MAX_ROWS)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_deepfm_train_forward_backward: batch too large (at most 4 194 240 rows, and B (L + 1) below 2^31): split it and accumulate on the host");
  if ((rc = check_lookup_ids(h, codes, B, 1, "row")) != DM_OK || (rc = check_lookup_ids(h, seqs, B * L, L, "row")) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_dfm_train *t = h->dfm_tr;
  const size_t b_codes = DevArena::up((size_t)B * 4), b_seqs = DevArena::up((size_t)B * L * 4), b_lab = DevArena::up((size_t)B * 4);
  if ((rc = t->io.reserve(h, b_codes + b_seqs + b_lab)) != DM_OK) return rc;
  int32_t *d_codes = (int32_t *)t->io.p, *d_seqs = (int32_t *)((char *)t->io.p + b_codes);
  float *d_lab = (float *)((char *)t->io.p + b_codes + b_seqs);
  HIPCHK(h, hipMemcpyAsync(d_codes, codes, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_seqs, seqs, (size_t)B * L * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_lab, labels, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  return dfm_train_fb_dev(h, d_codes, d_seqs, d_lab, B, out_loss);
}

// Adam.optimize over the padded device vector with dm_dr_adam_step's rules; then every copy computed from the weights is rebuilt and
// the clones are told: a model trained here serves exactly what a fresh handle loaded from its downloaded weights serves.
int dm_deepfm_adam_step(dm_handle_t h, float grad_scale) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_adam_step");
  int rc = dfm_train_check(h, "dm_deepfm_adam_step", true);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_dfm_train *t = h->dfm_tr;
  unsigned long long act = 0;
  HIPCHK(h, hipMemcpyAsync(&act, t->vec.active_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const AdamPlan plan = t->vec.plan_step(act);
  model_changed(h);                 // before the first launch: a step that fails half-way has still moved weights
  rc = timed(h, EV_DFT_ADAM, dfm_time_launches(), [&] { return adam_step(h, t->vec, plan, h->d_compact, false, false, grad_scale, false, 1024); });
  if (rc != DM_OK) return rc;
  t->vec.forget();                  // the step zeroed every gradient it visited, and it visited every row a batch has reached
  t->exchanged = false;
  if ((rc = dfm_rederive(h)) != DM_OK) return rc;
  model_changed(h);
  return DM_OK;
}

int dm_deepfm_train_param_count(dm_handle_t h, int64_t *n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_param_count");
  int rc = dfm_train_check(h, "dm_deepfm_train_param_count", false);
  if (rc != DM_OK) return rc;
  if (!n) return fail(h, DM_ERR_INVALID, "dm_deepfm_train_param_count: null argument");
  *n = deepfm_len_for(h->num_index, h->embed_log, h->dfm_L);
  return DM_OK;
}

// the device vector `what` (padded layout) on the host
static int dfm_train_fetch(dm_ctx *h, int what, std::vector<float> &dev) {
  dev.resize((size_t)deepfm_len_for(h->num_index, h->embed, h->dfm_L));
  const void *src = what == 0 ? h->d_compact : h->dfm_tr->vec.buffer(what);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(dev.data(), src, dev.size() * 4, hipMemcpyDeviceToHost));
  return DM_OK;
}

int dm_deepfm_train_download(dm_handle_t h, int what, float *out, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_download");
  int rc = dfm_train_check(h, "dm_deepfm_train_download", what != 0);      // the weights of a loaded model can be read without training state
  if (rc != DM_OK) return rc;
  if (!out || what < 0 || what > 3 || n != deepfm_len_for(h->num_index, h->embed_log, h->dfm_L))
    return fail(h, DM_ERR_INVALID, "dm_deepfm_train_download: what must be 0..3 and n the parameter count");
  std::vector<float> dev;
  if ((rc = dfm_train_fetch(h, what, dev)) != DM_OK) return rc;
  if (h->embed == h->embed_log) memcpy(out, dev.data(), (size_t)n * 4);
  else dfm_repad(dev.data(), h->embed, h->embed_log, h->num_index, h->dfm_L, out);
  return DM_OK;
}

// debug view, not in the public header: the same vectors as the device holds them (every E-wide block padded to `embed`); n = that
// length, or out == NULL to ask for it (tests: the padded columns stay exact zeros)
extern "C" int dm_debug_deepfm_train_padded(dm_handle_t h, int what, float *out, int64_t *n) {
  if (!h || !n) return DM_ERR_INVALID;
  int rc = dfm_train_check(h, "dm_debug_deepfm_train_padded", what != 0);
  if (rc != DM_OK) return rc;
  const int64_t len = deepfm_len_for(h->num_index, h->embed, h->dfm_L);
  if (!out) { *n = len; return DM_OK; }
  if (what < 0 || what > 3 || *n != len) return fail(h, DM_ERR_INVALID, "dm_debug_deepfm_train_padded: what must be 0..3 and *n the padded length");
  std::vector<float> dev;
  if ((rc = dfm_train_fetch(h, what, dev)) != DM_OK) return rc;
  memcpy(out, dev.data(), (size_t)len * 4);
  return DM_OK;
}

// ---- the sampler's twins: the rows of dm_tdm_make_train_batch / dm_tdm_sample_train_batch_dev without a mask (the graph has none)
static int dfm_sample_check(dm_ctx *h, const char *who, int64_t T, int L, const int32_t *neg_counts, int n_counts, const dm_sample_opts *o, int64_t *per) {
  const int rc = dfm_enter(h, who, &L, o ? o->use_mask : 0);
  if (rc != DM_OK) return rc;
  return sample_check(h, DM_KIND_DEEPFM, T, L, neg_counts, n_counts, o, per);
}

int dm_deepfm_sample_train_batch_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                     const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                     int32_t *d_seqs, float *d_labels, int64_t cap, int64_t *n_rows) {
  if (!h || !n_rows) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_sample_train_batch_dev");
  int64_t per = 0;
  int rc = dfm_sample_check(h, "dm_deepfm_sample_train_batch_dev", T, L, neg_counts, n_counts, opts, &per);
  if (rc != DM_OK) return rc;
  *n_rows = T * per;
  if (!d_codes) return DM_OK;                        // size query: an upper bound (targets outside the tree yield no rows)
  if (!d_seq_item_ids || !d_target_item_ids || !d_seqs || !d_labels || cap < T * per)
    return fail(h, DM_ERR_INVALID, "dm_deepfm_sample_train_batch_dev: output buffers too small");
  HIPCHK(h, hipSetDevice(h->device));
  return sample_dev(h, d_seq_item_ids, d_target_item_ids, T, L, neg_counts, opts, d_codes, d_seqs, nullptr, d_labels, cap, n_rows);
}

int dm_deepfm_sample_train_batch_csr_dev(dm_handle_t h, const int32_t *d_seq_item_ids, const int32_t *d_target_item_ids, int64_t T, int L,
                                         const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *d_codes,
                                         int32_t *d_seq_codes, int64_t *d_row_off, float *d_labels, int64_t cap, int64_t *n_rows) {
  if (!h || !n_rows) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_sample_train_batch_csr_dev");
  int64_t per = 0;
  int rc = dfm_sample_check(h, "dm_deepfm_sample_train_batch_csr_dev", T, L, neg_counts, n_counts, opts, &per);
  if (rc != DM_OK) return rc;
  *n_rows = T * per;
  if (!d_codes) return DM_OK;                        // size query: an upper bound, the row twin's
  if (!d_seq_item_ids || !d_target_item_ids || !d_seq_codes || !d_row_off || !d_labels || cap < T * per)
    return fail(h, DM_ERR_INVALID, "dm_deepfm_sample_train_batch_csr_dev: output buffers too small");
  HIPCHK(h, hipSetDevice(h->device));
  return sample_dev(h, d_seq_item_ids, d_target_item_ids, T, L, neg_counts, opts, d_codes, nullptr, nullptr, d_labels, cap, n_rows, d_seq_codes, d_row_off);
}

int dm_deepfm_make_train_batch(dm_handle_t h, const int32_t *seq_item_ids, const int32_t *target_item_ids, int64_t T, int L,
                               const int32_t *neg_counts, int n_counts, const dm_sample_opts *opts, int32_t *out_codes,
                               int32_t *out_seqs, float *out_labels, int64_t cap, int64_t *n_rows) {
  if (!h || !n_rows) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_make_train_batch");
  int64_t per = 0;
  int rc = dfm_sample_check(h, "dm_deepfm_make_train_batch", T, L, neg_counts, n_counts, opts, &per);
  if (rc != DM_OK) return rc;
  *n_rows = T * per;
  if (!out_codes) return DM_OK;                       // size query
  if (!seq_item_ids || !target_item_ids || !out_seqs || !out_labels || cap < T * per)
    return fail(h, DM_ERR_INVALID, "dm_deepfm_make_train_batch: output buffers too small");
  if (T == 0) { *n_rows = 0; return DM_OK; }
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t R = T * per;
  int32_t *d_seq = nullptr, *d_tgt = nullptr, *d_codes = nullptr, *d_seqs = nullptr;
  float *d_lab = nullptr;
  DevTemps t(h);
  if ((rc = t.alloc(d_seq, (size_t)T * L * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_tgt, (size_t)T * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_codes, (size_t)R * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_seqs, (size_t)R * L * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_lab, (size_t)R * 4)) != DM_OK) return rc;
  hipError_t e = hipMemcpyAsync(d_seq, seq_item_ids, (size_t)T * L * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tgt, target_item_ids, (size_t)T * 4, hipMemcpyHostToDevice, h->stream);
  if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_deepfm_make_train_batch: upload failed");
  int64_t n = 0;
  if ((rc = sample_dev(h, d_seq, d_tgt, T, L, neg_counts, opts, d_codes, d_seqs, nullptr, d_lab, R, &n)) != DM_OK) return rc;
  if (n > 0) {
    e = hipMemcpy(out_codes, d_codes, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_seqs, d_seqs, (size_t)n * L * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_labels, d_lab, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_deepfm_make_train_batch: download failed");
  }
  *n_rows = n;
  return rc;
}
