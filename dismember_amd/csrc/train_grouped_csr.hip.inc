// DIN training step, ragged user-grouped form for f32 models (dm_train_forward_backward_csr_dev; DESIGN.md §21): the step of
// train_kernel.hip.inc on a batch given as U histories seq[u][0..L) with one mask word each and B candidate rows, rows
// row_off[u] .. row_off[u + 1] belonging to user u (a user may have none).  Everything that depends on a history alone is computed once
// per user (k_j = emb[seq[u][j]], a zero row for -1 and for j >= L; W1a / W1b = the two halves of l1.W):
//   per user   T_j = att.W k_j     G_j = W1b T_j
//   per row    s_j = q . k_j / sqrt(embed_size) (-FLT_MAX where masked)    p = softmax(s)    z = W1a q + sum_j p_j G_j + b1    x = w2 . relu(z) + b2
//              gl = (sigmoid(x) - y) / B    dz = [z > 0] gl w2    dp_j = G_j . dz    ds_j = p_j (dp_j - sum_i p_i dp_i) / sqrt(embed_size) (0 where masked)
//              dq = W1a^T dz + sum_j ds_j k_j
//   per user   dG_j = sum_r p_j dz    dT_j = W1b^T dG_j    dk_j = sum_r ds_j q + att.W^T dT_j          (r: the user's rows, ascending)
//   weights    g_W1a = sum_rows dz (x) q    g_W1b = sum_{u,j} dG_j (x) T_j    g_att.W = sum_{u,j} dT_j (x) k_j    g_l1.b = sum dz
//              g_l2.W = sum gl relu(z)    g_l2.b = sum gl
//   table      dq at the candidate's row, dk_j at the history's rows
// Three E x E products per row tile (W1a q, W1a^T dz, and the g_W1a contraction) where the row step has nine, and the history rows are read
// once per user.
//
// Kernels (the fragment orders are dm_refresh_fragments_kernel's A orders, read through L2; lane (r, g) = (lane & 15, lane >> 4)):
//   dfm_tg_check_off_kernel    the offsets, read back before anything dereferences through them and before the workspace is reserved
//                              (dfm_train_grouped.hip.inc; the flag is the handle's d_loss word)
//   din_csr_idx_kernel         [codes ; seq] as one index array of B + U L slots, an id outside [0, num_index) becomes -1, so do the L
//                              slots of a user without rows
//   din_csr_tilecnt_kernel + dm_sample_scan_kernel (x2) + din_csr_slots_kernel   tiles of 16 rows per user, never straddling users, and
//                              their exclusive scan; the users that have rows numbered in order (slots), so that the per-user arrays
//                              hold them densely: the slabs of the two per-user products then do not depend on where rowless users sit,
//                              and a batch gives the same bytes with them removed
//   din_csr_setup_kernel       one wave per slot: K, T, G [U 16][E] (rows j >= L are zero); the slots past the last populated user are
//                              zeroed in all five per-user arrays (the products run over U 16 rows: no count is read back)
//   din_csr_rows_kernel        one wave per tile: the five attention products are 16x16x4 MFMAs against the user's K and G in both
//                              orientations (K as A operand with the position on the lane: Q K^T and G dz; with the position as k: sum_j p_j G_j
//                              and sum_j ds_j k_j, whose B operand is the lane's own four p / ds); writes dz, p, ds, dq and per row gl relu(z), gl, loss
//   din_csr_user_bwd_kernel    one wave per populated user: dG and sum_r ds_j q as MFMAs over four rows a step in ascending order, the transposes through
//                              the wave's LDS, then dT, dk
//   drt_gemm_kernel<float> (x3) + din_csr_slab_add_kernel   g_W1a and g_l1.b (ones column) over the B rows gathered through [codes]; g_W1b and
//                              g_att.W over the U 16 per-user rows; slabs added in slab order
//   din_csr_colsum_kernel + din_csr_tail_kernel   g_l2.W, g_l2.b and the loss: columns of 512-row slabs in row order (fp64), slabs in slab order
//   drt_sort_slots + dfm_seg_chunks_kernel + din_csr_seg_heads_add_kernel   the table gradient from the B + U L slots
// No floating-point atomics.  Every destination has one writer per call and every sum an order that depends on the batch alone: no per-workgroup
// partials exist, so the grid (DM_DIN_TRAIN_GRID) cannot enter the bytes.  The step ADDS into the handle's gradient.

struct DinCsrParams {
  const float *emb;
  const f32x4 *attA, *w1aA, *w1bA, *attTA, *w1aTA, *w1bTA;
  const float *b1, *w2;
  float b2, inv_B, sm_scale;
  const int32_t *idx;                  // [B] candidates, then [U][L] histories
  const uint32_t *umask;               // [U] or null
  const int64_t *row_off, *tile_off;   // [U + 1]
  const int64_t *slot_off;             // [U + 1]: populated users before u; [U] = their number
  const int32_t *slot_user;            // [U]: the user of a slot
  const float *labels;                 // [B]
  int64_t U, B;
  int L;
  float *K, *T, *G;                    // [U 16][E], by slot
  float *DZ;                           // [B][E]
  float *P, *DS;                       // [B][16]
  float *AUX;                          // [B][E + 4]: gl relu(z), then gl, the row's loss term, 0, 0
  float *dX;                           // [B + U L][E]: dq, then dk
  float *dG, *dT;                      // [U 16][E], by slot
};

// row_off has passed dfm_tg_check_off_kernel
__global__ void din_csr_idx_kernel(const int32_t *codes, const int32_t *seq, const int64_t *row_off, int64_t B, int64_t U, int L, int64_t num_index, int32_t *idx) {
  const int64_t n = B + U * L;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t id;
    if (i < B) id = codes[i];
    else { const int64_t u = (i - B) / L; id = row_off[u + 1] > row_off[u] ? seq[i - B] : -1; }
    idx[i] = (id >= 0 && id < num_index) ? id : -1;
  }
}
__global__ void din_csr_tilecnt_kernel(const int64_t *row_off, int64_t U, int64_t *cnt, int64_t *has) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < U; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = row_off[u + 1] - row_off[u];
    cnt[u] = (n + 15) >> 4;
    has[u] = n > 0 ? 1 : 0;
  }
}
__global__ void din_csr_slots_kernel(const int64_t *slot_off, int64_t U, int32_t *slot_user) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < U; u += (int64_t)gridDim.x * blockDim.x)
    if (slot_off[u + 1] > slot_off[u]) slot_user[slot_off[u]] = (int32_t)u;
}

// out[mt] = sum_jc W[mt][jc] x[jc] (row-fragment layout in and out), the fragments read through L2 from an opaque offset (left
// loop-invariant, hipcc hoists every fragment address out of the caller's loop and spills them: train_kernel.hip.inc)
template <int E>
__device__ __forceinline__ void din_csr_prod(const f32x4 *frag, const f32x4 (&x)[E / 16], f32x4 (&out)[E / 16], const bool accumulate) {
  constexpr int NJ = E / 16, NT = E / 16;
#pragma unroll
  for (int mt = 0; mt < NT; mt++) {
    f32x4 acc = accumulate ? out[mt] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      const f32x4 wa = frag[(mt * NJ + jc) * 64];
#pragma unroll
      for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t], x[jc][t], acc, 0, 0, 0);
    }
    out[mt] = acc;
  }
}

template <int E>
__global__ __launch_bounds__(256) void din_csr_setup_kernel(DinCsrParams p) {
  constexpr int NJ = E / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int64_t n_pop = p.slot_off[p.U];
  for (int64_t slot = (int64_t)blockIdx.x * 4 + wave; slot < p.U; slot += (int64_t)gridDim.x * 4) {
    const int64_t o = (slot * 16 + r) * E + 4 * g;
    if (slot >= n_pop) {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        *(f32x4 *)(p.K + o + 16 * jc) = z4; *(f32x4 *)(p.T + o + 16 * jc) = z4; *(f32x4 *)(p.G + o + 16 * jc) = z4;
        *(f32x4 *)(p.dG + o + 16 * jc) = z4; *(f32x4 *)(p.dT + o + 16 * jc) = z4;
      }
      continue;
    }
    const int64_t u = p.slot_user[slot];
    int zo = 0;
    asm volatile("" : "+v"(zo));
    const int32_t id = r < p.L ? p.idx[p.B + u * p.L + r] : -1;
    f32x4 kv[NJ], tv[NJ], gv[NJ];
#pragma unroll
    for (int jc = 0; jc < NJ; jc++)
      kv[jc] = id >= 0 ? *(const f32x4 *)(p.emb + (int64_t)id * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
    din_csr_prod<E>(p.attA + lane + zo, kv, tv, false);
    din_csr_prod<E>(p.w1bA + lane + zo, tv, gv, false);
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      *(f32x4 *)(p.K + o + 16 * jc) = kv[jc];
      *(f32x4 *)(p.T + o + 16 * jc) = tv[jc];
      *(f32x4 *)(p.G + o + 16 * jc) = gv[jc];
    }
  }
}

template <int E>
__global__ __launch_bounds__(256) void din_csr_rows_kernel(DinCsrParams p) {
  typedef DmTr<float> TR;
  constexpr int NJ = E / 16, NT = E / 16, EA = E + 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int64_t n_tiles = p.tile_off[p.U];
  const f32x4 vzero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    int64_t lo = 0, hi = p.U;            // the user of the tile: tile_off[lo] <= tile < tile_off[hi] throughout (users without tiles are skipped)
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (p.tile_off[mid] <= tile) lo = mid; else hi = mid; }
    const int64_t u = lo;
    const int64_t rend = p.row_off[u + 1];
    const int64_t row = p.row_off[u] + (tile - p.tile_off[u]) * 16 + r;
    const bool live = row < rend;        // (the dead rows of a user's last tile are neither gathered nor stored)
    int zo = 0;
    asm volatile("" : "+v"(zo));
    const int32_t code = live ? p.idx[row] : -1;
    f32x4 qa[NJ];
#pragma unroll
    for (int jc = 0; jc < NJ; jc++)
      qa[jc] = code >= 0 ? *(const f32x4 *)(p.emb + (int64_t)code * E + 16 * jc + 4 * g) : vzero;
    const unsigned mask = p.umask ? p.umask[u] : 0u;
    const int64_t slot = p.slot_off[u];
    const float *Ku = p.K + slot * 16 * E + zo, *Gu = p.G + slot * 16 * E + zo;
    // ---- S = K Q^T: lane (r, g) gets s of positions 4 g .. 4 g + 3 of row r
    f32x4 sv = vzero;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      const f32x4 kf = *(const f32x4 *)(Ku + r * E + 16 * jc + 4 * g);
#pragma unroll
      for (int t = 0; t < 4; t++) sv = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t], qa[jc][t], sv, 0, 0, 0);
    }
    float m = -INFINITY;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const int pos = 4 * g + rr;
      float v = sv[rr] * p.sm_scale;
      if ((mask >> pos) & 1u) v = -FLT_MAX;
      if (pos >= p.L) v = -INFINITY;
      sv[rr] = v;
      m = fmaxf(m, v);
    }
    m = fmaxf(m, __shfl_xor(m, 16)); m = fmaxf(m, __shfl_xor(m, 32));      // (position 0 exists: m is finite)
    f32x4 pr;
    float lsum = 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) { pr[rr] = expf(sv[rr] - m); lsum += pr[rr]; }
    lsum = TR::xsum(lsum);
    const float inv_l = 1.0f / lsum;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) pr[rr] *= inv_l;
    // ---- z = W1a q + sum_j p_j G_j + b1, x = w2 . relu(z) + b2
    const f32x4 *fW1a = p.w1aA + lane + zo, *fW1aT = p.w1aTA + lane + zo;
    const float *fb1 = p.b1 + zo, *fw2 = p.w2 + zo;
    f32x4 zv[NT];
    float part = 0.f;
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      f32x4 acc = vzero;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 wa = fW1a[(mt * NJ + jc) * 64];
#pragma unroll
        for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t], qa[jc][t], acc, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Gu[(4 * g + t) * E + 16 * mt + r], pr[t], acc, 0, 0, 0);
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int f = 16 * mt + 4 * g + rr;
        acc[rr] += fb1[f];
        part = fmaf(acc[rr] > 0 ? acc[rr] : 0.f, fw2[f], part);
      }
      zv[mt] = acc;
    }
    const float x = TR::xsum(part) + p.b2;
    const float y = live ? p.labels[row] : 0.f;
    const float gl = live ? (1.0f / (1.0f + expf(-x)) - y) * p.inv_B : 0.f;
    // ---- dz (in place of z), gl relu(z), the row's gl and loss term
    float *aux = p.AUX + row * EA;
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      f32x4 hg;
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const float zz = zv[mt][rr];
        hg[rr] = zz > 0 ? gl * zz : 0.f;
        zv[mt][rr] = zz > 0 ? gl * fw2[16 * mt + 4 * g + rr] : 0.f;
      }
      if (live) {
        *(f32x4 *)(p.DZ + row * E + 16 * mt + 4 * g) = zv[mt];
        *(f32x4 *)(aux + 16 * mt + 4 * g) = hg;
      }
    }
    if (live && g == 0) {
      const float lt = ((x > 0 ? x : 0.f) + logf(1.0f + expf(-(x < 0 ? -x : x)))) - x * y;
      *(f32x4 *)(aux + E) = (f32x4){gl, lt, 0.f, 0.f};
    }
    // ---- dp = G dz, ds
    f32x4 dp = vzero;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      const f32x4 gf = *(const f32x4 *)(Gu + r * E + 16 * jc + 4 * g);
#pragma unroll
      for (int t = 0; t < 4; t++) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[t], zv[jc][t], dp, 0, 0, 0);
    }
    float dot = 0.f;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) dot = fmaf(pr[rr], dp[rr], dot);
    dot = TR::xsum(dot);
    f32x4 ds;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      ds[rr] = (dp[rr] - dot) * pr[rr] * p.sm_scale;
      if ((mask >> (4 * g + rr)) & 1u) ds[rr] = 0.f;
    }
    if (live) {
      *(f32x4 *)(p.P + row * 16 + 4 * g) = pr;
      *(f32x4 *)(p.DS + row * 16 + 4 * g) = ds;
    }
    // ---- dq = W1a^T dz + sum_j ds_j k_j
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      f32x4 acc = vzero;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 wa = fW1aT[(mt * NJ + jc) * 64];
#pragma unroll
        for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t], zv[jc][t], acc, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ku[(4 * g + t) * E + 16 * mt + r], ds[t], acc, 0, 0, 0);
      if (live) *(f32x4 *)(p.dX + row * E + 16 * mt + 4 * g) = acc;
    }
  }
}

template <int E>
__global__ __launch_bounds__(256) void din_csr_user_bwd_kernel(DinCsrParams p) {
  constexpr int NJ = E / 16, NT = E / 16, LD = E + 4;
  __shared__ __attribute__((aligned(16))) float xl[4][16 * LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  float *X = xl[wave];
  const f32x4 vzero = {0.f, 0.f, 0.f, 0.f};
  const int64_t n_pop = p.slot_off[p.U];
  for (int64_t slot = (int64_t)blockIdx.x * 4 + wave; slot < n_pop; slot += (int64_t)gridDim.x * 4) {
    const int64_t u = p.slot_user[slot];
    int zo = 0;
    asm volatile("" : "+v"(zo));
    // ---- dG[j][f] = sum_r P[r][j] dz[r][f], dK[j][f] = sum_r DS[r][j] q[r][f]: four rows a step, ascending; lane (r, g) = (j or f, row of the step)
    const int64_t rlo = p.row_off[u], rhi = p.row_off[u + 1];
    f32x4 accG[NT], accK[NT];
#pragma unroll
    for (int mt = 0; mt < NT; mt++) { accG[mt] = vzero; accK[mt] = vzero; }
    for (int64_t row0 = rlo; row0 < rhi; row0 += 4) {
      const int64_t row = row0 + g;
      const bool in = row < rhi;
      const float ap = in ? p.P[row * 16 + r] : 0.f, ad = in ? p.DS[row * 16 + r] : 0.f;
      const int32_t id = in ? p.idx[row] : -1;
#pragma unroll
      for (int mt = 0; mt < NT; mt++) {
        const float bz = in ? p.DZ[row * E + 16 * mt + r] : 0.f;
        const float bq = id >= 0 ? p.emb[(int64_t)id * E + 16 * mt + r] : 0.f;
        accG[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, bz, accG[mt], 0, 0, 0);
        accK[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad, bq, accK[mt], 0, 0, 0);
      }
    }
    // ---- lane (r, g) holds [j = 4 g + rr][f = 16 mt + r]: to the row-fragment layout ([j = r][f = 16 jc + 4 g + t]) through the wave's LDS
    f32x4 gv[NJ], kv[NJ], tv[NJ];
#pragma unroll
    for (int mt = 0; mt < NT; mt++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) X[(4 * g + rr) * LD + 16 * mt + r] = accG[mt][rr];
    DFM_WAVE_LDS_SYNC();
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) gv[jc] = *(const f32x4 *)(X + r * LD + 16 * jc + 4 * g);
    DFM_WAVE_LDS_SYNC();
#pragma unroll
    for (int mt = 0; mt < NT; mt++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) X[(4 * g + rr) * LD + 16 * mt + r] = accK[mt][rr];
    DFM_WAVE_LDS_SYNC();
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) kv[jc] = *(const f32x4 *)(X + r * LD + 16 * jc + 4 * g);
    DFM_WAVE_LDS_SYNC();               // (the next user overwrites X)
    // ---- dT = W1b^T dG, dk = dK + att.W^T dT
    din_csr_prod<E>(p.w1bTA + lane + zo, gv, tv, false);
    din_csr_prod<E>(p.attTA + lane + zo, tv, kv, true);
    const int64_t o = (slot * 16 + r) * E + 4 * g;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      *(f32x4 *)(p.dG + o + 16 * jc) = gv[jc];
      *(f32x4 *)(p.dT + o + 16 * jc) = tv[jc];
      if (r < p.L) *(f32x4 *)(p.dX + (p.B + u * p.L + r) * E + 16 * jc + 4 * g) = kv[jc];
    }
  }
}

// slabs [S][K][pc] -> gw [K][cols] += (row stride ldw) and gb [K] += column `cols` (or NULL: dropped), slab 0 first
__global__ void din_csr_slab_add_kernel(const float *part, int S, int K, int pc, int cols, float *gw, float *gb, int64_t ldw) {
  const int64_t n = (int64_t)K * pc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float s = part[i];
    for (int z = 1; z < S; z++) s += part[(int64_t)z * n + i];
    const int64_t k = i / pc;
    const int c = (int)(i % pc);
    if (c < cols) gw[k * ldw + c] += s; else if (gb && c == cols) gb[k] += s;
  }
}

// the E + 2 live columns of AUX: rows of a slab in row order (fp64), then slabs in slab order
__global__ __launch_bounds__(256) void din_csr_colsum_kernel(const float *aux, int64_t B, int EA, int64_t slabs, double *part) {
  const int c = threadIdx.x;
  if (c >= EA) return;
  for (int64_t z = blockIdx.x; z < slabs; z += gridDim.x) {
    const int64_t lo = z * DRT_SLAB, hi = lo + DRT_SLAB < B ? lo + DRT_SLAB : B;
    double s = 0.0;
    for (int64_t row = lo; row < hi; row++) s += (double)aux[row * EA + c];
    part[z * EA + c] = s;
  }
}
__global__ __launch_bounds__(256) void din_csr_tail_kernel(const double *part, int64_t slabs, int E, int64_t B, float *g_l2w, float *g_l2b, double *loss) {
  const int c = threadIdx.x, EA = E + 4;
  if (c >= E + 2) return;
  double s = 0.0;
  for (int64_t z = 0; z < slabs; z++) s += part[z * EA + c];
  if (c < E) g_l2w[c] += (float)s;
  else if (c == E) g_l2b[0] += (float)s;
  else loss[0] = s / (double)B;
}

// dfm_seg_heads_kernel, adding: the handle's gradient accumulates until dm_adam_step
__global__ __launch_bounds__(256) void din_csr_seg_heads_add_kernel(const unsigned long long *keys, const int32_t *vals, int64_t m, int64_t NR, const float *dX, int E, float *grad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < m; i += (int64_t)gridDim.x * 4) {
    const unsigned long long key = keys[i];
    if (key >= (unsigned long long)NR || (i > 0 && keys[i - 1] == key)) continue;
    const int64_t qe = drt_segment_end(keys, i, m, key, lane);
    const int64_t next = (i / DFM_SEG_CHUNK + 1) * DFM_SEG_CHUNK;
    float *dst = grad + (int64_t)key * E;
    for (int e = lane; e < E; e += 64) {
      float acc = dX[(int64_t)vals[i] * E + e];
      for (int64_t q = next; q < qe; q += DFM_SEG_CHUNK) acc += dX[(int64_t)vals[q] * E + e];
      dst[e] += acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline bool din_train_time_launches() { return env_on("DM_TRAIN_TIME_LAUNCHES"); }

// B + U L slots are sorted with 32-bit values; the slabs of the three products are a grid's z (B / 512 and U 16 / 512 of them)
static bool din_csr_too_large(int64_t U, int64_t B, int L) {
  return U > (int64_t)DRT_MAX_ROWS / 2 || B > (int64_t)DRT_MAX_ROWS || B + U * (int64_t)L >= ((int64_t)1 << 31);
}

static int train_fb_csr_dev(dm_ctx *h, const int32_t *d_seq, const uint32_t *d_umask, const int64_t *d_row_off, const int32_t *d_codes, const float *d_labels,
                            int64_t U, int64_t B, int L, float *loss) {
  const int E = h->embed, EA = E + 4;
  const int64_t NI = h->num_index, UL = U * L, m = B + UL, U16 = U * 16;
  const bool detail = din_train_time_launches();
  const int64_t slabs_b = (B + DRT_SLAB - 1) / DRT_SLAB, slabs_u = (U16 + DRT_SLAB - 1) / DRT_SLAB;
  unsigned nb = (unsigned)std::min<int64_t>((B / 16 + U + 3) / 4, (int64_t)h->n_cu * 8);       // rows kernel: at most B / 16 + U tiles
  unsigned nbu = (unsigned)std::min<int64_t>((U + 3) / 4, (int64_t)h->n_cu * 8);               // the two user kernels
  unsigned nbs = (unsigned)std::min<int64_t>(slabs_b, (int64_t)h->n_cu * 16);
  if (const long long g_ = env_int("DM_DIN_TRAIN_GRID")) nb = nbu = nbs = (unsigned)std::min<long long>(g_, 65535);      // (tests: partial rounds)
  int rc;
  // ---- the offsets, before anything dereferences through them, before the workspace is reserved and before the gradient is touched
  {
    unsigned long long *d_bad = (unsigned long long *)h->d_loss, bad = 0;      // (16 bytes of the training state; the row step zeroes them itself)
    HIPCHK(h, hipMemsetAsync(d_bad, 0xFF, 8, h->stream));
    if ((rc = LAUNCH(h, dfm_tg_check_off_kernel, dim3(drt_blocks(h, U + 1, 256)), dim3(256), 0, d_row_off, U, B, d_bad)) != DM_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad != ~0ull) {
      char msg[256];
      if (bad == (unsigned long long)U) snprintf(msg, sizeof msg, "dm_train_forward_backward_csr: row_off[U] must equal B = %lld (user %lld)", (long long)B, (long long)U);
      else snprintf(msg, sizeof msg, "dm_train_forward_backward_csr: row_off must start at 0 and never decrease (first offending user %llu)", bad);
      return fail(h, DM_ERR_INVALID, msg);
    }
  }
  DevArena ar(h->ws, 8);
  const size_t o_loss = ar.add(8), o_idx = ar.add((size_t)m * 4);
  const size_t o_tc = ar.add((size_t)(U + 1) * 8), o_to = ar.add((size_t)(U + 1) * 8);
  const size_t o_hc = ar.add((size_t)(U + 1) * 8), o_so = ar.add((size_t)(U + 1) * 8), o_su = ar.add((size_t)U * 4);
  const size_t o_K = ar.add((size_t)U16 * E * 4), o_T = ar.add((size_t)U16 * E * 4), o_G = ar.add((size_t)U16 * E * 4);
  const size_t o_dG = ar.add((size_t)U16 * E * 4), o_dT = ar.add((size_t)U16 * E * 4);
  const size_t o_dz = ar.add((size_t)B * E * 4), o_P = ar.add((size_t)B * 16 * 4), o_DS = ar.add((size_t)B * 16 * 4), o_aux = ar.add((size_t)B * EA * 4);
  const size_t o_dx = ar.add((size_t)m * E * 4);
  const size_t o_k0 = ar.add((size_t)m * 8), o_k1 = ar.add((size_t)m * 8), o_v0 = ar.add((size_t)m * 4), o_v1 = ar.add((size_t)m * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_part = ar.add(std::max((size_t)slabs_b * E * ((size_t)E + 1), (size_t)slabs_u * E * E) * 4);
  const size_t o_cs = ar.add((size_t)slabs_b * EA * 8);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  if ((rc = train_touch_reserve(h, (size_t)m)) != DM_OK) return rc;
  int32_t *idx = ar.ptr<int32_t>(o_idx);
  int64_t *tcnt = ar.ptr<int64_t>(o_tc), *toff = ar.ptr<int64_t>(o_to), *hcnt = ar.ptr<int64_t>(o_hc), *soff = ar.ptr<int64_t>(o_so);
  int32_t *suser = ar.ptr<int32_t>(o_su);
  float *grad = (float *)h->train.grad;
  float *g_att = grad + NI * E, *g_l1 = g_att + (int64_t)E * E, *g_l1b = g_l1 + (int64_t)E * 2 * E, *g_l2w = g_l1b + E, *g_l2b = g_l2w + E;
  LAUNCHCHK(h, din_csr_idx_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, d_codes, d_seq, d_row_off, B, U, L, NI, idx);
  LAUNCHCHK(h, din_csr_tilecnt_kernel, dim3(drt_blocks(h, U, 256)), dim3(256), 0, d_row_off, U, tcnt, hcnt);
  LAUNCHCHK(h, dm_sample_scan_kernel, dim3(1), dim3(1024), 0, tcnt, toff, U);
  LAUNCHCHK(h, dm_sample_scan_kernel, dim3(1), dim3(1024), 0, hcnt, soff, U);
  LAUNCHCHK(h, din_csr_slots_kernel, dim3(drt_blocks(h, U, 256)), dim3(256), 0, soff, U, suser);
  // ---- per user, per row, per user
  DinCsrParams p{};
  p.emb = (const float *)h->d_compact;
  p.attA = (const f32x4 *)h->d_attA; p.w1aA = (const f32x4 *)h->d_w1aA; p.w1bA = (const f32x4 *)h->d_w1bA;
  p.attTA = (const f32x4 *)h->d_attTA; p.w1aTA = (const f32x4 *)h->d_w1aTA; p.w1bTA = (const f32x4 *)h->d_w1bTA;
  p.b1 = (const float *)h->d_b1; p.w2 = (const float *)h->d_w2; p.b2 = (float)h->b2;
  p.inv_B = (float)(1.0 / (double)B); p.sm_scale = (float)sm_scale64(h);
  p.idx = idx; p.umask = d_umask; p.row_off = d_row_off; p.tile_off = toff; p.slot_off = soff; p.slot_user = suser; p.labels = d_labels; p.U = U; p.B = B; p.L = L;
  p.K = ar.ptr<float>(o_K); p.T = ar.ptr<float>(o_T); p.G = ar.ptr<float>(o_G); p.dG = ar.ptr<float>(o_dG); p.dT = ar.ptr<float>(o_dT);
  p.DZ = ar.ptr<float>(o_dz); p.P = ar.ptr<float>(o_P); p.DS = ar.ptr<float>(o_DS); p.AUX = ar.ptr<float>(o_aux); p.dX = ar.ptr<float>(o_dx);
  rc = timed(h, EV_DTC_SETUP, detail, [&] {
    return dispatch_E(h, E, "unsupported embed size", [&](auto e) { return LAUNCH(h, din_csr_setup_kernel<decltype(e)::value>, dim3(nbu), dim3(256), 0, p); }); });
  if (rc != DM_OK) return rc;
  rc = timed(h, EV_DTC_ROWS, detail, [&] {
    return dispatch_E(h, E, "unsupported embed size", [&](auto e) { return LAUNCH(h, din_csr_rows_kernel<decltype(e)::value>, dim3(nb), dim3(256), 0, p); }); });
  if (rc != DM_OK) return rc;
  rc = timed(h, EV_DTC_USER_BWD, detail, [&] {
    return dispatch_E(h, E, "unsupported embed size", [&](auto e) { return LAUNCH(h, din_csr_user_bwd_kernel<decltype(e)::value>, dim3(nbu), dim3(256), 0, p); }); });
  if (rc != DM_OK) return rc;
  // ---- the dense gradients
  rc = timed(h, EV_DTC_DW, detail, [&]() -> int {
    float *part = ar.ptr<float>(o_part);
    double *cs = ar.ptr<double>(o_cs);
    LAUNCHCHK(h, din_csr_colsum_kernel, dim3(nbs), dim3(256), 0, p.AUX, B, EA, slabs_b, cs);
    LAUNCHCHK(h, din_csr_tail_kernel, dim3(1), dim3(256), 0, cs, slabs_b, E, B, g_l2w, g_l2b, ar.ptr<double>(o_loss));
    // g_W1a, g_l1.b: dz^T [E x B] . [Q | 1]
    DrtGemmParams<float> gp{};
    gp.A = p.DZ; gp.a_rs = 1; gp.a_cs = E;
    gp.B = p.emb; gp.gidx = idx; gp.Lg = 1; gp.E = E; gp.gcols = E;
    gp.C = part; gp.ldc = E + 1; gp.c_slab = (int64_t)E * (E + 1); gp.M = E; gp.N = E + 1; gp.Kd = B; gp.slab = DRT_SLAB;
    int rc_ = drt_launch_gemm<float>(h, gp, EV_DTC_DW, false);
    if (rc_ != DM_OK) return rc_;
    LAUNCHCHK(h, din_csr_slab_add_kernel, dim3(drt_blocks(h, (int64_t)E * (E + 1), 256)), dim3(256), 0, part, (int)slabs_b, E, E + 1, E, g_l1, g_l1b, (int64_t)2 * E);
    // g_W1b = dG^T T, g_att.W = dT^T K over the U 16 per-user rows
    gp.gidx = nullptr; gp.Lg = 0; gp.gcols = 0; gp.b_rs = 1; gp.b_cs = E;
    gp.ldc = E; gp.c_slab = (int64_t)E * E; gp.N = E; gp.Kd = U16;
    gp.A = p.dG; gp.B = p.T;
    if ((rc_ = drt_launch_gemm<float>(h, gp, EV_DTC_DW, false)) != DM_OK) return rc_;
    LAUNCHCHK(h, din_csr_slab_add_kernel, dim3(drt_blocks(h, (int64_t)E * E, 256)), dim3(256), 0, part, (int)slabs_u, E, E, E, g_l1 + E, nullptr, (int64_t)2 * E);
    gp.A = p.dT; gp.B = p.K;
    if ((rc_ = drt_launch_gemm<float>(h, gp, EV_DTC_DW, false)) != DM_OK) return rc_;
    LAUNCHCHK(h, din_csr_slab_add_kernel, dim3(drt_blocks(h, (int64_t)E * E, 256)), dim3(256), 0, part, (int)slabs_u, E, E, E, g_att, nullptr, (int64_t)E);
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  // ---- the table: sort the B + U L slots by destination row, chunk sums, one wave per destination adds its heads
  rc = timed(h, EV_DTC_EMB, detail, [&]() -> int {
    const DrtSortBufs sb{ar.ptr<unsigned long long>(o_k0), ar.ptr<unsigned long long>(o_k1), ar.ptr<int32_t>(o_v0), ar.ptr<int32_t>(o_v1), ar.ptr<uint32_t>(o_tmp)};
    const unsigned long long *ks;
    const int32_t *vs;
    int rc_ = drt_sort_slots(h, idx, m, NI, sb, ks, vs);
    if (rc_ != DM_OK) return rc_;
    LAUNCHCHK(h, dfm_seg_chunks_kernel, dim3(drt_blocks(h, m, 4)), dim3(256), 0, ks, vs, m, NI, p.dX, E);
    LAUNCHCHK(h, din_csr_seg_heads_add_kernel, dim3(drt_blocks(h, m, 4)), dim3(256), 0, ks, vs, m, NI, p.dX, E, grad);
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  // rows the gradient reached: the candidates and the histories of users that have rows (the others' slots are -1 in idx)
  LAUNCHCHK(h, dm_mark_touched_kernel, dim3(256), dim3(256), 0, idx, nullptr, m, 0, h->d_touch_bits, h->d_touch_list, h->d_touch_cnt, h->touch_cap, NI);
  if ((rc = h->train.mark_active(h, 256, idx, m)) != DM_OK) return rc;
  double l = 0.0;
  HIPCHK(h, hipMemcpyAsync(&l, ar.ptr<double>(o_loss), 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->last_loss = (double)(float)l;
  if (loss) *loss = (float)l;
  return DM_OK;
}

int dm_train_forward_backward_csr_dev(dm_handle_t h, const int32_t *d_seq_codes, const uint32_t *d_umask, const int64_t *d_row_off, const int32_t *d_codes,
                                      const float *d_labels, int64_t U, int64_t B, int L, float *loss) {
  if (!h) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_forward_backward_csr_dev");
  if (rc != DM_OK) return rc;
  if (h->dtype == DM_F64)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_train_forward_backward_csr_dev: f32 models only (an f64 model keeps dm_train_forward_backward_grouped_dev)");
  if (U <= 0 || B <= 0 || !d_seq_codes || !d_row_off || !d_codes || !d_labels || L < 1 || L > DM_PIPE_MAXL)
    return fail(h, DM_ERR_INVALID, "dm_train_forward_backward_csr_dev: U and B must be positive, the arrays other than d_umask non-null and L in 1..32");
  if (L > DM_MAXL) return fail(h, DM_ERR_UNSUPPORTED, "dm_train_forward_backward_csr_dev: histories longer than 16 keep the row step");
  if (din_csr_too_large(U, B, L))
    return fail(h, DM_ERR_UNSUPPORTED, "dm_train_forward_backward_csr_dev: batch too large (at most 4 194 240 rows, 2 097 120 users, and B + U L below 2^31): split it and accumulate");
  HIPCHK(h, hipSetDevice(h->device));
  return train_fb_csr_dev(h, d_seq_codes, d_umask, d_row_off, d_codes, d_labels, U, B, L, loss);
}
