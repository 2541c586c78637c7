// DeepFM training step, user-grouped form (dm_deepfm_train_forward_backward_grouped_dev; DESIGN.md §16): the step of dfm_train.hip.inc on a
// batch given as U histories seq[u][0..L) and R candidate rows per user (code[u][r], y[u][r]), B = U R, never expanded to B copies of every
// history.  The graph has no mask and its hidden layer is T = L + 1 units wide, so all that depends on a history is computed once per user,
// exactly (notation of dfm_train.hip.inc; x_j = emb[seq[u][j]], x_c = emb[code[u][r]], W1_i = block i of l1.W, block 0 the candidate's):
//   per user   bufh = sum_j x_j      sqh = sum_j |x_j|^2      Hh = sum_j x_j W1_{1+j}^T
//   per row    zpre = Hh + x_c W1_0^T + l1.b     buf = bufh + x_c     fm = (|buf|^2 - sqh - |x_c|^2) / 2     h, z, loss, g_r, dh_r as the row step
//              dXc_r = dh_r W1_0 + g_r bufh                                      (= the row step's dh W1_0 + g (buf - x_c))
//   per user   DH = sum_r dh_r     Gs = sum_r g_r     GBc = sum_r g_r x_c,r     dXh_j = DH W1_{1+j} + (Gs bufh + GBc) - Gs x_j
//   g_l1W      block 0 = sum_r dh_r (x) x_c,r      blocks 1 + j = sum_u DH_u (x) x_j,u      g_l1b = sum_r dh_r
//   g_emb      scatters dXc (B slots) and dXh (U L slots) to the rows they read
//
// Kernels (the fragment orders of l1.W are dfm_train_derive_kernel's fragF / fragB, read through L2):
//   dfm_tg_idx_kernel       [codes ; seq] as one index array of B + U L slots; an id outside [0, num_index) becomes -1
//   dfm_tg_setup_kernel     one wave per tile of 16 users: pass 1 of dfm_train_rows_kernel over blocks 1 .. L -> Hh, bufh, sqh
//   dfm_tg_rows_kernel      one wave per 16 consecutive rows of B, u = row / R (a tile may straddle users): gathers the candidate block
//                           only, starts the accumulators from Hh[u(row)], the row step's epilogue, pass 2 for block 0 -> dH, g, dXc
//   dfm_tg_user_bwd_kernel  one wave per tile of 16 users: lane (g, r) walks user r's R rows in row order and adds g x_c (its own
//                           features: GBc in the gather layout), dH[row][4 ks + g] (DH in pass 2's operand layout) and g; then pass 2
//                           over blocks 1 .. L with DH as the operand -> dXh, DH
//   dfm_train_sum_kernel, drt_gemm_kernel<float> (twice: the B rows through [codes] for block 0 and l1.b, the U users through [seq] for
//   blocks 1 .. L), drt_slab_sum_kernel, drt_sort_slots + dfm_seg_chunks_kernel + dfm_seg_heads_kernel over the B + U L slots
// Nothing of size B x L E is read or written.  No floating-point atomics; every sum has a fixed order.
//
// Ragged (CSR) form (dm_deepfm_train_forward_backward_csr_dev; DESIGN.md §17): rows row_off[u] .. row_off[u + 1] of codes / labels belong to
// user u, a user may have none.  The same kernels with CSR = true: the rows kernel reads the user of a row from row_user [B] where the
// rectangular instance divides by R, the user-backward kernel walks row_off[u] .. row_off[u + 1] (lanes of a tile have different trip
// counts; still no cross-lane sum, rows ascending).  Two more kernels:
//   dfm_tg_check_off_kernel  row_off[0] == 0, non-decreasing, row_off[U] == B: the first offending user by an integer atomicMin, read back
//                            before any other kernel dereferences through the offsets
//   dfm_tg_idx_csr_kernel    dfm_tg_idx_kernel, plus row_user by a binary search of row_off per row, and -1 for all L history slots of a
//                            user without rows (it scatters nothing, and dfm_train_emb_grad never marks its history)

__global__ void dfm_tg_idx_kernel(const int32_t *codes, const int32_t *seq, int64_t B, int64_t UL, int64_t num_index, int32_t *idx) {
  const int64_t n = B + UL;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t id = i < B ? codes[i] : seq[i - B];
    idx[i] = (id >= 0 && id < num_index) ? id : -1;
  }
}

// first u whose offsets are wrong: 0 for row_off[0] != 0, u for row_off[u + 1] < row_off[u], U for row_off[U] != B; *bad starts at ~0
__global__ void dfm_tg_check_off_kernel(const int64_t *row_off, int64_t U, int64_t B, unsigned long long *bad) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u <= U; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = row_off[u];
    const bool wrong = u == U ? a != B : ((u == 0 && a != 0) || row_off[u + 1] < a);
    if (wrong) atomicMin(bad, (unsigned long long)u);
  }
}

// row_off has passed dfm_tg_check_off_kernel: 0 = row_off[0] <= .. <= row_off[U] = B
__global__ void dfm_tg_idx_csr_kernel(const int32_t *codes, const int32_t *seq, const int64_t *row_off, int64_t B, int64_t U, int L, int64_t num_index,
                                      int32_t *idx, int32_t *row_user) {
  const int64_t n = B + U * L;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t id;
    if (i < B) {
      id = codes[i];
      int64_t lo = 0, hi = U;            // the last u with row_off[u] <= i: row_off[lo] <= i < row_off[hi] throughout
      while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (row_off[mid] <= i) lo = mid; else hi = mid; }
      row_user[i] = (int32_t)lo;
    } else {
      const int64_t u = (i - B) / L;
      id = row_off[u + 1] > row_off[u] ? seq[i - B] : -1;
    }
    idx[i] = (id >= 0 && id < num_index) ? id : -1;
  }
}

struct DfmTgParams {
  const float *emb, *l1_b, *l2_w, *l2_b;
  const f32x4 *fragF, *fragB;
  const int32_t *idx;                  // [B] candidates, then [U][L] histories
  const float *labels;                 // [B]
  int64_t U, B;
  int R, T;
  float *Hh, *bufh, *sqh;              // [U][NC], [U][E], [U]
  float *dH, *g, *dX;                  // [B][NC] (columns >= T: 0), [B], [B + U L][E]: dXc, then dXh
  float *DH;                           // [U][NC]
  double *ploss;                       // [gridDim.x] of the rows kernel
  float *pg;                           // [gridDim.x][1 + NC]: g_l2b, g_l2W
  const int32_t *row_user;             // CSR instances only: [B] the user of a row
  const int64_t *row_off;              // CSR instances only: [U + 1]
};

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_tg_setup_kernel(DfmTgParams p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int L = p.T - 1;
  const int64_t tiles = (p.U + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t u0 = tile * 16, myu = u0 + r;
    const bool in = myu < p.U;
    const int32_t *ids = p.idx + p.B + myu * L;
    f32x4 buf[NJ], acc[NCT];
    float sq = 0.0f;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) buf[jc] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int i = 1; i <= L; i++) {
      const int32_t id = in ? ids[i - 1] : -1;
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
    sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
    if (in) {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) *(f32x4 *)(p.bufh + myu * E + 16 * jc + 4 * g) = buf[jc];
      if (g == 0) p.sqh[myu] = sq;
    }
    // C layout: lane (g, r) holds users 4 g .. 4 g + 3 of column 16 ct + r
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++)
        if (u0 + 4 * g + rr < p.U) p.Hh[(u0 + 4 * g + rr) * NC + 16 * ct + r] = acc[ct][rr];
  }
}

template <int E, int NCT, bool CSR = false>
__global__ __launch_bounds__(256) void dfm_tg_rows_kernel(DfmTgParams p) {
  constexpr int NJ = E / 16, NC = NCT * 16, LDH = NC + 1;
  __shared__ float dhl[4][16 * LDH];
  __shared__ double wloss[4];
  __shared__ float wpg[4][1 + NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int64_t tiles = (p.B + 15) / 16;
  const DfmTrainEpi q{p.l1_b, p.l2_w, p.labels, p.dH, p.g, p.B, p.T, (float)p.B, p.l2_b[0]};
  double lsum = 0.0;
  float gsum = 0.0f, pw2[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) pw2[ct] = 0.0f;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 16, myrow = row0 + r;
    const bool in = myrow < p.B;
    int64_t myu = 0;
    if constexpr (CSR) { if (in) myu = p.row_user[myrow]; } else myu = in ? myrow / p.R : 0;
    const int32_t id = in ? p.idx[myrow] : -1;
    // ---- pass 1, block 0 only: H = Hh[u] + x_c W1_0^T, buf = bufh[u] + x_c
    f32x4 bh[NJ], x[NJ], acc[NCT];
    float sqc = 0.0f, ss = 0.0f;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      bh[jc] = in ? *(const f32x4 *)(p.bufh + myu * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
      x[jc] = id >= 0 ? *(const f32x4 *)(p.emb + (int64_t)id * E + 16 * jc + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
      const f32x4 buf = bh[jc] + x[jc];
#pragma unroll
      for (int c = 0; c < 4; c++) { sqc = fmaf(x[jc][c], x[jc][c], sqc); ss = fmaf(buf[c], buf[c], ss); }
    }
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {                    // each of the lane's four C-layout rows reads its own user
      const int64_t row = row0 + 4 * g + rr;
      int64_t ru = 0;
      if constexpr (CSR) { if (row < p.B) ru = p.row_user[row]; } else ru = row < p.B ? row / p.R : 0;
      const float *hh = p.Hh + ru * NC + r;
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) acc[ct][rr] = row < p.B ? hh[16 * ct] : 0.0f;
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 b = p.fragF[((int64_t)ct * NJ + jc) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 4; c++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[jc][c], b[c], acc[ct], 0, 0, 0);
      }
    ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);
    sqc += __shfl_xor(sqc, 16); sqc += __shfl_xor(sqc, 32);
    const float fm = 0.5f * ((ss - (in ? p.sqh[myu] : 0.0f)) - sqc);        // of row r, in every lane (., r)
    // ---- the row step's epilogue (dfm_train_epilogue; it also keeps g [B]), then pass 2, block 0 only: dXc^T = W1_0^T dH^T + g bufh
    float grow, dhb[4 * NCT];
    dfm_train_epilogue<NCT>(q, acc, fm, row0, r, g, dhl[wave], lsum, gsum, pw2, grow, dhb);
    float *dst = p.dX + myrow * E + 4 * g;
#pragma unroll
    for (int jn = 0; jn < NJ; jn++) {
      f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kq = 0; kq < NCT; kq++) {
        const f32x4 a = p.fragB[((int64_t)jn * NCT + kq) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 4; c++) c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], dhb[4 * kq + c], c4, 0, 0, 0);
      }
#pragma unroll
      for (int c = 0; c < 4; c++) c4[c] = fmaf(grow, bh[jn][c], c4[c]);
      if (in) *(f32x4 *)(dst + 16 * jn) = c4;
    }
    DFM_WAVE_LDS_SYNC();               // the next tile overwrites dhl
  }
  dfm_train_partials<NCT>(lsum, gsum, pw2, wloss, wpg, p.ploss, p.pg);
}

template <int E, int NCT, bool CSR = false>
__global__ __launch_bounds__(256) void dfm_tg_user_bwd_kernel(DfmTgParams p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int L = p.T - 1, R = p.R;
  const int64_t tiles = (p.U + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t myu = tile * 16 + r;
    const bool in = myu < p.U;
    // ---- the user's rows in row order: Gs, GBc (this lane's features), DH (units 4 ks + g): no cross-lane sum
    f32x4 gbc[NJ];
    float gs = 0.0f, dhb[4 * NCT];
#pragma unroll
    for (int jn = 0; jn < NJ; jn++) gbc[jn] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4 * NCT; ks++) dhb[ks] = 0.0f;
    if (in) {
      int64_t rlo = myu * R;
      int nr = R;                      // (CSR: the lanes of a tile have different trip counts; nothing in the loop crosses lanes)
      if constexpr (CSR) { rlo = p.row_off[myu]; nr = (int)(p.row_off[myu + 1] - rlo); }
      for (int q = 0; q < nr; q++) {
        const int64_t row = rlo + q;
        const float gv = p.g[row];
        const int32_t id = p.idx[row];
        gs += gv;
#pragma unroll
        for (int ks = 0; ks < 4 * NCT; ks++) dhb[ks] += p.dH[row * NC + 4 * ks + g];
        if (id >= 0) {
#pragma unroll
          for (int jn = 0; jn < NJ; jn++) {
            const f32x4 x = *(const f32x4 *)(p.emb + (int64_t)id * E + 16 * jn + 4 * g);
#pragma unroll
            for (int c = 0; c < 4; c++) gbc[jn][c] = fmaf(gv, x[c], gbc[jn][c]);
          }
        }
      }
#pragma unroll
      for (int ks = 0; ks < 4 * NCT; ks++) p.DH[myu * NC + 4 * ks + g] = dhb[ks];
      // base = Gs bufh + GBc
#pragma unroll
      for (int jn = 0; jn < NJ; jn++) {
        const f32x4 bh = *(const f32x4 *)(p.bufh + myu * E + 16 * jn + 4 * g);
#pragma unroll
        for (int c = 0; c < 4; c++) gbc[jn][c] = fmaf(gs, bh[c], gbc[jn][c]);
      }
    }
    // ---- pass 2 over blocks 1 .. L: dXh_j^T = W1_{1+j}^T DH^T + base - Gs x_j
    const int32_t *ids = p.idx + p.B + myu * L;
    for (int i = 1; i <= L; i++) {
      const int32_t id = in ? ids[i - 1] : -1;
      float *dst = p.dX + (p.B + myu * L + (i - 1)) * E + 4 * g;
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
        for (int c = 0; c < 4; c++) c4[c] += fmaf(-gs, x[c], gbc[jn][c]);
        if (in) *(f32x4 *)(dst + 16 * jn) = c4;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline bool dfm_train_grouped_enabled() { return env_on("DM_DFM_TRAIN_GROUPED"); }

template <int E, int NCT, bool CSR>
static int dfm_tg_launch(dm_ctx *h, const DfmTgParams &p, int which, unsigned nb, bool on) {
  return timed(h, which == 0 ? EV_DFG_SETUP : which == 1 ? EV_DFG_ROWS : EV_DFG_USER_BWD, on, [&] {
    return which == 0   ? LAUNCH(h, (dfm_tg_setup_kernel<E, NCT>), dim3(nb), dim3(256), 0, p)
           : which == 1 ? LAUNCH(h, (dfm_tg_rows_kernel<E, NCT, CSR>), dim3(nb), dim3(256), 0, p)
                        : LAUNCH(h, (dfm_tg_user_bwd_kernel<E, NCT, CSR>), dim3(nb), dim3(256), 0, p);
  });
}

static bool dfm_tg_too_large(int64_t U, int64_t R, int L) {
  if (U > (int64_t)DRT_MAX_ROWS || R > (int64_t)DRT_MAX_ROWS) return true;       // (before the product: U R cannot overflow)
  const int64_t B = U * R;
  return B > (int64_t)DRT_MAX_ROWS || B + U * (int64_t)L >= ((int64_t)1 << 31);
}

static bool dfm_tg_csr_too_large(int64_t U, int64_t B, int L) {
  return U > (int64_t)DRT_MAX_ROWS || B > (int64_t)DRT_MAX_ROWS || B + U * (int64_t)L >= ((int64_t)1 << 31);
}

// d_row_off == nullptr: the rectangular batch, B = U R.  Otherwise the ragged one: rows row_off[u] .. row_off[u + 1] are user u's, R is unused
static int dfm_train_fb_grouped_dev(dm_ctx *h, const int32_t *d_seq, const int64_t *d_row_off, const int32_t *d_codes, const float *d_labels, int64_t U, int R,
                                    int64_t B_csr, double *out_loss) {
  dm_dfm_train *t = h->dfm_tr;
  const bool csr = d_row_off != nullptr;
  const int E = h->embed, L = h->dfm_L, T = L + 1, NCT = dfm_train_col_tiles(L), NC = 16 * NCT;
  // B + U L slots are sorted with 32-bit values; the slabs of the l1.W products are a grid's z
  if (csr && dfm_tg_csr_too_large(U, B_csr, L))
    return fail(h, DM_ERR_UNSUPPORTED, "dm_deepfm_train_forward_backward_csr: batch too large (at most 4 194 240 rows and as many users, and B + U L below 2^31): split it and accumulate on the host");
  if (!csr && dfm_tg_too_large(U, R, L))
    return fail(h, DM_ERR_UNSUPPORTED, "dm_deepfm_train_forward_backward_grouped: batch too large (at most 4 194 240 rows, and U rows_per_user + U L below 2^31): split it and accumulate on the host");
  const int64_t NI = h->num_index, B = csr ? B_csr : U * R, UL = U * L, m = B + UL;
  const bool detail = dfm_time_launches();
  const int64_t slabs_b = (B + DRT_SLAB - 1) / DRT_SLAB, slabs_u = (U + DRT_SLAB - 1) / DRT_SLAB;
  int nb = (int)std::min<int64_t>(((B + 15) / 16 + 3) / 4, 1024);            // workgroups of the rows kernel: a function of (U, R) alone
  int nbu = (int)std::min<int64_t>(((U + 15) / 16 + 3) / 4, 1024);           // ... and of the two user kernels
  if (const long long g_ = env_int("DM_DFM_TRAIN_GRID")) nb = nbu = (int)std::min<long long>(g_, 65535);      // (tests: partial rounds)
  int rc;
  DevArena ar(t->ws, 8);
  const size_t o_idx = ar.add((size_t)m * 4), o_hh = ar.add((size_t)U * NC * 4), o_bufh = ar.add((size_t)U * E * 4), o_sqh = ar.add((size_t)U * 4);
  const size_t o_dh = ar.add((size_t)B * NC * 4), o_g = ar.add((size_t)B * 4), o_dx = ar.add((size_t)m * E * 4), o_DH = ar.add((size_t)U * NC * 4);
  const size_t o_k0 = ar.add((size_t)m * 8), o_k1 = ar.add((size_t)m * 8), o_v0 = ar.add((size_t)m * 4), o_v1 = ar.add((size_t)m * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_part = ar.add(std::max((size_t)slabs_b * T * ((size_t)E + 1), (size_t)slabs_u * T * ((size_t)L * E + 1)) * 4);
  const size_t o_pl = ar.add((size_t)nb * 8), o_pg = ar.add((size_t)nb * (1 + NC) * 4), o_loss = ar.add(8);
  const size_t o_ru = csr ? ar.add((size_t)B * 4) : 0, o_bad = csr ? ar.add(8) : 0;
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  // ---- the offsets, before anything dereferences through them (and before the gradient is touched)
  if (csr) {
    unsigned long long *d_bad = ar.ptr<unsigned long long>(o_bad), bad = 0;
    HIPCHK(h, hipMemsetAsync(d_bad, 0xFF, 8, h->stream));
    if ((rc = LAUNCH(h, dfm_tg_check_off_kernel, dim3(drt_blocks(h, U + 1, 256)), dim3(256), 0, d_row_off, U, B, d_bad)) != DM_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad != ~0ull) {
      char msg[256];
      if (bad == (unsigned long long)U) snprintf(msg, sizeof msg, "dm_deepfm_train_forward_backward_csr: row_off[U] must equal B = %lld (user %lld)", (long long)B, (long long)U);
      else snprintf(msg, sizeof msg, "dm_deepfm_train_forward_backward_csr: row_off must start at 0 and never decrease (first offending user %llu)", bad);
      return fail(h, DM_ERR_INVALID, msg);
    }
  }
  int32_t *idx = ar.ptr<int32_t>(o_idx);
  float *dX = ar.ptr<float>(o_dx), *part = ar.ptr<float>(o_part);
  float *grad = (float *)t->vec.grad;
  float *g_l1w = grad + NI * E, *g_l1b = g_l1w + (int64_t)T * T * E, *g_l2w = g_l1b + T, *g_l2b = g_l2w + T;
  // ---- zeroGradParameters: the rows the last batch reached (the dense blocks are overwritten below)
  if ((rc = dfm_train_clear_prev(h, t)) != DM_OK) return rc;
  rc = csr ? LAUNCH(h, dfm_tg_idx_csr_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, d_codes, d_seq, d_row_off, B, U, L, NI, idx, ar.ptr<int32_t>(o_ru))
           : LAUNCH(h, dfm_tg_idx_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, d_codes, d_seq, B, UL, NI, idx);
  if (rc != DM_OK) return rc;
  // ---- per user, per row, per user
  DfmTgParams p;
  {
    const DfmBlocks b = dfm_blocks(h);
    p.emb = h->d_emb32; p.l1_b = b.l1_b; p.l2_w = b.l2_w; p.l2_b = b.l2_b; p.fragF = (const f32x4 *)t->fragF; p.fragB = (const f32x4 *)t->fragB;
    p.idx = idx; p.labels = d_labels; p.U = U; p.B = B; p.R = R; p.T = T;
    p.Hh = ar.ptr<float>(o_hh); p.bufh = ar.ptr<float>(o_bufh); p.sqh = ar.ptr<float>(o_sqh);
    p.dH = ar.ptr<float>(o_dh); p.g = ar.ptr<float>(o_g); p.dX = dX; p.DH = ar.ptr<float>(o_DH);
    p.ploss = ar.ptr<double>(o_pl); p.pg = ar.ptr<float>(o_pg);
    p.row_user = csr ? ar.ptr<const int32_t>(o_ru) : nullptr; p.row_off = d_row_off;
    for (int which = 0; which < 3; which++) {
      rc = dispatch_E_NCT(h, E, NCT, "unsupported embed size", [&](auto e, auto n) {
        const unsigned nbw = (unsigned)(which == 1 ? nb : nbu);
        return csr ? dfm_tg_launch<decltype(e)::value, decltype(n)::value, true>(h, p, which, nbw, detail)
                   : dfm_tg_launch<decltype(e)::value, decltype(n)::value, false>(h, p, which, nbw, detail); });
      if (rc != DM_OK) return rc;
    }
    if ((rc = LAUNCH(h, dfm_train_sum_kernel, dim3(1), dim3(64), 0, p.ploss, p.pg, nb, NC, T, B, ar.ptr<double>(o_loss), g_l2w, g_l2b)) != DM_OK) return rc;
  }
  // ---- g_l1W, g_l1b: dH^T [T x B] . [Xc | 1] into block 0 and l1.b, then DH^T [T x U] . Xh into blocks 1 .. L; slabs added in slab order
  {
    const int ldw = T * E;
    DrtGemmParams<float> g{};
    g.A = p.dH; g.a_rs = 1; g.a_cs = NC;
    g.B = h->d_emb32; g.gidx = idx; g.Lg = 1; g.E = E; g.gcols = E;
    g.C = part; g.ldc = E + 1; g.c_slab = (int64_t)T * (E + 1); g.M = T; g.N = E + 1; g.Kd = B; g.slab = DRT_SLAB;
    if ((rc = drt_launch_gemm<float>(h, g, EV_DFT_DW, detail)) != DM_OK) return rc;
    rc = timed(h, EV_DFT_DW, detail, [&] {
      return LAUNCH(h, drt_slab_sum_kernel<float>, dim3(drt_blocks(h, (int64_t)T * (E + 1), 256)), dim3(256), 0, part, (int)slabs_b, T, E, g_l1w, g_l1b, ldw);
    });
    if (rc != DM_OK) return rc;
    const int cols = L * E;            // (the ones column of this product is computed and dropped: l1.b came with the rows)
    g.A = p.DH; g.gidx = idx + B; g.Lg = L; g.gcols = cols;
    g.ldc = cols + 1; g.c_slab = (int64_t)T * (cols + 1); g.N = cols + 1; g.Kd = U;
    if ((rc = drt_launch_gemm<float>(h, g, EV_DFT_DW, detail)) != DM_OK) return rc;
    rc = timed(h, EV_DFT_DW, detail, [&] {
      return LAUNCH(h, drt_slab_sum_kernel<float>, dim3(drt_blocks(h, (int64_t)T * (cols + 1), 256)), dim3(256), 0, part, (int)slabs_u, T, cols, g_l1w + E, nullptr, ldw);
    });
    if (rc != DM_OK) return rc;
  }
  // ---- g_emb: sort the B + U L slots by destination row, chunk sums, one wave per destination
  {
    const DrtSortBufs sb{ar.ptr<unsigned long long>(o_k0), ar.ptr<unsigned long long>(o_k1), ar.ptr<int32_t>(o_v0), ar.ptr<int32_t>(o_v1), ar.ptr<uint32_t>(o_tmp)};
    if ((rc = dfm_train_emb_grad(h, t, idx, m, dX, sb, detail)) != DM_OK) return rc;
  }
  if (out_loss) HIPCHK(h, hipMemcpyAsync(out_loss, ar.ptr<double>(o_loss), 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_deepfm_train_forward_backward_grouped_dev(dm_handle_t h, const int32_t *d_seq_codes, const int32_t *d_codes, const float *d_labels, int64_t U, int rows_per_user,
                                                 int L, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_forward_backward_grouped");
  int rc = dfm_train_check(h, "dm_deepfm_train_forward_backward_grouped", true);
  if (rc != DM_OK) return rc;
  if (U <= 0 || rows_per_user <= 0 || !d_seq_codes || !d_codes || !d_labels)
    return fail(h, DM_ERR_INVALID, "dm_deepfm_train_forward_backward_grouped: U and rows_per_user must be positive and the arrays non-null");
  if ((rc = dfm_check_L(h, "dm_deepfm_train_forward_backward_grouped", L)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return dfm_train_fb_grouped_dev(h, d_seq_codes, nullptr, d_codes, d_labels, U, rows_per_user, 0, out_loss);
}

int dm_deepfm_train_forward_backward_csr_dev(dm_handle_t h, const int32_t *d_seq_codes, const int64_t *d_row_off, const int32_t *d_codes, const float *d_labels,
                                             int64_t U, int64_t B, int L, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_forward_backward_csr");
  int rc = dfm_train_check(h, "dm_deepfm_train_forward_backward_csr", true);
  if (rc != DM_OK) return rc;
  if (U <= 0 || B <= 0 || !d_seq_codes || !d_row_off || !d_codes || !d_labels)
    return fail(h, DM_ERR_INVALID, "dm_deepfm_train_forward_backward_csr: U and B must be positive and the arrays non-null");
  if ((rc = dfm_check_L(h, "dm_deepfm_train_forward_backward_csr", L)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return dfm_train_fb_grouped_dev(h, d_seq_codes, d_row_off, d_codes, d_labels, U, 0, B, out_loss);
}
