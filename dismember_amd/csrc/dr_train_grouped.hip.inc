// Deep-Retrieval E-step, the LAYER model's step on a SAMPLE-GROUPED batch (dm_dr_train_forward_backward_grouped*, dm_dr_layer_loss;
// DESIGN.md §24).  transformLayerData (D/dataset/MiniBatch.scala:18-50) repeats a sample's history once per path of its target item;
// the row step (dr_train.hip.inc) then multiplies every history J times on identical operands.  Here the batch is S samples with J paths
// each, row r = s J + j, R = S J, every mean over R: the row step on the expanded batch, re-associated.
//
//   Wh_d = the first L E columns of W_d, Wn_d the rest;  Xs[s] = the gathered history;  Xn_d[r] = the d node rows of path r
//   H[s]    = Xs[s] [Wh_0 .. Wh_{D-1}]^T + [b_0 .. b_{D-1}]                       one [S x LE] . [LE x DK] product over d_wseq
//   Z_d[r]  = H[s(r), dK ..] + Xn_d[r] Wn_d^T  (d >= 1);  Z_0 is H's first K columns, the same for the J rows of a sample
//   G_d     = (softmax(Z_d) - onehot) / R  (d >= 1, written);  Gs_d[s] = sum_j G_d[sJ + j];  Gs_0[s] = (J P_0[s] - sum_j onehot) / R
//   dXh     = Gs Wseq                                                              one [S x DK] . [DK x LE] product
//   dW_d[:, :LE], db_d = Gs_d^T [Xs | 1] over S;  dW_d[:, LE:] = G_d^T Xn_d over R;  dXn_d = G_d Wn_d, added layer by layer
//   demb    one stable sort over S L history slots followed by R (D-1) node slots (the row step sorts R (L + D - 1))
//
// The biases: d_sbias is refreshed by dr_derive only, so it is stale during training.  The forward copies the D bias blocks into it on
// every call (D copies of K values; the values dr_derive would write, so the search's copy is never wrong because of it).
// Kernels: dr_gemm_kernel (forward), drt_gemm_kernel / drt_slab_sum_kernel (backward), drt_seg_rows_kernel (demb) as the row step uses
// them, with other operands; new are the index builder and the softmax / cross-entropy that walks a sample's J rows.
// No floating-point atomics, a fixed order in every sum; the handle is left as the row step leaves it (prev keys, the clear of the last
// batch's rows, exchanged = false, dense blocks overwritten): dm_dr_adam_step and dm_dr_train_sync_gradients follow unchanged.

// all[i]: the embedding row of slot i: history slots [S x L] first, then node slots [R x (D-1)] (-1: padding).  idx[d][r][t], t < d,
// 1 <= d < D: the node rows that feed layer d's input; idx[D-1] IS the node part of all.
struct DrtgIdxParams { const int32_t *seq, *paths; int64_t SL, R; int D, K; int64_t num_item; int32_t *all; int32_t *idx[DR_MAXD]; };
__global__ void drtg_build_idx_kernel(DrtgIdxParams p) {
  const int Dn = p.D - 1;
  const int64_t n = p.SL + p.R * Dn;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < p.SL) { p.all[i] = p.seq[i]; continue; }
    const int64_t q = i - p.SL, r = q / Dn;
    const int t = (int)(q % Dn);
    const int32_t id = (int32_t)(p.num_item + (int64_t)t * p.K + p.paths[r * p.D + t]);
    for (int d = t + 1; d < p.D; d++) p.idx[d][r * d + t] = id;
  }
}

template <typename T>
struct DrtgSoftmaxParams { T *H; T *Zn; const int32_t *paths; int64_t S, R; int J, K, D; double *partial; };
// One wave per (sample, layer = blockIdx.y), the sample's J rows in j order.  H [S x DK]: in, the logits' history part; out (GRAD), Gs.
// Zn [R x (D-1)K]: in, the node part of Z_d, d >= 1; out (GRAD), G_d.  K <= 1024: a row, H's row and the running Gs live in registers;
// longer rows are read again, and Gs is then the sum of the G rows just written, read back in j order.
// partial[d * gridDim.x + blockIdx.x] = the workgroup's sum of -log P[r, path[r][d]] (a wave adds its rows in order, the four waves in
// wave order).  GRAD = false (dm_dr_layer_loss) writes nothing but the partials.
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void drtg_softmax_ce_kernel(DrtgSoftmaxParams<T> p) {
  __shared__ double wl[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = blockIdx.y, K = p.K, J = p.J, D = p.D;
  const int64_t NK = (int64_t)(D - 1) * K;
  const T fR = (T)p.R, fJ = (T)J;
  double lsum = 0;
  for (int64_t smp = (int64_t)blockIdx.x * 4 + wave; smp < p.S; smp += (int64_t)gridDim.x * 4) {
    T *h = p.H + smp * ((int64_t)D * K) + (int64_t)d * K;
    const int32_t *pa = p.paths + smp * J * D + d;                // pa[j D]: the target of row sJ + j
    T *zn = d ? p.Zn + smp * J * NK + (int64_t)(d - 1) * K : nullptr;      // zn + j NK: row sJ + j
    if (K <= 1024) {
      T hv[16], acc[16];
#pragma unroll
      for (int i = 0; i < 16; i++) { const int k = lane + 64 * i; hv[i] = k < K ? h[k] : (T)-INFINITY; acc[i] = 0; }
      if (d == 0) {                                               // one softmax for the J rows
        T m = -INFINITY, s = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) m = hv[i] > m ? hv[i] : m;
        m = dr_wave_max<T>(m);
#pragma unroll
        for (int i = 0; i < 16; i++) { hv[i] = DrKey<T>::ex(hv[i] - m); s += hv[i]; }
        s = dr_wave_sum<T>(s);
        const T lse = m + DrTol<T>::lg(s);
        for (int j = 0; j < J; j++) {
          const int tgt = pa[(int64_t)j * D];
          lsum += (double)(lse - h[tgt]);
#pragma unroll
          for (int i = 0; i < 16; i++) acc[i] += (lane + 64 * i == tgt ? (T)1 : (T)0);
        }
        if (GRAD) {
#pragma unroll
          for (int i = 0; i < 16; i++) { const int k = lane + 64 * i; if (k < K) h[k] = (fJ * (hv[i] / s) - acc[i]) / fR; }
        }
      } else {
        for (int j = 0; j < J; j++) {
          T *z = zn + (int64_t)j * NK;
          const int tgt = pa[(int64_t)j * D];
          const T zt = h[tgt] + z[tgt];
          T v[16], m = -INFINITY, s = 0;
#pragma unroll
          for (int i = 0; i < 16; i++) { const int k = lane + 64 * i; v[i] = k < K ? hv[i] + z[k] : (T)-INFINITY; m = v[i] > m ? v[i] : m; }
          m = dr_wave_max<T>(m);
#pragma unroll
          for (int i = 0; i < 16; i++) { v[i] = DrKey<T>::ex(v[i] - m); s += v[i]; }
          s = dr_wave_sum<T>(s);
          if (GRAD) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
              const int k = lane + 64 * i;
              const T g = (v[i] / s - (k == tgt ? (T)1 : (T)0)) / fR;
              if (k < K) { z[k] = g; acc[i] += g; }
            }
          }
          lsum += (double)((m + DrTol<T>::lg(s)) - zt);
        }
        if (GRAD) {
#pragma unroll
          for (int i = 0; i < 16; i++) { const int k = lane + 64 * i; if (k < K) h[k] = acc[i]; }
        }
      }
    } else if (d == 0) {
      T m = -INFINITY, s = 0;
      for (int k = lane; k < K; k += 64) { const T x = h[k]; m = x > m ? x : m; }
      m = dr_wave_max<T>(m);
      for (int k = lane; k < K; k += 64) s += DrKey<T>::ex(h[k] - m);
      s = dr_wave_sum<T>(s);
      const T lse = m + DrTol<T>::lg(s);
      for (int j = 0; j < J; j++) lsum += (double)(lse - h[pa[(int64_t)j * D]]);
      if (GRAD)
        for (int k = lane; k < K; k += 64) {
          T cnt = 0;
          for (int j = 0; j < J; j++) cnt += (pa[(int64_t)j * D] == k ? (T)1 : (T)0);
          h[k] = (fJ * (DrKey<T>::ex(h[k] - m) / s) - cnt) / fR;
        }
    } else {
      for (int j = 0; j < J; j++) {
        T *z = zn + (int64_t)j * NK;
        const int tgt = pa[(int64_t)j * D];
        const T zt = h[tgt] + z[tgt];
        T m = -INFINITY, s = 0;
        for (int k = lane; k < K; k += 64) { const T x = h[k] + z[k]; m = x > m ? x : m; }
        m = dr_wave_max<T>(m);
        for (int k = lane; k < K; k += 64) s += DrKey<T>::ex((h[k] + z[k]) - m);
        s = dr_wave_sum<T>(s);
        if (GRAD)
          for (int k = lane; k < K; k += 64) z[k] = (DrKey<T>::ex((h[k] + z[k]) - m) / s - (k == tgt ? (T)1 : (T)0)) / fR;
        lsum += (double)((m + DrTol<T>::lg(s)) - zt);
      }
      if (GRAD)
        for (int k = lane; k < K; k += 64) {                      // (a lane reads back what it wrote itself)
          T a = 0;
          for (int j = 0; j < J; j++) a += zn[(int64_t)j * NK + k];
          h[k] = a;
        }
    }
  }
  if (lane == 0) wl[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[(int64_t)d * gridDim.x + blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

// ---------------------------------------------------------------------------------------------------------------- host
static int drtg_check_shape(dm_ctx *h, const char *who, int64_t S, int64_t J, const void *a, const void *b, bool slots) {
  const dm_dr_state *s = h->dr;
  if (S <= 0 || J <= 0 || !a || !b) return fail(h, DM_ERR_INVALID, std::string(who) + ": S and J must be positive and the arrays non-null");
  // the row tiles of the products are a grid's y (64 rows each); the S L + R (D - 1) slots are sorted with 32-bit values
  if (S > (int64_t)DRT_MAX_ROWS || J > (int64_t)DRT_MAX_ROWS || S * J > (int64_t)DRT_MAX_ROWS)
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": batch too large (at most 4 194 240 rows S J): split it and accumulate on the host");
  if (slots && S * s->L + S * J * (s->D - 1) >= ((int64_t)1 << 31))
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": batch too large (S L + S J (D - 1) must stay below 2^31): split it and accumulate on the host");
  return DM_OK;
}
static int drtg_check_nodes(dm_ctx *h, const char *who, const int32_t *paths, int64_t n) {
  const int K = h->dr->K;
  for (int64_t i = 0; i < n; i++)
    if (paths[i] < 0 || paths[i] >= K) return fail(h, DM_ERR_INDEX, std::string(who) + ": path node outside [0, num_node)");
  return DM_OK;
}

// The grouped forward and the softmax / cross-entropy: H (GRAD: Gs afterwards) and Zn (GRAD: G_d, d >= 1), the per-layer loss SUMS over
// the R rows at d_loss [D].  idxn[d], 1 <= d < D: [R x d] node rows (drtg_build_idx_kernel).  d_lp: D nb doubles, nb = drtg_loss_blocks(S).
static int drtg_loss_blocks(int64_t S) { return (int)std::min<int64_t>((S + 3) / 4, 1024); }      // a function of S alone
template <typename T, bool GRAD>
static int drtg_forward(dm_ctx *h, const int32_t *d_seq, const int32_t *d_paths, int32_t *const *idxn, int64_t S, int J, T *H, T *Zn, double *d_lp,
                        double *d_loss, bool detail) {
  dm_dr_state *s = h->dr;
  const int K = s->K, D = s->D, L = s->L, E = s->E;
  const int64_t DK = (int64_t)D * K, R = S * J;
  int rc;
  if (s->wseq_stale && (rc = dr_refresh_wseq<T>(h, s)) != DM_OK) return rc;
  for (int d = 0; d < D; d++)               // d_sbias is dr_derive's and stale while training: the D bias blocks, every call
    HIPCHK(h, hipMemcpyAsync((char *)s->d_sbias + (size_t)d * K * sizeof(T), s->d_b[d], (size_t)K * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
  {
    DrGemmParams<T> g{};
    g.A = (const T *)s->d_layer_emb; g.lda = 0; g.gidx = d_seq; g.Lg = L; g.E = E;
    g.B = (const T *)s->d_wseq; g.ldb = (int64_t)L * E; g.bias = (const T *)s->d_sbias; g.zero = (const T *)s->d_zero;
    g.C = H; g.ldc = DK; g.M = S; g.N = (int)DK; g.Kd = L * E;
    dim3 grid((unsigned)((g.N + DR_TN - 1) / DR_TN), (unsigned)((g.M + DR_TM - 1) / DR_TM));
    if ((rc = timed(h, EV_DRT_FWD, detail, [&] { return LAUNCH(h, dr_gemm_kernel<T>, grid, dim3(256), 0, g); })) != DM_OK) return rc;
  }
  for (int d = 1; d < D; d++) {
    DrGemmParams<T> g{};
    g.A = (const T *)s->d_layer_emb; g.lda = 0; g.gidx = idxn[d]; g.Lg = d; g.E = E;
    g.B = (const T *)s->d_w[d] + (int64_t)L * E; g.ldb = (int64_t)(L + d) * E; g.bias = nullptr; g.zero = (const T *)s->d_zero;
    g.C = Zn + (int64_t)(d - 1) * K; g.ldc = (int64_t)(D - 1) * K; g.M = R; g.N = K; g.Kd = d * E;
    dim3 grid((unsigned)((g.N + DR_TN - 1) / DR_TN), (unsigned)((g.M + DR_TM - 1) / DR_TM));
    if ((rc = timed(h, EV_DRT_FWD, detail, [&] { return LAUNCH(h, dr_gemm_kernel<T>, grid, dim3(256), 0, g); })) != DM_OK) return rc;
  }
  DrtgSoftmaxParams<T> sp{};
  sp.H = H; sp.Zn = Zn; sp.paths = d_paths; sp.S = S; sp.R = R; sp.J = J; sp.K = K; sp.D = D; sp.partial = d_lp;
  const int nb = drtg_loss_blocks(S);
  return timed(h, EV_DRT_SOFTMAX, detail, [&] {
    const int r = LAUNCH(h, (drtg_softmax_ce_kernel<T, GRAD>), dim3((unsigned)nb, (unsigned)D), dim3(256), 0, sp);
    return r != DM_OK ? r : LAUNCH(h, drt_loss_sum_kernel, dim3(1), dim3(64), 0, (const double *)d_lp, nb, D, (int64_t)1, d_loss);      // B = 1: the sums
  });
}

static void drtg_idx_params(DrtgIdxParams &ip, const dm_dr_state *s, const int32_t *d_seq, const int32_t *d_paths, int64_t S, int J, int32_t *all,
                            int32_t *const *idxn) {
  ip.seq = d_seq; ip.paths = d_paths; ip.SL = S * s->L; ip.R = S * J; ip.D = s->D; ip.K = s->K; ip.num_item = s->num_item; ip.all = all;
  for (int d = 1; d < s->D; d++) ip.idx[d] = idxn[d];
}

template <typename T>
static int dr_train_fb_grouped_dev_t(dm_ctx *h, const int32_t *d_seq, const int32_t *d_paths, int64_t S, int J, double *out_loss) {
  dm_dr_state *s = h->dr;
  dm_dr_train *t = s->tr;
  const int K = s->K, D = s->D, L = s->L, E = s->E, Dn = D - 1;
  const int64_t NR = s->num_item + (int64_t)K * Dn, DK = (int64_t)D * K, NK = (int64_t)Dn * K, R = S * J, SL = S * L, m = SL + R * Dn;
  const bool detail = dr_time_launches();
  const int64_t slabs_s = (S + DRT_SLAB - 1) / DRT_SLAB, slabs_r = (R + DRT_SLAB - 1) / DRT_SLAB;
  const int nb = drtg_loss_blocks(S);
  int rc;
  // ---- the step's buffers
  DevArena ar(t->ws, 8);
  const size_t o_h = ar.add((size_t)S * DK * sizeof(T)), o_zn = ar.add((size_t)R * NK * sizeof(T)), o_dx = ar.add((size_t)m * E * sizeof(T));
  const size_t o_all = ar.add((size_t)m * 4);
  size_t o_idx[DR_MAXD] = {};
  for (int d = 1; d < Dn; d++) o_idx[d] = ar.add((size_t)R * d * 4);
  const size_t o_k0 = ar.add((size_t)m * 8), o_k1 = ar.add((size_t)m * 8), o_v0 = ar.add((size_t)m * 4), o_v1 = ar.add((size_t)m * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_part = ar.add(std::max((size_t)slabs_s * K * ((size_t)L * E + 1), (size_t)slabs_r * K * ((size_t)Dn * E + 1)) * sizeof(T));
  const size_t o_lp = ar.add((size_t)D * nb * 8), o_loss = ar.add((size_t)D * 8);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  T *H = ar.ptr<T>(o_h), *Zn = ar.ptr<T>(o_zn), *dX = ar.ptr<T>(o_dx), *part = ar.ptr<T>(o_part);
  T *dXn = dX + SL * E;
  T *grad = (T *)t->vec.grad;
  int32_t *all = ar.ptr<int32_t>(o_all), *idxn[DR_MAXD] = {};
  for (int d = 1; d < Dn; d++) idxn[d] = ar.ptr<int32_t>(o_idx[d]);
  if (Dn >= 1) idxn[Dn] = all + SL;
  // ---- zeroGradParameters: the rows the last batch reached, as the row step clears them (the dense blocks are overwritten below)
  t->exchanged = false;
  if (t->vec.prev_m > 0) {
    if ((rc = LAUNCH(h, (drt_seg_rows_kernel<T, true>), dim3(drt_blocks(h, t->vec.prev_m, 4)), dim3(256), 0, (const unsigned long long *)t->vec.prev.p, nullptr,
                     t->vec.prev_m, NR, nullptr, E, grad)) != DM_OK) return rc;
    t->vec.forget();
  }
  // ---- inputs, forward, softmax + cross-entropy: H -> Gs, Zn -> G_d
  DrtgIdxParams ip{};
  drtg_idx_params(ip, s, d_seq, d_paths, S, J, all, idxn);
  if ((rc = LAUNCH(h, drtg_build_idx_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, ip)) != DM_OK) return rc;
  if ((rc = drtg_forward<T, true>(h, d_seq, d_paths, idxn, S, J, H, Zn, ar.ptr<double>(o_lp), ar.ptr<double>(o_loss), detail)) != DM_OK) return rc;
  // ---- dX: the history slots from Gs in one product, the node slots layer by layer (the last layer writes, the others add)
  {
    DrtGemmParams<T> g{};
    g.A = H; g.a_rs = DK; g.a_cs = 1;
    g.B = (const T *)s->d_wseq; g.b_rs = 1; g.b_cs = (int64_t)L * E;
    g.C = dX; g.ldc = (int64_t)L * E; g.M = S; g.N = L * E; g.Kd = DK; g.slab = DK;
    if ((rc = drt_launch_gemm<T>(h, g, EV_DRT_DX, detail)) != DM_OK) return rc;
    for (int d = Dn; d >= 1; d--) {
      DrtGemmParams<T> q{};
      q.A = Zn + (int64_t)(d - 1) * K; q.a_rs = NK; q.a_cs = 1;
      q.B = (const T *)s->d_w[d] + (int64_t)L * E; q.b_rs = 1; q.b_cs = (int64_t)(L + d) * E;
      q.C = dXn; q.ldc = (int64_t)Dn * E; q.M = R; q.N = d * E; q.Kd = K; q.slab = K;
      q.accumulate = d != Dn;
      if ((rc = drt_launch_gemm<T>(h, q, EV_DRT_DX, detail)) != DM_OK) return rc;
    }
  }
  // ---- dW_d, db_d: history columns and the bias over the S samples, node columns over the R rows; slabs added in slab order
  {
    int64_t off = NR * E;
    for (int d = 0; d < D; d++) {
      const int cols = (L + d) * E, hc = L * E, nc = d * E;
      DrtGemmParams<T> g{};
      g.A = H + (int64_t)d * K; g.a_rs = 1; g.a_cs = DK;
      g.B = (const T *)s->d_layer_emb; g.gidx = d_seq; g.Lg = L; g.E = E; g.gcols = hc;
      g.C = part; g.ldc = hc + 1; g.c_slab = (int64_t)K * (hc + 1); g.M = K; g.N = hc + 1; g.Kd = S; g.slab = DRT_SLAB;
      if ((rc = drt_launch_gemm<T>(h, g, EV_DRT_DW, detail)) != DM_OK) return rc;
      rc = timed(h, EV_DRT_DW, detail, [&] {
        return LAUNCH(h, drt_slab_sum_kernel<T>, dim3(drt_blocks(h, (int64_t)K * (hc + 1), 256)), dim3(256), 0, (const T *)part, (int)slabs_s, K, hc, grad + off,
                      grad + off + (int64_t)K * cols, (int64_t)cols);
      });
      if (rc != DM_OK) return rc;
      if (d >= 1) {                           // (the column of ones behind Xn_d would give db_d a second time: summed and dropped)
        DrtGemmParams<T> q{};
        q.A = Zn + (int64_t)(d - 1) * K; q.a_rs = 1; q.a_cs = NK;
        q.B = (const T *)s->d_layer_emb; q.gidx = idxn[d]; q.Lg = d; q.E = E; q.gcols = nc;
        q.C = part; q.ldc = nc + 1; q.c_slab = (int64_t)K * (nc + 1); q.M = K; q.N = nc + 1; q.Kd = R; q.slab = DRT_SLAB;
        if ((rc = drt_launch_gemm<T>(h, q, EV_DRT_DW, detail)) != DM_OK) return rc;
        rc = timed(h, EV_DRT_DW, detail, [&] {
          return LAUNCH(h, drt_slab_sum_kernel<T>, dim3(drt_blocks(h, (int64_t)K * (nc + 1), 256)), dim3(256), 0, (const T *)part, (int)slabs_r, K, nc,
                        grad + off + hc, (T *)nullptr, (int64_t)cols);
        });
        if (rc != DM_OK) return rc;
      }
      off += (int64_t)K * cols + K;
    }
  }
  // ---- embedding gradient: one sort over the history slots followed by the node slots, one wave per destination
  rc = timed(h, EV_DRT_EMB, detail, [&]() -> int {
    const DrtSortBufs sb{ar.ptr<unsigned long long>(o_k0), ar.ptr<unsigned long long>(o_k1), ar.ptr<int32_t>(o_v0), ar.ptr<int32_t>(o_v1), ar.ptr<uint32_t>(o_tmp)};
    const unsigned long long *ks;
    const int32_t *vs;
    if ((rc = drt_sort_slots(h, all, m, NR, sb, ks, vs)) != DM_OK) return rc;
    if ((rc = LAUNCH(h, (drt_seg_rows_kernel<T, false>), dim3(drt_blocks(h, m, 4)), dim3(256), 0, ks, vs, m, NR, (const T *)dX, E, grad)) != DM_OK) return rc;
    if ((rc = t->vec.remember(h, ks, m)) != DM_OK) return rc;
    return t->vec.mark_active(h, drt_blocks(h, m, 256), all, m);
  });
  if (rc != DM_OK) return rc;
  double sums[DR_MAXD] = {};
  HIPCHK(h, hipMemcpyAsync(sums, ar.ptr<double>(o_loss), (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (out_loss)
    for (int d = 0; d < D; d++) out_loss[d] = sums[d] / (double)R;
  return DM_OK;
}

int dm_dr_train_forward_backward_grouped_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_paths, int64_t S, int64_t J, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_forward_backward_grouped");
  int rc = dr_train_check(h, "dm_dr_train_forward_backward_grouped", true);
  if (rc != DM_OK) return rc;
  if ((rc = drtg_check_shape(h, "dm_dr_train_forward_backward_grouped", S, J, d_seq_ids, d_paths, true)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return h->dr->dtype == DM_F32 ? dr_train_fb_grouped_dev_t<float>(h, d_seq_ids, d_paths, S, (int)J, out_loss)
                                : dr_train_fb_grouped_dev_t<double>(h, d_seq_ids, d_paths, S, (int)J, out_loss);
}

int dm_dr_train_forward_backward_grouped(dm_handle_t h, const int32_t *seq_ids, const int32_t *paths, int64_t S, int64_t J, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_forward_backward_grouped");
  int rc = dr_train_check(h, "dm_dr_train_forward_backward_grouped", true);
  if (rc != DM_OK) return rc;
  if ((rc = drtg_check_shape(h, "dm_dr_train_forward_backward_grouped", S, J, seq_ids, paths, true)) != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, S * s->L)) != DM_OK) return rc;
  if ((rc = drtg_check_nodes(h, "dm_dr_train_forward_backward_grouped", paths, S * J * s->D)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n_seq = (size_t)S * s->L * 4, n_paths = (size_t)S * J * s->D * 4, b_seq = DevArena::up(n_seq);
  if ((rc = s->tr->io.reserve(h, b_seq + DevArena::up(n_paths))) != DM_OK) return rc;
  int32_t *d_seq = (int32_t *)s->tr->io.p, *d_pa = (int32_t *)((char *)s->tr->io.p + b_seq);
  HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids, n_seq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_pa, paths, n_paths, hipMemcpyHostToDevice, h->stream));
  return dm_dr_train_forward_backward_grouped_dev(h, d_seq, d_pa, S, J, out_loss);
}

// Evaluator.evaluateLayerModel: the grouped forward and cross-entropy alone, in chunks of samples whose activations (H and Zn) stay under
// 256 MB (DM_DR_LAYER_LOSS_ROWS in the environment forces a chunk size in samples); the chunks' loss sums are added in chunk order.
// Every array is a temporary of the call: nothing of the training state is read or written, and none is needed.
template <typename T>
static int dr_layer_loss_t(dm_ctx *h, const int32_t *seq_ids, const int32_t *paths, int64_t S, int J, double *out) {
  dm_dr_state *s = h->dr;
  const int K = s->K, D = s->D, L = s->L, Dn = D - 1;
  const int64_t per = ((int64_t)D * K + (int64_t)J * Dn * K) * (int64_t)sizeof(T);
  int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / per);
  if (const long long v_ = env_int("DM_DR_LAYER_LOSS_ROWS")) chunk = v_;
  chunk = std::min(std::min(chunk, S), (int64_t)DRT_MAX_ROWS / J);
  const int64_t Rc = chunk * J, mc = chunk * L + Rc * Dn;
  const int nb = drtg_loss_blocks(chunk);
  DevTemps tmp(h);
  int32_t *d_seq = nullptr, *d_pa = nullptr, *all = nullptr, *idxn[DR_MAXD] = {};
  T *H = nullptr, *Zn = nullptr;
  double *lp = nullptr;
  int rc;
  if ((rc = tmp.alloc(d_seq, (size_t)chunk * L * 4)) != DM_OK || (rc = tmp.alloc(d_pa, (size_t)Rc * D * 4)) != DM_OK ||
      (rc = tmp.alloc(all, (size_t)mc * 4)) != DM_OK || (rc = tmp.alloc(H, (size_t)chunk * D * K * sizeof(T))) != DM_OK ||
      (rc = tmp.alloc(Zn, std::max<size_t>((size_t)Rc * Dn * K * sizeof(T), 256))) != DM_OK || (rc = tmp.alloc(lp, (size_t)(D * nb + D) * 8)) != DM_OK) return rc;
  for (int d = 1; d < Dn; d++)
    if ((rc = tmp.alloc(idxn[d], (size_t)Rc * d * 4)) != DM_OK) return rc;
  double total[DR_MAXD] = {};
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t n = std::min(chunk, S - s0);
    if (Dn >= 1) idxn[Dn] = all + n * L;
    HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids + s0 * L, (size_t)n * L * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_pa, paths + s0 * J * D, (size_t)n * J * D * 4, hipMemcpyHostToDevice, h->stream));
    DrtgIdxParams ip{};
    drtg_idx_params(ip, s, d_seq, d_pa, n, J, all, idxn);
    if ((rc = LAUNCH(h, drtg_build_idx_kernel, dim3(drt_blocks(h, n * L + n * J * Dn, 256)), dim3(256), 0, ip)) != DM_OK) return rc;
    if ((rc = drtg_forward<T, false>(h, d_seq, d_pa, idxn, n, J, H, Zn, lp, lp + (size_t)D * nb, false)) != DM_OK) return rc;
    double part[DR_MAXD] = {};
    HIPCHK(h, hipMemcpyAsync(part, lp + (size_t)D * nb, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int d = 0; d < D; d++) total[d] += part[d];
  }
  for (int d = 0; d < D; d++) out[d] = total[d] / (double)(S * J);
  return DM_OK;
}

int dm_dr_layer_loss(dm_handle_t h, const int32_t *seq_ids, const int32_t *paths, int64_t S, int64_t J, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_layer_loss");
  int rc = dr_train_check(h, "dm_dr_layer_loss", false);
  if (rc != DM_OK) return rc;
  if (S <= 0 || J <= 0 || !seq_ids || !paths || !out_loss) return fail(h, DM_ERR_INVALID, "dm_dr_layer_loss: S and J must be positive and the arguments non-null");
  // the samples are walked in chunks, so S is not bounded by a grid; one sample's J rows are
  if (J > (int64_t)DRT_MAX_ROWS) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_layer_loss: too many paths per sample (at most 4 194 240)");
  if (S > ((int64_t)1 << 62) / J / std::max(1, h->dr->D)) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_layer_loss: S J D overflows");
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, S * s->L)) != DM_OK) return rc;
  if ((rc = drtg_check_nodes(h, "dm_dr_layer_loss", paths, S * J * s->D)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return s->dtype == DM_F32 ? dr_layer_loss_t<float>(h, seq_ids, paths, S, (int)J, out_loss) : dr_layer_loss_t<double>(h, seq_ids, paths, S, (int)J, out_loss);
}
