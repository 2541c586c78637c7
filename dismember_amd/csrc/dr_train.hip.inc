// Deep-Retrieval E-step on the device: one training step of the LAYER model (dm_dr_train_*, dm_dr_adam_step; DESIGN.md §10).
// Reference: deep-retrieval/src/main/scala/com/mass/dr/ (D/) model/LayerModel.scala:22-49 (the graph: one shared embedding, per layer
// d a Linear((L+d)E -> K) over [history rows ; node rows of the path so far]), dataset/MiniBatch.scala:18-50 (transformLayerData: one
// row per (sample, path of the target item)), loss/CrossEntropyLayer.scala + scalann nn/{LogSoftMax,ClassNLLCriterion} (per layer the
// mean over the batch of -log softmax(z)[path_d]), optim/LocalOptimizer.scala:58-116, scalann optim/Adam.scala:19-73.
//
//   Z_d = X_d W_d^T + b_d          X_d[r] = [emb[seq[r][0..L)] ; emb[num_item + t K + path[r][t]], t < d],  id -1 = a zero row, no gradient
//   P_d = softmax rows;  loss_d = -(1/B) sum_r log P_d[r, path[r][d]];  G_d = (P_d - onehot(path[:, d])) / B
//   dW_d = G_d^T X_d;  db_d = sum_r G_d[r];  dX_d = G_d W_d;  demb[id] += the E-wide slices of dX_d that row id fed
//
// The gradient is the mean over the WHOLE batch.  The reference splits a batch over its threads and averages the per-thread means
// (LocalOptimizer.scala:135-194): the same value whenever the thread count divides B, and the reading taken here.
//
// Kernels (T = float | double through DrMma<T>: v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64):
//   forward      dr_gemm_kernel<T>, rows gathered through a per-layer index array of Lg = L + d ids; all Z_d side by side in one [B x DK] block
//   softmax/CE   drt_softmax_ce_kernel: one wave per row, one read of the row (K <= 1024: in registers), row maximum, G_d written in place,
//                loss partials per workgroup, summed in workgroup order by drt_loss_sum_kernel
//   dX           history part of every layer in ONE product [B x DK] . [DK x LE] over d_wseq; the node parts of layer d (its d products
//                [B x K] . [K x E], adjacent in W_d) as one product per layer, added layer by layer into the node slots
//   dW_d, db_d   drt_gemm_kernel reduces over the batch in slabs of DRT_SLAB rows (a column of ones behind X_d gives db_d), drt_slab_sum_kernel
//                adds the slabs in slab order
//   demb         no floating-point atomics: (destination row, source slot) pairs, stable dev_radix_sort_pairs by destination, one wave per
//                destination adds its slots in sorted (= batch) order.  K (D-1) node rows receive B (D-1) contributions: with atomics those
//                would serialise on a few thousand addresses AND arrive in a different order every run
// Every sum has a fixed order: the same state and batch give the same bytes (the M-step is a discontinuous function of the model).

struct dm_dr_train {
  TrainVec vec;              // over d_par: [layer_emb ; W_0 ; b_0 ; ...], rows = the embedding table's
  DevGrow ws, io;
  DevGrow sync;                              // staging of dm_dr_train_sync_gradients (dr_train_sync.hip.inc): all ranks' blocks, their tails
  bool exchanged = false;                    // vec.grad holds the sum over ranks: until the next forward/backward or Adam step
};

static void dr_train_release(dm_dr_state *s) {
  dm_dr_train *t = s->tr;
  if (!t) return;
  t->vec.release();
  for (DevGrow *g : {&t->ws, &t->io, &t->sync}) g->release();
  delete t;
  s->tr = nullptr;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
struct DrtIdxParams { const int32_t *seq, *paths; int64_t B; int L, D, K; int64_t num_item; int32_t *idx[DR_MAXD]; };
// idx[d][r][j], j < L + d: the embedding row that feeds position j of layer d's input (-1: padding)
__global__ void drt_build_idx_kernel(DrtIdxParams p) {
  const int W = p.L + p.D - 1;
  const int64_t n = p.B * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / W;
    const int j = (int)(i % W);
    const int32_t id = j < p.L ? p.seq[r * p.L + j] : (int32_t)(p.num_item + (int64_t)(j - p.L) * p.K + p.paths[r * p.D + (j - p.L)]);
    for (int d = j < p.L ? 0 : j - p.L + 1; d < p.D; d++) p.idx[d][r * (p.L + d) + j] = id;
  }
}

template <typename T>
struct DrtSoftmaxParams { T *Z; const int32_t *paths; int64_t B; int K, D; double *partial; };
// rows of Z_d (columns [dK, (d+1)K) of the [B x DK] block) -> G_d in place; blockIdx.y = d; partial[d * gridDim.x + blockIdx.x] = the
// workgroup's sum of -log P[r, path[r][d]] (each wave adds its rows in row order, the four waves are added in wave order)
template <typename T>
__global__ __launch_bounds__(256) void drt_softmax_ce_kernel(DrtSoftmaxParams<T> p) {
  __shared__ double wl[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = blockIdx.y, K = p.K;
  const T fB = (T)p.B;
  double lsum = 0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < p.B; row += (int64_t)gridDim.x * 4) {
    T *z = p.Z + row * ((int64_t)p.D * K) + (int64_t)d * K;
    const int tgt = p.paths[row * p.D + d];
    const T zt = z[tgt];
    T m = -INFINITY, s = 0;
    if (K <= 1024) {                                   // the row lives in registers between its one read and its one write
      T v[16];
#pragma unroll
      for (int j = 0; j < 16; j++) { const int k = lane + 64 * j; v[j] = k < K ? z[k] : (T)-INFINITY; m = v[j] > m ? v[j] : m; }
      m = dr_wave_max<T>(m);
#pragma unroll
      for (int j = 0; j < 16; j++) { v[j] = DrKey<T>::ex(v[j] - m); s += v[j]; }       // exp(-inf) = 0 past the row's end
      s = dr_wave_sum<T>(s);
#pragma unroll
      for (int j = 0; j < 16; j++) { const int k = lane + 64 * j; if (k < K) z[k] = (v[j] / s - (k == tgt ? (T)1 : (T)0)) / fB; }
    } else {
      for (int k = lane; k < K; k += 64) { const T x = z[k]; m = x > m ? x : m; }
      m = dr_wave_max<T>(m);
      for (int k = lane; k < K; k += 64) s += DrKey<T>::ex(z[k] - m);
      s = dr_wave_sum<T>(s);
      for (int k = lane; k < K; k += 64) z[k] = (DrKey<T>::ex(z[k] - m) / s - (k == tgt ? (T)1 : (T)0)) / fB;
    }
    lsum += (double)((m + DrTol<T>::lg(s)) - zt);
  }
  if (lane == 0) wl[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[(int64_t)d * gridDim.x + blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}
__global__ void drt_loss_sum_kernel(const double *partial, int nb, int D, int64_t B, double *out) {
  const int d = threadIdx.x;
  if (d >= D) return;
  double s = 0;
  for (int i = 0; i < nb; i++) s += partial[(int64_t)d * nb + i];
  out[d] = s / (double)B;
}

// C[m][n] (+)= sum over c in this slab of A(m, c) B(n, c), 64 x 64 per workgroup (4 waves of 32 x 32), k step 16, MFMA 16x16x4.
//   A(m, c) = A[m a_rs + c a_cs];  B(n, c) = B[n b_rs + c b_cs], n is the fast index of B in every use here;
//   gather mode (gidx): B(n, c) = element n % E of table row gidx[c Lg + n / E] (a zero row for id -1) for n < gcols, 1 at n == gcols.
// blockIdx.z = slab: c in [z slab, min(Kd, (z+1) slab)), written to C + z c_slab.  Every load is bounds-checked (no operand is padded).
template <typename T>
struct DrtGemmParams {
  const T *A; int64_t a_rs, a_cs;
  const T *B; int64_t b_rs, b_cs;
  const int32_t *gidx; int Lg, E, gcols;
  T *C; int64_t ldc, c_slab;
  int64_t M; int N;
  int64_t Kd, slab;
  int accumulate;
};
#define DRT_T 64
#define DRT_K 16
#define DRT_LDP (64 + 16)   // row stride = 16 (mod 64) words, as DR_LDP
#define DRT_SLAB 512
#define DRT_MAX_ROWS (65535 * DRT_T)      // a grid's y and z are at most 65 535: B / 64 row tiles (dX), B / 128 (forward), B / 512 slabs (dW)
template <typename T>
__global__ __launch_bounds__(256) void drt_gemm_kernel(DrtGemmParams<T> p) {
  typedef typename DrMma<T>::acc_t acc_t;
  __shared__ T As[DRT_K][DRT_LDP];
  __shared__ T Bs[DRT_K][DRT_LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.y * DRT_T;
  const int n0 = blockIdx.x * DRT_T;
  const int64_t c_lo = (int64_t)blockIdx.z * p.slab, c_hi = c_lo + p.slab < p.Kd ? c_lo + p.slab : p.Kd;
  acc_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (acc_t){0, 0, 0, 0};
  const bool a_mfast = p.a_rs == 1;            // which index of A is contiguous: the four elements a thread stages run along it
  T av[4], bv[4];
  auto load_tile = [&](int64_t c0) {
    if (a_mfast) {
      const int64_t c = c0 + (tid >> 4), mb = m0 + (tid & 15) * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) av[e] = (c < c_hi && mb + e < p.M) ? p.A[(mb + e) + c * p.a_cs] : (T)0;
    } else {
      const int64_t m = m0 + (tid >> 2), cb = c0 + (tid & 3) * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) av[e] = (m < p.M && cb + e < c_hi) ? p.A[m * p.a_rs + (cb + e) * p.a_cs] : (T)0;
    }
    const int64_t c = c0 + (tid >> 4);
    const int nb = n0 + (tid & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; e++) bv[e] = (T)0;
    if (c < c_hi) {
      if (p.gidx) {                                 // (nb % 4 == 0 and gcols % 16 == 0: the four columns share a table row, or start at gcols)
        if (nb < p.gcols) {
          const int32_t id = p.gidx[c * p.Lg + nb / p.E];
          if (id >= 0) {
            const T *src = p.B + (int64_t)id * p.E + nb % p.E;
#pragma unroll
            for (int e = 0; e < 4; e++) bv[e] = src[e];
          }
        } else if (nb == p.gcols) bv[0] = (T)1;
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) if (nb + e < p.N) bv[e] = p.B[(int64_t)(nb + e) * p.b_rs + c * p.b_cs];
      }
    }
  };
  auto store_tile = [&]() {
    if (a_mfast) {
#pragma unroll
      for (int e = 0; e < 4; e++) As[tid >> 4][(tid & 15) * 4 + e] = av[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) As[(tid & 3) * 4 + e][tid >> 2] = av[e];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) Bs[tid >> 4][(tid & 15) * 4 + e] = bv[e];
  };
  if (c_lo < c_hi) load_tile(c_lo);
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += DRT_K) {
    store_tile();
    __syncthreads();
    if (c0 + DRT_K < c_hi) load_tile(c0 + DRT_K);      // next tile's loads fly under this tile's MFMAs
#pragma unroll
    for (int kk = 0; kk < DRT_K / 4; kk++) {
      T a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) a[i] = As[4 * kk + (lane >> 4)][wm * 32 + 16 * i + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; j++) b[j] = Bs[4 * kk + (lane >> 4)][wn * 32 + 16 * j + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = DrMma<T>::mma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  T *C = p.C + (int64_t)blockIdx.z * p.c_slab;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int n = n0 + wn * 32 + 16 * j + (lane & 15);
      if (n >= p.N) continue;
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int64_t m = m0 + wm * 32 + 16 * i + DrMma<T>::row(lane, rr);
        if (m >= p.M) continue;
        T *dst = C + m * p.ldc + n;
        *dst = p.accumulate ? *dst + acc[i][j][rr] : acc[i][j][rr];
      }
    }
}

// slabs [S][K][cols + 1] -> dW [K][cols] (row stride ldw: a column range of a wider matrix) and db [K] (or NULL: dropped), slab 0 first
template <typename T>
__global__ void drt_slab_sum_kernel(const T *part, int S, int K, int cols, T *gw, T *gb, int64_t ldw) {
  const int64_t n = (int64_t)K * (cols + 1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T s = part[i];
    for (int z = 1; z < S; z++) s += part[(int64_t)z * n + i];
    const int64_t k = i / (cols + 1);
    const int c = (int)(i % (cols + 1));
    if (c < cols) gw[k * ldw + c] = s; else if (gb) gb[k] = s;
  }
}

// slot i of the [B x (L+D-1)] input positions -> (destination row | NR for padding, i)
__global__ void drt_pairs_kernel(const int32_t *idx, int64_t m, int64_t NR, unsigned long long *keys, int32_t *vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t id = idx[i];
    keys[i] = id >= 0 ? (unsigned long long)id : (unsigned long long)NR;
    vals[i] = (int32_t)i;
  }
}
// the end of the segment of equal keys that starts at position i (all 64 lanes call it), 64 positions per look
__device__ __forceinline__ int64_t drt_segment_end(const unsigned long long *keys, int64_t i, int64_t m, unsigned long long key, int lane) {
  int64_t qe = i + 1;
  while (qe < m) {
    const bool differs = qe + lane >= m || keys[qe + lane] != key;
    const unsigned long long mask = __ballot(differs);
    if (mask) { qe += __builtin_ctzll(mask); break; }
    qe += 64;
  }
  return qe > m ? m : qe;
}
// one wave per sorted position; the wave at a destination's FIRST position owns the row.  zero: clear it; otherwise add the E-wide
// slices dX[slot] of its slots in sorted order (the sort is stable: ascending slot = batch order)
template <typename T, bool ZERO>
__global__ __launch_bounds__(256) void drt_seg_rows_kernel(const unsigned long long *keys, const int32_t *vals, int64_t m, int64_t NR,
                                                           const T *dX, int E, T *grad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < m; i += (int64_t)gridDim.x * 4) {
    const unsigned long long key = keys[i];
    if (key >= (unsigned long long)NR || (i > 0 && keys[i - 1] == key)) continue;
    T *dst = grad + (int64_t)key * E;
    if (ZERO) { for (int e = lane; e < E; e += 64) dst[e] = (T)0; continue; }
    const int64_t qe = drt_segment_end(keys, i, m, key, lane);
    for (int e = lane; e < E; e += 64) {
      T acc = 0;
      int64_t q = i;
      for (; q + 4 <= qe; q += 4) {                         // four loads in flight, added in order
        const T x0 = dX[(int64_t)vals[q] * E + e], x1 = dX[(int64_t)vals[q + 1] * E + e], x2 = dX[(int64_t)vals[q + 2] * E + e], x3 = dX[(int64_t)vals[q + 3] * E + e];
        acc += x0; acc += x1; acc += x2; acc += x3;
      }
      for (; q < qe; q++) acc += dX[(int64_t)vals[q] * E + e];
      dst[e] = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// (launch kinds under DM_DR_TIME_LAUNCHES=1: EV_DRT_* in host_request.hip.inc)
static int dr_train_check(dm_ctx *h, const char *who, bool need_init) {
  dm_dr_state *s = h->dr;
  if (!s || !s->loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": Deep-Retrieval model not loaded");
  if (need_init && !s->tr) return fail(h, DM_ERR_STATE, std::string(who) + ": call dm_dr_train_init first");
  return DM_OK;
}

int dm_dr_train_init(dm_handle_t h, const dm_adam_opts *o) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_init");
  int rc = dr_train_check(h, "dm_dr_train_init", false);
  if (rc != DM_OK) return rc;
  if (!o || !(o->lr > 0)) return fail(h, DM_ERR_INVALID, "dm_dr_train_init: bad optimizer options");
  HIPCHK(h, hipSetDevice(h->device));
  dm_dr_state *s = h->dr;
  dr_train_release(s);
  dm_dr_train *t = new dm_dr_train();
  s->tr = t;
  if ((rc = t->vec.init(h, s->num_item + (int64_t)s->K * (s->D - 1), s->E, s->n_par, s->dtype == DM_F64 ? 8 : 4, *o)) != DM_OK) {
    dr_train_release(s);
    return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_dr_train_free(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_free");
  if (!h->dr) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dr_train_release(h->dr);
  return DM_OK;
}

// grid of a grid-stride kernel: one workgroup per `per` elements, at most 16 per compute unit
static unsigned drt_blocks(dm_ctx *h, int64_t n, int per) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, (int64_t)h->n_cu * 16)); }

// "Scatter a batch's per-slot values into table rows in a fixed order", first half: slot i of ids[0..m) -> (destination row | NR for
// padding, i), sorted by destination (stable: ascending slot = batch order inside a destination).  ks / vs: where the sorted pairs are.
// The caller's segment kernel (one wave per destination) adds the slots' values; then TrainVec::remember and mark_active.
struct DrtSortBufs { unsigned long long *k0, *k1; int32_t *v0, *v1; uint32_t *tmp; };
static int drt_sort_slots(dm_ctx *h, const int32_t *ids, int64_t m, int64_t NR, const DrtSortBufs &b, const unsigned long long *&ks, const int32_t *&vs) {
  const int rc = LAUNCH(h, drt_pairs_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, ids, m, NR, b.k0, b.v0);
  if (rc != DM_OK) return rc;
  int bits = 1;
  while (((int64_t)1 << bits) <= NR) bits++;                // NR itself (padding) sorts last
  int where = 0;
  HIPCHK(h, dev_radix_sort_pairs(h->stream, b.k0, b.v0, b.k1, b.v1, m, 0, bits, b.tmp, &where));
  ks = where ? b.k1 : b.k0;
  vs = where ? b.v1 : b.v0;
  return DM_OK;
}

template <typename T>
static int drt_launch_gemm(dm_ctx *h, const DrtGemmParams<T> &p, int kind, bool on) {
  if (p.M <= 0 || p.N <= 0 || p.Kd <= 0) return DM_OK;
  const int64_t slabs = (p.Kd + p.slab - 1) / p.slab;
  dim3 grid((unsigned)((p.N + DRT_T - 1) / DRT_T), (unsigned)((p.M + DRT_T - 1) / DRT_T), (unsigned)slabs);
  return timed(h, kind, on, [&] { return LAUNCH(h, drt_gemm_kernel<T>, grid, dim3(256), 0, p); });
}

template <typename T>
static int dr_train_fb_dev_t(dm_ctx *h, const int32_t *d_seq, const int32_t *d_paths, int64_t B, double *out_loss) {
  dm_dr_state *s = h->dr;
  dm_dr_train *t = s->tr;
  const int K = s->K, D = s->D, L = s->L, E = s->E, W = L + D - 1;
  const int64_t NR = s->num_item + (int64_t)K * (D - 1), DK = (int64_t)D * K, m = B * W;
  // B (L + D - 1) slots are sorted with 32-bit values; the row tiles of the products are a grid's y (64 rows each: the smallest tile)
  if (m >= ((int64_t)1 << 31) || B > (int64_t)DRT_MAX_ROWS)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_train_forward_backward: batch too large (at most 4 194 240 rows, and B (L + D - 1) below 2^31): split it and accumulate on the host");
  const bool detail = dr_time_launches();
  const int64_t slabs = (B + DRT_SLAB - 1) / DRT_SLAB;
  const int nb = (int)std::min<int64_t>((B + 3) / 4, 1024);                  // loss partials per layer: a function of B alone
  int rc;
  // ---- the step's buffers
  DevArena ar(t->ws, 8);
  const size_t o_z = ar.add((size_t)B * DK * sizeof(T)), o_dx = ar.add((size_t)m * E * sizeof(T));
  size_t o_idx[DR_MAXD];
  for (int d = 0; d < D; d++) o_idx[d] = ar.add((size_t)B * (L + d) * 4);
  const size_t o_k0 = ar.add((size_t)m * 8), o_k1 = ar.add((size_t)m * 8), o_v0 = ar.add((size_t)m * 4), o_v1 = ar.add((size_t)m * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_part = ar.add((size_t)slabs * K * ((size_t)W * E + 1) * sizeof(T));
  const size_t o_lp = ar.add((size_t)D * nb * 8), o_loss = ar.add((size_t)D * 8);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  T *Z = ar.ptr<T>(o_z), *dX = ar.ptr<T>(o_dx), *part = ar.ptr<T>(o_part);
  T *grad = (T *)t->vec.grad;
  if (s->wseq_stale && (rc = dr_refresh_wseq<T>(h, s)) != DM_OK) return rc;
  // ---- zeroGradParameters: the rows the last batch reached (the dense blocks are overwritten below).  After a gradient exchange `prev`
  // is the concatenation of every rank's rows, sorted only inside a rank: the kernel clears at every change of key, so a row may be
  // cleared more than once, which changes nothing
  t->exchanged = false;
  if (t->vec.prev_m > 0) {
    if ((rc = LAUNCH(h, (drt_seg_rows_kernel<T, true>), dim3(drt_blocks(h, t->vec.prev_m, 4)), dim3(256), 0, (const unsigned long long *)t->vec.prev.p, nullptr,
                     t->vec.prev_m, NR, nullptr, E, grad)) != DM_OK) return rc;
    t->vec.forget();
  }
  // ---- inputs
  DrtIdxParams ip{};
  ip.seq = d_seq; ip.paths = d_paths; ip.B = B; ip.L = L; ip.D = D; ip.K = K; ip.num_item = s->num_item;
  for (int d = 0; d < D; d++) ip.idx[d] = ar.ptr<int32_t>(o_idx[d]);
  if ((rc = LAUNCH(h, drt_build_idx_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, ip)) != DM_OK) return rc;
  // ---- forward
  for (int d = 0; d < D; d++) {
    DrGemmParams<T> g{};
    g.A = (const T *)s->d_layer_emb; g.lda = 0; g.gidx = ip.idx[d]; g.Lg = L + d; g.E = E;
    g.B = (const T *)s->d_w[d]; g.ldb = (int64_t)(L + d) * E; g.bias = (const T *)s->d_b[d]; g.zero = (const T *)s->d_zero;
    g.C = Z + (int64_t)d * K; g.ldc = DK; g.M = B; g.N = K; g.Kd = (L + d) * E;
    dim3 grid((unsigned)((g.N + DR_TN - 1) / DR_TN), (unsigned)((g.M + DR_TM - 1) / DR_TM));
    if ((rc = timed(h, EV_DRT_FWD, detail, [&] { return LAUNCH(h, dr_gemm_kernel<T>, grid, dim3(256), 0, g); })) != DM_OK) return rc;
  }
  // ---- softmax + cross-entropy: Z_d -> G_d
  {
    DrtSoftmaxParams<T> sp{};
    sp.Z = Z; sp.paths = d_paths; sp.B = B; sp.K = K; sp.D = D; sp.partial = ar.ptr<double>(o_lp);
    rc = timed(h, EV_DRT_SOFTMAX, detail, [&] {
      const int r = LAUNCH(h, drt_softmax_ce_kernel<T>, dim3((unsigned)nb, (unsigned)D), dim3(256), 0, sp);
      return r != DM_OK ? r : LAUNCH(h, drt_loss_sum_kernel, dim3(1), dim3(64), 0, sp.partial, nb, D, B, ar.ptr<double>(o_loss));
    });
    if (rc != DM_OK) return rc;
  }
  // ---- dX: history columns of every layer in one product, then the node columns layer by layer (the last layer writes, the others add)
  {
    DrtGemmParams<T> g{};
    g.A = Z; g.a_rs = DK; g.a_cs = 1;
    g.B = (const T *)s->d_wseq; g.b_rs = 1; g.b_cs = (int64_t)L * E;
    g.C = dX; g.ldc = (int64_t)W * E; g.M = B; g.N = L * E; g.Kd = DK; g.slab = DK;
    if ((rc = drt_launch_gemm<T>(h, g, EV_DRT_DX, detail)) != DM_OK) return rc;
    for (int d = D - 1; d >= 1; d--) {
      DrtGemmParams<T> q{};
      q.A = Z + (int64_t)d * K; q.a_rs = DK; q.a_cs = 1;
      q.B = (const T *)s->d_w[d] + (int64_t)L * E; q.b_rs = 1; q.b_cs = (int64_t)(L + d) * E;
      q.C = dX + (int64_t)L * E; q.ldc = (int64_t)W * E; q.M = B; q.N = d * E; q.Kd = K; q.slab = K;
      q.accumulate = d != D - 1;
      if ((rc = drt_launch_gemm<T>(h, q, EV_DRT_DX, detail)) != DM_OK) return rc;
    }
  }
  // ---- dW_d, db_d: slabs of the batch, added in slab order
  {
    int64_t off = NR * E;
    for (int d = 0; d < D; d++) {
      const int cols = (L + d) * E;
      DrtGemmParams<T> g{};
      g.A = Z + (int64_t)d * K; g.a_rs = 1; g.a_cs = DK;
      g.B = (const T *)s->d_layer_emb; g.gidx = ip.idx[d]; g.Lg = L + d; g.E = E; g.gcols = cols;
      g.C = part; g.ldc = cols + 1; g.c_slab = (int64_t)K * (cols + 1); g.M = K; g.N = cols + 1; g.Kd = B; g.slab = DRT_SLAB;
      if ((rc = drt_launch_gemm<T>(h, g, EV_DRT_DW, detail)) != DM_OK) return rc;
      rc = timed(h, EV_DRT_DW, detail, [&] {
        return LAUNCH(h, drt_slab_sum_kernel<T>, dim3(drt_blocks(h, (int64_t)K * (cols + 1), 256)), dim3(256), 0, part, (int)slabs, K, cols, grad + off,
                      grad + off + (int64_t)K * cols, cols);
      });
      if (rc != DM_OK) return rc;
      off += (int64_t)K * cols + K;
    }
  }
  // ---- embedding gradient: sort the slots by destination row, one wave per destination
  rc = timed(h, EV_DRT_EMB, detail, [&]() -> int {
    const DrtSortBufs sb{ar.ptr<unsigned long long>(o_k0), ar.ptr<unsigned long long>(o_k1), ar.ptr<int32_t>(o_v0), ar.ptr<int32_t>(o_v1), ar.ptr<uint32_t>(o_tmp)};
    const int32_t *full = ip.idx[D - 1];                    // [B x (L+D-1)]: every input position of the batch
    const unsigned long long *ks;
    const int32_t *vs;
    if ((rc = drt_sort_slots(h, full, m, NR, sb, ks, vs)) != DM_OK) return rc;
    if ((rc = LAUNCH(h, (drt_seg_rows_kernel<T, false>), dim3(drt_blocks(h, m, 4)), dim3(256), 0, ks, vs, m, NR, dX, E, grad)) != DM_OK) return rc;
    if ((rc = t->vec.remember(h, ks, m)) != DM_OK) return rc;
    return t->vec.mark_active(h, drt_blocks(h, m, 256), full, m);
  });
  if (rc != DM_OK) return rc;
  if (out_loss) HIPCHK(h, hipMemcpyAsync(out_loss, ar.ptr<double>(o_loss), (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_dr_train_forward_backward_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_paths, int64_t B, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_forward_backward");
  int rc = dr_train_check(h, "dm_dr_train_forward_backward", true);
  if (rc != DM_OK) return rc;
  if (B <= 0 || !d_seq_ids || !d_paths) return fail(h, DM_ERR_INVALID, "dm_dr_train_forward_backward: B must be positive and the arrays non-null");
  HIPCHK(h, hipSetDevice(h->device));
  return h->dr->dtype == DM_F32 ? dr_train_fb_dev_t<float>(h, d_seq_ids, d_paths, B, out_loss) : dr_train_fb_dev_t<double>(h, d_seq_ids, d_paths, B, out_loss);
}

int dm_dr_train_forward_backward(dm_handle_t h, const int32_t *seq_ids, const int32_t *paths, int64_t B, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_forward_backward");
  int rc = dr_train_check(h, "dm_dr_train_forward_backward", true);
  if (rc != DM_OK) return rc;
  if (B <= 0 || !seq_ids || !paths) return fail(h, DM_ERR_INVALID, "dm_dr_train_forward_backward: B must be positive and the arrays non-null");
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, B * s->L)) != DM_OK) return rc;
  for (int64_t i = 0; i < B * s->D; i++)
    if (paths[i] < 0 || paths[i] >= s->K) return fail(h, DM_ERR_INDEX, "dm_dr_train_forward_backward: path node outside [0, num_node)");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t b_seq = DevArena::up((size_t)B * s->L * 4), b_paths = DevArena::up((size_t)B * s->D * 4);
  if ((rc = s->tr->io.reserve(h, b_seq + b_paths)) != DM_OK) return rc;
  int32_t *d_seq = (int32_t *)s->tr->io.p, *d_pa = (int32_t *)((char *)s->tr->io.p + b_seq);
  HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids, (size_t)B * s->L * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_pa, paths, (size_t)B * s->D * 4, hipMemcpyHostToDevice, h->stream));
  return dm_dr_train_forward_backward_dev(h, d_seq, d_pa, B, out_loss);
}

// Adam.optimize over [layer_emb ; W_0 ; b_0 ; ...] with dm_adam_step's kernels and rules: the embedding rows a gradient has ever reached
// and the dense blocks, or the whole vector when eps == 0, when a quarter of the rows is active, or under DM_ADAM_DENSE=1.
int dm_dr_adam_step(dm_handle_t h, float grad_scale) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_adam_step");
  int rc = dr_train_check(h, "dm_dr_adam_step", true);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_dr_state *s = h->dr;
  dm_dr_train *t = s->tr;
  unsigned long long act = 0;
  HIPCHK(h, hipMemcpyAsync(&act, t->vec.active_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const AdamPlan plan = t->vec.plan_step(act);
  s->derived_stale = true; s->wseq_stale = true;      // before the first launch: a step that fails half-way has still moved weights
  t->exchanged = false;
  rc = timed(h, EV_DRT_ADAM, dr_time_launches(), [&] { return adam_step(h, t->vec, plan, s->d_par, s->dtype == DM_F64, false, grad_scale, false, 1024); });
  if (rc == DM_OK) t->vec.forget();                // the step zeroed every gradient it visited, and it visited every row a batch has reached
  return rc;
}

int dm_dr_train_param_count(dm_handle_t h, int64_t *n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_param_count");
  int rc = dr_train_check(h, "dm_dr_train_param_count", false);
  if (rc != DM_OK) return rc;
  if (!n) return fail(h, DM_ERR_INVALID, "dm_dr_train_param_count: null argument");
  *n = h->dr->n_par;
  return DM_OK;
}

int dm_dr_train_download(dm_handle_t h, int what, void *out, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_download");
  int rc = dr_train_check(h, "dm_dr_train_download", what != 0);      // the weights of a loaded model can be read without training state
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if (!out || what < 0 || what > 3 || n != s->n_par) return fail(h, DM_ERR_INVALID, "dm_dr_train_download: what must be 0..3 and n the parameter count");
  const void *src = what == 0 ? s->d_par : s->tr->vec.buffer(what);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, src, (size_t)n * (s->dtype == DM_F64 ? 8 : 4), hipMemcpyDeviceToHost));
  return DM_OK;
}
