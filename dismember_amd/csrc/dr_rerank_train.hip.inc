// Deep-Retrieval E-step on the device: one training step of the RERANK model (dm_dr_rerank_*; DESIGN.md §11).
// Reference: deep-retrieval/src/main/scala/com/mass/dr/ (D/) model/RerankModel.scala (the graph: Embedding(num_item, E) -> flatten ->
// Linear(L E -> E), plus the softmax tables), scalann nn/SampledSoftmaxLoss.scala with nn/mixin/ParameterOptimizer.scala (the criterion:
// sampled softmax, and ITS OWN Adam over the two tables), dataset/MiniBatch.scala:52-61, optim/LocalOptimizer.scala:118-133,
// evaluation/Evaluator.scala:83-93 (fullEvaluate).
//
//   U = X rerank_w^T + rerank_b          X[r] = [rerank_emb[seq[r][j]], j < L],  id -1 = a zero row, no gradient;  U [B x E]
//   item[r][0] = target[r];  item[r][1..S] = S distinct ids != target[r], uniform over [0, num_item), ascending
//   z[r][s] = softmax_w[item[r][s]] . U[r] + softmax_b[item[r][s]];  loss = -(1/B) sum_r log softmax(z[r])[0];  G = (softmax(z) - onehot_0) / B
//   dU[r] = sum_s G[r][s] softmax_w[item[r][s]];  g_smw[item[r][s]] += G[r][s] U[r];  g_smb[item[r][s]] += G[r][s]
//   dW = dU^T X;  db = sum_r dU[r];  dX = dU rerank_w;  demb[id] += the E-wide slices of dX that row id fed
//
// Two trainable vectors, each with its own Adam: the graph's [rerank_emb ; rerank_w ; rerank_b] (dm_adam_opts rules, gradient replaced
// by every batch) and the criterion's [softmax_w ; softmax_b] (the reference's: eps 1e-7, no decay, its own time step).  The reference
// never clears the criterion's gradient (ParameterOptimizer.scala:65-88 only adds): accumulate = 1 keeps that running sum, accumulate = 0
// replaces it per batch.  The reference updates the tables inside criterion.backward, before model.backward; dU is fixed by then and the
// graph never reads the tables, so "all gradients, then both Adam updates" (dm_dr_rerank_adam_step) gives the same values.
//
// New kernels (T = float | double):
//   drr_sample_kernel           one wave per row, the row's ids in registers; counter RNG, bounded rejection, deterministic fallback
//   drr_sampled_softmax_kernel  one wave per row; lanes in groups of E / 4 (rounded up to a power of two) so that a wave holds
//                               64 / group slots at once and every lane loads four adjacent elements: z, softmax, G, dU, loss partial
//   drr_seg_smx_kernel          (item, slot) pairs sorted by item; one wave per destination adds G[slot] U[row(slot)] over its segment in
//                               sorted (= batch) order; nothing of size [B (S+1) x E] is ever written
// The graph half is the layer model's machinery: dr_gemm_kernel (U), drt_gemm_kernel (dX, dW/db in slabs), drt_pairs_kernel + sort +
// drt_seg_rows_kernel (demb).  Every sum has a fixed order, no floating-point atomics: the same state, batch, seed and step give the same bytes.

struct dm_dr_rr_train {
  TrainVec g, c;                                              // the graph's vector over d_rr_par, the criterion's over d_sm_par: each its own Adam
  int S = 0, accumulate = 1;
  unsigned long long seed = 0;
  int64_t fb_count = 0;                                       // forward/backward calls so far: the sampler's `step` of the next one
  DevGrow ws, io;
};

static void dr_rr_train_release(dm_dr_state *s) {
  dm_dr_rr_train *t = s->rt;
  if (!t) return;
  t->g.release(); t->c.release();
  for (DevGrow *g : {&t->ws, &t->io}) g->release();
  delete t;
  s->rt = nullptr;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
#define DRR_MAX_S1 256        // S + 1 slots of a row: four per lane
#define DRR_MAX_DRAWS 32      // draws per negative before the fallback
#define DRR_KEEP 16           // passes of gathered softmax_w rows a wave keeps in registers between the dot products and dU

// items[r][0] = target[r]; items[r][1 + k] = negatives[r][k] when they are given (else drr_sample_kernel fills them)
__global__ void drr_items_kernel(const int32_t *targets, const int32_t *negatives, int64_t B, int S, int32_t *items) {
  const int S1 = S + 1;
  const int64_t n = B * S1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / S1;
    const int k = (int)(i % S1);
    if (k == 0) items[i] = targets[r];
    else if (negatives) items[i] = negatives[r * S + (k - 1)];
  }
}

// The negative sampler: out[r * ld + k], k < S = S distinct ids != targets[r] in ascending order.  One wave per row; lane l holds the
// ids of positions l, l + 64, l + 128, l + 192 in registers.
//   key(row)   = splitmix(splitmix(seed ^ splitmix(step)) ^ row * 0xD6E8FEB86659FD93)
//   draw(c)    = splitmix(key(row) + c),  c = k * DRR_MAX_DRAWS + attempt  (k: the negative being drawn, attempt < DRR_MAX_DRAWS)
//   id(draw)   = ((draw >> 32) * num_item) >> 32      the high 32 bits scaled to [0, num_item): num_item < 2^31, bias below num_item / 2^32
// Negative k takes the first of its DRR_MAX_DRAWS draws that is neither the target nor one of the k ids held.  If all are taken: the
// fallback probes id + 1, id + 2, ... (cyclically) from the last draw.  At most k + 1 <= S ids are taken and S < num_item, so one of the
// next S + 1 ids is free: the probe loop has S + 1 trips.  No loop's trip count depends on a value the RNG produced.
struct DrrSampleParams { const int32_t *targets; int64_t B; int S; int64_t num_item; unsigned long long seed; long long step; int32_t *out; int64_t ld; };
__device__ __forceinline__ bool drr_id_free(const int32_t (&hv)[4], int lane, int k, int32_t c, int32_t tgt) {
  bool hit = false;
#pragma unroll
  for (int j = 0; j < 4; j++) hit = hit || (lane + 64 * j < k && hv[j] == c);
  return !__any(hit) && c != tgt;
}
__global__ __launch_bounds__(256) void drr_sample_kernel(DrrSampleParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = p.S;
  const int32_t N = (int32_t)p.num_item;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < p.B; row += (int64_t)gridDim.x * 4) {
    const int32_t tgt = p.targets[row];
    const unsigned long long key =
        dm_dev_splitmix(dm_dev_splitmix(p.seed ^ dm_dev_splitmix((unsigned long long)p.step)) ^ ((unsigned long long)row * 0xD6E8FEB86659FD93ull));
    int32_t hv[4] = {0, 0, 0, 0};
    for (int k = 0; k < S; k++) {
      int32_t c = 0;
      bool ok = false;
      for (int a = 0; a < DRR_MAX_DRAWS && !ok; a++) {
        const unsigned long long x = dm_dev_splitmix(key + (unsigned long long)(k * DRR_MAX_DRAWS + a));
        c = (int32_t)(((x >> 32) * (unsigned long long)N) >> 32);
        ok = drr_id_free(hv, lane, k, c, tgt);
      }
      for (int q = 0; q <= S && !ok; q++) {
        c = c + 1 >= N ? 0 : c + 1;
        ok = drr_id_free(hv, lane, k, c, tgt);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) if (lane + 64 * j == k) hv[j] = c;
    }
    // ascending order: the ids are distinct, so an id's position is the number of smaller ids
    int rank[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j2 = 0; j2 < 4; j2++)
      for (int l = 0; l < 64 && 64 * j2 + l < S; l++) {
        const int32_t v = __shfl(hv[j2], l);
#pragma unroll
        for (int j = 0; j < 4; j++) rank[j] += v < hv[j] ? 1 : 0;
      }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (lane + 64 * j < S) p.out[row * p.ld + rank[j]] = hv[j];      // (rank < S: S - 1 other ids at most are smaller)
  }
}

// Steps 3-4 of a row up to dU, one wave per row.  lps = 2^lg lanes share a slot (lane = grp * lps + sub): sub owns elements [4 c, 4 c + 4)
// of the slot's softmax_w row for c = sub, sub + lps, ... < E / 4, and the wave holds 64 / lps slots per pass (slot = pass * (64 / lps) + grp).
// KEEP: E / 4 <= lps and at most DRR_KEEP passes — the gathered rows stay in registers from the dot products to dU; otherwise they are
// read a second time (from the cache: a row's S + 1 rows are at most 256 E values).
// dU[r][e]: every group adds its slots in pass order, the groups are added in group order.  Loss partials as drt_softmax_ce_kernel.
template <typename T>
struct DrrSmxParams { const T *U, *sm_w, *sm_b; const int32_t *items; int64_t B; int S1, E, lg; T *G, *dU; double *partial; };
template <typename T, bool KEEP>
__global__ __launch_bounds__(256) void drr_sampled_softmax_kernel(DrrSmxParams<T> p) {
  __shared__ T zb[4][DRR_MAX_S1];          // a row's logits, then its G
  __shared__ T pt[4][256];                 // per group partial dU of one window of 4 lps elements
  __shared__ double wl[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lps = 1 << p.lg, grp = lane >> p.lg, sub = lane & (lps - 1), spw = 64 >> p.lg;
  const int E = p.E, S1 = p.S1, nchunk = E >> 2, npass = (S1 + spw - 1) / spw;
  const T fB = (T)p.B;
  double lsum = 0;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < p.B; base += (int64_t)gridDim.x * 4) {      // (the same trip count in all four waves: barriers below)
    const int64_t row = base + wave;
    const bool active = row < p.B;
    const T *u = p.U + (active ? row : 0) * E;
    const int32_t *it = p.items + (active ? row : 0) * S1;
    T wk[KEEP ? DRR_KEEP : 1][4];
    // ---- logits
    if (active) {
      if (KEEP) {
        T uv[4] = {0, 0, 0, 0};
        if (sub < nchunk) {
#pragma unroll
          for (int e = 0; e < 4; e++) uv[e] = u[4 * sub + e];
        }
#pragma unroll
        for (int ps = 0; ps < DRR_KEEP; ps++) {
          if (ps < npass) {
            const int s = ps * spw + grp;
            const bool live = s < S1;
            const int32_t id = live ? it[s] : 0;
#pragma unroll
            for (int e = 0; e < 4; e++) wk[ps][e] = 0;
            if (live && sub < nchunk) {
              const T *wr = p.sm_w + (int64_t)id * E + 4 * sub;
#pragma unroll
              for (int e = 0; e < 4; e++) wk[ps][e] = wr[e];
            }
            T d = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) d += uv[e] * wk[ps][e];
            for (int o = lps >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o);
            if (live && sub == 0) zb[wave][s] = d + p.sm_b[id];
          }
        }
      } else {
        for (int ps = 0; ps < npass; ps++) {
          const int s = ps * spw + grp;
          const bool live = s < S1;
          const int32_t id = live ? it[s] : 0;
          T d = 0;
          if (live) {
            const T *wr = p.sm_w + (int64_t)id * E;
            for (int c = sub; c < nchunk; c += lps) {
#pragma unroll
              for (int e = 0; e < 4; e++) d += u[4 * c + e] * wr[4 * c + e];
            }
          }
          for (int o = lps >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o);
          if (live && sub == 0) zb[wave][s] = d + p.sm_b[id];
        }
      }
    }
    __syncthreads();
    // ---- softmax over the S + 1 slots, G, the row's loss
    if (active) {
      T v[4], m = -INFINITY, sum = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) { const int k = lane + 64 * j; v[j] = k < S1 ? zb[wave][k] : (T)-INFINITY; m = v[j] > m ? v[j] : m; }
      const T z0 = __shfl(v[0], 0);
      m = dr_wave_max<T>(m);
#pragma unroll
      for (int j = 0; j < 4; j++) { v[j] = DrKey<T>::ex(v[j] - m); sum += v[j]; }
      sum = dr_wave_sum<T>(sum);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int k = lane + 64 * j;
        if (k < S1) {
          const T g = (v[j] / sum - (k == 0 ? (T)1 : (T)0)) / fB;
          zb[wave][k] = g;
          p.G[row * S1 + k] = g;
        }
      }
      lsum += (double)((m + DrTol<T>::lg(sum)) - z0);
    }
    __syncthreads();
    // ---- dU, one window of 4 lps elements at a time (KEEP: the only one)
    for (int c0 = 0; c0 < nchunk; c0 += lps) {
      const int c = c0 + sub;
      if (active) {
        T acc[4] = {0, 0, 0, 0};
        if (KEEP) {
#pragma unroll
          for (int ps = 0; ps < DRR_KEEP; ps++) {
            if (ps < npass) {
              const int s = ps * spw + grp;
              if (s < S1) {
                const T g = zb[wave][s];
#pragma unroll
                for (int e = 0; e < 4; e++) acc[e] += g * wk[ps][e];
              }
            }
          }
        } else if (c < nchunk) {
          for (int ps = 0; ps < npass; ps++) {
            const int s = ps * spw + grp;
            if (s < S1) {
              const T g = zb[wave][s];
              const T *wr = p.sm_w + (int64_t)it[s] * E + 4 * c;
#pragma unroll
              for (int e = 0; e < 4; e++) acc[e] += g * wr[e];
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) pt[wave][(grp * lps + sub) * 4 + e] = acc[e];
      }
      __syncthreads();
      if (active) {
        for (int x = lane; x < 4 * lps; x += 64) {
          const int e = 4 * c0 + x;
          if (e < E) {
            T a = pt[wave][x];
            for (int g = 1; g < spw; g++) a += pt[wave][g * 4 * lps + x];
            p.dU[row * E + e] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  if (lane == 0) wl[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

// The softmax tables' gradient.  keys (item ids, sorted, stable) / vals (slot = r (S+1) + s): one wave per sorted position, the wave at a
// destination's FIRST position owns the row.  MODE 0: clear row and bias; 1: write; 2: add the batch's sum into the stored gradient.
// The segment is added in sorted (= batch) order: gw[item][e] = sum_q G[slot_q] U[slot_q / (S+1)][e], gb[item] = sum_q G[slot_q] (lane 63).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void drr_seg_smx_kernel(const unsigned long long *keys, const int32_t *vals, int64_t m, int64_t NR, const T *G,
                                                          const T *U, int S1, int E, T *gw, T *gb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < m; i += (int64_t)gridDim.x * 4) {
    const unsigned long long key = keys[i];
    if (key >= (unsigned long long)NR || (i > 0 && keys[i - 1] == key)) continue;
    T *dst = gw + (int64_t)key * E;
    if (MODE == 0) {
      for (int e = lane; e < E; e += 64) dst[e] = (T)0;
      if (lane == 63) gb[key] = (T)0;
      continue;
    }
    const int64_t qe = drt_segment_end(keys, i, m, key, lane);
    for (int e = lane; e < E; e += 64) {
      T acc = 0;
      int64_t q = i;
      for (; q + 4 <= qe; q += 4) {                         // four loads in flight, added in order
        const int32_t v0 = vals[q], v1 = vals[q + 1], v2 = vals[q + 2], v3 = vals[q + 3];
        const T g0 = G[v0], g1 = G[v1], g2 = G[v2], g3 = G[v3];
        const T x0 = U[(int64_t)(v0 / S1) * E + e], x1 = U[(int64_t)(v1 / S1) * E + e], x2 = U[(int64_t)(v2 / S1) * E + e], x3 = U[(int64_t)(v3 / S1) * E + e];
        acc += g0 * x0; acc += g1 * x1; acc += g2 * x2; acc += g3 * x3;
      }
      for (; q < qe; q++) { const int32_t v = vals[q]; acc += G[v] * U[(int64_t)(v / S1) * E + e]; }
      dst[e] = MODE == 2 ? dst[e] + acc : acc;
    }
    if (lane == 63) {
      T b = 0;
      for (int64_t q = i; q < qe; q++) b += G[vals[q]];
      gb[key] = MODE == 2 ? gb[key] + b : b;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// (launch kinds under DM_DR_TIME_LAUNCHES=1: EV_DRR_* in host_request.hip.inc)
static int drr_check(dm_ctx *h, const char *who, bool need_init) {
  dm_dr_state *s = h->dr;
  if (!s || !s->loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": Deep-Retrieval model not loaded");
  if (!s->has_rerank) return fail(h, DM_ERR_STATE, std::string(who) + ": model was loaded without rerank arrays");
  if (need_init && !s->rt) return fail(h, DM_ERR_STATE, std::string(who) + ": call dm_dr_rerank_train_init first");
  return DM_OK;
}

int dm_dr_rerank_train_init(dm_handle_t h, const dm_adam_opts *graph, const dm_adam_opts *softmax, int num_sampled, uint64_t seed, int accumulate) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_train_init");
  int rc = drr_check(h, "dm_dr_rerank_train_init", false);
  if (rc != DM_OK) return rc;
  if (!graph || !(graph->lr > 0) || (softmax && !(softmax->lr > 0))) return fail(h, DM_ERR_INVALID, "dm_dr_rerank_train_init: bad optimizer options");
  dm_dr_state *s = h->dr;
  if (num_sampled < 1 || num_sampled >= s->num_item) return fail(h, DM_ERR_INVALID, "dm_dr_rerank_train_init: num_sampled must be in [1, num_item)");
  if (num_sampled + 1 > DRR_MAX_S1) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_train_init: at most 255 sampled classes");
  HIPCHK(h, hipSetDevice(h->device));
  dr_rr_train_release(s);
  dm_dr_rr_train *t = new dm_dr_rr_train();
  s->rt = t;
  const size_t es = s->dtype == DM_F64 ? 8 : 4;
  const int64_t NI = s->num_item, E = s->E;
  dm_adam_opts crit{};
  if (softmax) crit = *softmax;
  else { crit.lr = graph->lr; crit.lr_decay = 0; crit.beta1 = 0.9; crit.beta2 = 0.999; crit.eps = 1e-7; }      // SampledSoftmaxLoss.scala
  if ((rc = t->g.init(h, NI, (int)E, NI * E + E * (int64_t)s->L * E + E, es, *graph)) != DM_OK || (rc = t->c.init(h, NI, (int)E, NI * E + NI, es, crit)) != DM_OK) {
    dr_rr_train_release(s);      // (a handle that is not training, not one that trains on null buffers)
    return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  t->S = num_sampled; t->seed = seed; t->accumulate = accumulate ? 1 : 0;
  return DM_OK;
}

int dm_dr_rerank_train_free(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_train_free");
  if (!h->dr) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dr_rr_train_release(h->dr);
  return DM_OK;
}

static int drr_launch_sampler(dm_ctx *h, const int32_t *d_tgt, int64_t B, long long step, int32_t *out, int64_t ld) {
  dm_dr_state *s = h->dr;
  DrrSampleParams sp{};
  sp.targets = d_tgt; sp.B = B; sp.S = s->rt->S; sp.num_item = s->num_item; sp.seed = s->rt->seed; sp.step = step; sp.out = out; sp.ld = ld;
  return LAUNCH(h, drr_sample_kernel, dim3(drt_blocks(h, B, 4)), dim3(256), 0, sp);
}

// rows x [L] ids -> U [rows x E] (RerankModel.forward; the same launch dm_dr_recommend makes for its user vectors)
template <typename T>
static int drr_user_vectors(dm_ctx *h, const int32_t *d_seq, int64_t rows, T *U, int kind, bool on) {
  dm_dr_state *s = h->dr;
  DrGemmParams<T> g{};
  g.A = (const T *)s->d_rr_emb; g.lda = 0; g.gidx = d_seq; g.Lg = s->L; g.E = s->E;
  g.B = (const T *)s->d_rr_w; g.ldb = (int64_t)s->L * s->E; g.bias = (const T *)s->d_rr_b; g.zero = (const T *)s->d_zero;
  g.C = U; g.ldc = s->E; g.M = rows; g.N = s->E; g.Kd = s->L * s->E;
  dim3 grid((unsigned)((g.N + DR_TN - 1) / DR_TN), (unsigned)((g.M + DR_TM - 1) / DR_TM));
  return timed(h, kind, on, [&] { return LAUNCH(h, dr_gemm_kernel<T>, grid, dim3(256), 0, g); });
}

template <typename T>
static int drr_fb_dev_t(dm_ctx *h, const int32_t *d_seq, const int32_t *d_tgt, const int32_t *d_neg, int64_t B, double *out_loss) {
  dm_dr_state *s = h->dr;
  dm_dr_rr_train *t = s->rt;
  const int L = s->L, E = s->E, S = t->S, S1 = S + 1;
  const int64_t NI = s->num_item, m1 = B * L, m2 = B * S1, mm = std::max(m1, m2);
  if (mm >= ((int64_t)1 << 31) || B > (int64_t)DRT_MAX_ROWS)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_forward_backward: batch too large (at most 4 194 240 rows, and B max(L, S + 1) below 2^31): split it and accumulate on the host");
  if (!d_neg && 2 * (int64_t)S > NI)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_forward_backward: the device draws negatives for 2 num_sampled <= num_item only: pass the negatives");
  const bool detail = dr_time_launches();
  const int64_t slabs = (B + DRT_SLAB - 1) / DRT_SLAB;
  const int nb = (int)std::min<int64_t>((B + 3) / 4, 1024);                  // loss partials: a function of B alone
  const int cols = L * E;
  int rc;
  DevArena ar(t->ws, 8);
  const size_t o_u = ar.add((size_t)B * E * sizeof(T)), o_du = ar.add((size_t)B * E * sizeof(T)), o_g = ar.add((size_t)m2 * sizeof(T));
  const size_t o_items = ar.add((size_t)m2 * 4), o_dx = ar.add((size_t)m1 * E * sizeof(T));
  const size_t o_k0 = ar.add((size_t)mm * 8), o_k1 = ar.add((size_t)mm * 8), o_v0 = ar.add((size_t)mm * 4), o_v1 = ar.add((size_t)mm * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(mm));
  const size_t o_part = ar.add((size_t)slabs * E * ((size_t)cols + 1) * sizeof(T));
  const size_t o_lp = ar.add((size_t)nb * 8), o_loss = ar.add(8);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  T *U = ar.ptr<T>(o_u), *dU = ar.ptr<T>(o_du), *G = ar.ptr<T>(o_g), *dX = ar.ptr<T>(o_dx), *part = ar.ptr<T>(o_part);
  int32_t *items = ar.ptr<int32_t>(o_items);
  const DrtSortBufs sb{ar.ptr<unsigned long long>(o_k0), ar.ptr<unsigned long long>(o_k1), ar.ptr<int32_t>(o_v0), ar.ptr<int32_t>(o_v1), ar.ptr<uint32_t>(o_tmp)};
  const unsigned long long *ks;
  const int32_t *vs;
  T *gg = (T *)t->g.grad, *sg = (T *)t->c.grad;
  // ---- zeroGradParameters of the graph: the rows the last batch reached (the dense blocks are overwritten below); the criterion's
  // gradient is cleared only when it does not accumulate
  if (t->g.prev_m > 0) {
    if ((rc = LAUNCH(h, (drt_seg_rows_kernel<T, true>), dim3(drt_blocks(h, t->g.prev_m, 4)), dim3(256), 0, (const unsigned long long *)t->g.prev.p, nullptr,
                     t->g.prev_m, NI, nullptr, E, gg)) != DM_OK) return rc;
    t->g.forget();
  }
  if (t->c.prev_m > 0) {
    if ((rc = LAUNCH(h, (drr_seg_smx_kernel<T, 0>), dim3(drt_blocks(h, t->c.prev_m, 4)), dim3(256), 0, (const unsigned long long *)t->c.prev.p, nullptr,
                     t->c.prev_m, NI, nullptr, nullptr, S1, E, sg, sg + NI * E)) != DM_OK) return rc;
    t->c.forget();
  }
  // ---- the S + 1 classes of every row
  rc = timed(h, EV_DRR_SAMPLE, detail, [&] {
    const int r = LAUNCH(h, drr_items_kernel, dim3(drt_blocks(h, m2, 256)), dim3(256), 0, d_tgt, d_neg, B, S, items);
    return r != DM_OK || d_neg ? r : drr_launch_sampler(h, d_tgt, B, (long long)t->fb_count, items + 1, S1);
  });
  if (rc != DM_OK) return rc;
  t->fb_count += 1;
  // ---- forward: user vectors, then logits / softmax / G / dU / loss in one kernel
  if ((rc = drr_user_vectors<T>(h, d_seq, B, U, EV_DRR_FWD, detail)) != DM_OK) return rc;
  {
    DrrSmxParams<T> sp{};
    sp.U = U; sp.sm_w = (const T *)s->d_sm_w; sp.sm_b = (const T *)s->d_sm_b; sp.items = items; sp.B = B; sp.S1 = S1; sp.E = E;
    sp.G = G; sp.dU = dU; sp.partial = ar.ptr<double>(o_lp);
    int lg = 2;
    while ((1 << lg) < E / 4 && lg < 6) lg++;
    sp.lg = lg;
    const int spw = 64 >> lg;
    const bool keep = E / 4 <= (1 << lg) && (S1 + spw - 1) / spw <= DRR_KEEP;
    rc = timed(h, EV_DRR_SOFTMAX, detail, [&] {
      const int r = keep ? LAUNCH(h, (drr_sampled_softmax_kernel<T, true>), dim3((unsigned)nb), dim3(256), 0, sp)
                         : LAUNCH(h, (drr_sampled_softmax_kernel<T, false>), dim3((unsigned)nb), dim3(256), 0, sp);
      return r != DM_OK ? r : LAUNCH(h, drt_loss_sum_kernel, dim3(1), dim3(64), 0, sp.partial, nb, 1, B, ar.ptr<double>(o_loss));
    });
    if (rc != DM_OK) return rc;
  }
  // ---- the softmax tables' gradient: sort the slots by item, one wave per item
  rc = timed(h, EV_DRR_SMGRAD, detail, [&]() -> int {
    if ((rc = drt_sort_slots(h, items, m2, NI, sb, ks, vs)) != DM_OK) return rc;
    rc = t->accumulate ? LAUNCH(h, (drr_seg_smx_kernel<T, 2>), dim3(drt_blocks(h, m2, 4)), dim3(256), 0, ks, vs, m2, NI, G, U, S1, E, sg, sg + NI * E)
                       : LAUNCH(h, (drr_seg_smx_kernel<T, 1>), dim3(drt_blocks(h, m2, 4)), dim3(256), 0, ks, vs, m2, NI, G, U, S1, E, sg, sg + NI * E);
    if (rc != DM_OK) return rc;
    if (!t->accumulate && (rc = t->c.remember(h, ks, m2)) != DM_OK) return rc;
    return t->c.mark_active(h, drt_blocks(h, m2, 256), items, m2);
  });
  if (rc != DM_OK) return rc;
  // ---- the graph: dX = dU rerank_w, then dW / db over slabs of the batch
  {
    DrtGemmParams<T> g{};
    g.A = dU; g.a_rs = E; g.a_cs = 1;
    g.B = (const T *)s->d_rr_w; g.b_rs = 1; g.b_cs = cols;
    g.C = dX; g.ldc = cols; g.M = B; g.N = cols; g.Kd = E; g.slab = E;
    if ((rc = drt_launch_gemm<T>(h, g, EV_DRR_DX, detail)) != DM_OK) return rc;
    DrtGemmParams<T> q{};
    q.A = dU; q.a_rs = 1; q.a_cs = E;
    q.B = (const T *)s->d_rr_emb; q.gidx = d_seq; q.Lg = L; q.E = E; q.gcols = cols;
    q.C = part; q.ldc = cols + 1; q.c_slab = (int64_t)E * (cols + 1); q.M = E; q.N = cols + 1; q.Kd = B; q.slab = DRT_SLAB;
    if ((rc = drt_launch_gemm<T>(h, q, EV_DRR_DW, detail)) != DM_OK) return rc;
    rc = timed(h, EV_DRR_DW, detail, [&] {
      return LAUNCH(h, drt_slab_sum_kernel<T>, dim3(drt_blocks(h, (int64_t)E * (cols + 1), 256)), dim3(256), 0, part, (int)slabs, E, cols, gg + NI * E,
                    gg + NI * E + (int64_t)E * cols, cols);
    });
    if (rc != DM_OK) return rc;
  }
  // ---- embedding gradient: sort the history slots by item, one wave per item
  rc = timed(h, EV_DRR_EMB, detail, [&]() -> int {
    if ((rc = drt_sort_slots(h, d_seq, m1, NI, sb, ks, vs)) != DM_OK) return rc;
    if ((rc = LAUNCH(h, (drt_seg_rows_kernel<T, false>), dim3(drt_blocks(h, m1, 4)), dim3(256), 0, ks, vs, m1, NI, dX, E, gg)) != DM_OK) return rc;
    if ((rc = t->g.remember(h, ks, m1)) != DM_OK) return rc;
    return t->g.mark_active(h, drt_blocks(h, m1, 256), d_seq, m1);
  });
  if (rc != DM_OK) return rc;
  if (out_loss) HIPCHK(h, hipMemcpyAsync(out_loss, ar.ptr<double>(o_loss), 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_dr_rerank_forward_backward_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_targets, const int32_t *d_negatives, int64_t B, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_forward_backward");
  int rc = drr_check(h, "dm_dr_rerank_forward_backward", true);
  if (rc != DM_OK) return rc;
  if (B <= 0 || !d_seq_ids || !d_targets) return fail(h, DM_ERR_INVALID, "dm_dr_rerank_forward_backward: B must be positive and the arrays non-null");
  HIPCHK(h, hipSetDevice(h->device));
  return h->dr->dtype == DM_F32 ? drr_fb_dev_t<float>(h, d_seq_ids, d_targets, d_negatives, B, out_loss)
                                : drr_fb_dev_t<double>(h, d_seq_ids, d_targets, d_negatives, B, out_loss);
}

static int drr_check_items(dm_ctx *h, const int32_t *ids, int64_t n, const char *what) {
  const int64_t ni = h->dr->num_item;
  for (int64_t i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= ni) return fail(h, DM_ERR_INDEX, std::string("Deep-Retrieval rerank: ") + what + " outside [0, num_item)");
  return DM_OK;
}

int dm_dr_rerank_forward_backward(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, const int32_t *negatives, int64_t B, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_forward_backward");
  int rc = drr_check(h, "dm_dr_rerank_forward_backward", true);
  if (rc != DM_OK) return rc;
  if (B <= 0 || !seq_ids || !targets) return fail(h, DM_ERR_INVALID, "dm_dr_rerank_forward_backward: B must be positive and the arrays non-null");
  dm_dr_state *s = h->dr;
  dm_dr_rr_train *t = s->rt;
  if (B > (int64_t)DRT_MAX_ROWS || B * std::max<int64_t>(s->L, t->S + 1) >= ((int64_t)1 << 31))
    return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_forward_backward: batch too large (at most 4 194 240 rows, and B max(L, S + 1) below 2^31): split it and accumulate on the host");
  if ((rc = dr_check_ids(h, seq_ids, B * s->L)) != DM_OK) return rc;
  if ((rc = drr_check_items(h, targets, B, "target")) != DM_OK) return rc;
  if (negatives && (rc = drr_check_items(h, negatives, B * t->S, "negative")) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t b_seq = DevArena::up((size_t)B * s->L * 4), b_tgt = DevArena::up((size_t)B * 4), b_neg = DevArena::up((size_t)B * t->S * 4);
  if ((rc = t->io.reserve(h, b_seq + b_tgt + b_neg)) != DM_OK) return rc;
  int32_t *d_seq = (int32_t *)t->io.p, *d_tgt = (int32_t *)((char *)t->io.p + b_seq), *d_neg = (int32_t *)((char *)t->io.p + b_seq + b_tgt);
  HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids, (size_t)B * s->L * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_tgt, targets, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  if (negatives) HIPCHK(h, hipMemcpyAsync(d_neg, negatives, (size_t)B * t->S * 4, hipMemcpyHostToDevice, h->stream));
  return dm_dr_rerank_forward_backward_dev(h, d_seq, d_tgt, negatives ? d_neg : nullptr, B, out_loss);
}

int dm_dr_rerank_sample(dm_handle_t h, const int32_t *targets, int64_t B, int64_t step, int32_t *out) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_sample");
  int rc = drr_check(h, "dm_dr_rerank_sample", true);
  if (rc != DM_OK) return rc;
  if (B <= 0 || !targets || !out) return fail(h, DM_ERR_INVALID, "dm_dr_rerank_sample: B must be positive and the arrays non-null");
  dm_dr_state *s = h->dr;
  dm_dr_rr_train *t = s->rt;
  if (B > (int64_t)DRT_MAX_ROWS || B * (int64_t)(t->S + 1) >= ((int64_t)1 << 31)) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_sample: batch too large");
  if (2 * (int64_t)t->S > s->num_item) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_sample: the device draws negatives for 2 num_sampled <= num_item only");
  if ((rc = drr_check_items(h, targets, B, "target")) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t b_tgt = DevArena::up((size_t)B * 4), b_out = (size_t)B * t->S * 4;
  if ((rc = t->io.reserve(h, b_tgt + b_out)) != DM_OK) return rc;
  int32_t *d_tgt = (int32_t *)t->io.p, *d_out = (int32_t *)((char *)t->io.p + b_tgt);
  HIPCHK(h, hipMemcpyAsync(d_tgt, targets, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  if ((rc = drr_launch_sampler(h, d_tgt, B, (long long)step, d_out, t->S)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

// Both Adam updates, each with its own time step and its own rows-path / dense-path decision (TrainVec::plan_step).  The graph's tail
// [rerank_w ; rerank_b] is dense; the criterion's is softmax_b, one value per table row, and its gradient is put back when it accumulates.
int dm_dr_rerank_adam_step(dm_handle_t h, float grad_scale) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_adam_step");
  int rc = drr_check(h, "dm_dr_rerank_adam_step", true);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_dr_state *s = h->dr;
  dm_dr_rr_train *t = s->rt;
  unsigned long long act[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(&act[0], t->g.active_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&act[1], t->c.active_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const AdamPlan plan_g = t->g.plan_step(act[0]), plan_c = t->c.plan_step(act[1]);
  const bool f64 = s->dtype == DM_F64;
  rc = timed(h, EV_DRR_ADAM, dr_time_launches(), [&] {
    const int r = adam_step(h, t->g, plan_g, s->d_rr_par, f64, false, grad_scale, false, 1024);
    return r != DM_OK ? r : adam_step(h, t->c, plan_c, s->d_sm_par, f64, t->accumulate != 0, grad_scale, true, 256);
  });
  if (rc == DM_OK) { t->g.forget(); t->c.forget(); }      // the steps zeroed every gradient they visited (the accumulating criterion keeps no list)
  return rc;
}

int dm_dr_rerank_download(dm_handle_t h, int vec, int what, void *out, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_download");
  int rc = drr_check(h, "dm_dr_rerank_download", what != 0);       // the weights of a loaded model can be read without training state
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  const int64_t NI = s->num_item, E = s->E;
  const int64_t want = vec == 0 ? NI * E + E * (int64_t)s->L * E + E : NI * E + NI;
  if (!out || vec < 0 || vec > 1 || what < 0 || what > 3 || n != want)
    return fail(h, DM_ERR_INVALID, "dm_dr_rerank_download: vec must be 0 or 1, what 0..3 and n the vector's length");
  const void *src = what == 0 ? (vec == 0 ? s->d_rr_par : s->d_sm_par) : (vec == 0 ? s->rt->g : s->rt->c).buffer(what);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, src, (size_t)n * (s->dtype == DM_F64 ? 8 : 4), hipMemcpyDeviceToHost));
  return DM_OK;
}

// Evaluator.evaluateReRankModel's fullEvaluate: -mean log softmax(U softmax_w^T + softmax_b)[target] over all num_item classes.  Row chunks
// whose [rows x num_item] logits stay under 256 MB (DM_DR_FULL_LOSS_ROWS forces a chunk size); chunk sums are added in chunk order.
template <typename T>
static int drr_full_loss_t(dm_ctx *h, const int32_t *seq_ids, const int32_t *targets, int64_t B, double *out) {
  dm_dr_state *s = h->dr;
  const int L = s->L, E = s->E;
  const int64_t NI = s->num_item;
  int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / (NI * (int64_t)sizeof(T)));
  chunk = std::min<int64_t>(chunk, (int64_t)1 << 20);
  if (const long long v_ = env_int("DM_DR_FULL_LOSS_ROWS")) chunk = std::min<int64_t>(v_, (int64_t)1 << 20);
  chunk = std::min(chunk, B);
  const int nb = (int)std::min<int64_t>((chunk + 3) / 4, 1024);
  DevTemps tmp(h);
  int32_t *d_seq = nullptr, *d_tgt = nullptr;
  T *U = nullptr, *Z = nullptr;
  double *lp = nullptr;
  int rc;
  if ((rc = tmp.alloc(d_seq, (size_t)chunk * L * 4)) != DM_OK || (rc = tmp.alloc(d_tgt, (size_t)chunk * 4)) != DM_OK ||
      (rc = tmp.alloc(U, (size_t)chunk * E * sizeof(T))) != DM_OK || (rc = tmp.alloc(Z, (size_t)chunk * NI * sizeof(T))) != DM_OK ||
      (rc = tmp.alloc(lp, (size_t)(nb + 1) * 8)) != DM_OK) return rc;
  double total = 0;
  for (int64_t r0 = 0; r0 < B; r0 += chunk) {
    const int64_t n = std::min(chunk, B - r0);
    const int nbc = (int)std::min<int64_t>((n + 3) / 4, 1024);
    HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids + r0 * L, (size_t)n * L * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tgt, targets + r0, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = drr_user_vectors<T>(h, d_seq, n, U, EV_MAIN, false)) != DM_OK) return rc;
    DrGemmParams<T> g{};
    g.A = U; g.lda = E; g.gidx = nullptr; g.Lg = 0; g.E = E;
    g.B = (const T *)s->d_sm_w; g.ldb = E; g.bias = (const T *)s->d_sm_b; g.zero = (const T *)s->d_zero;
    g.C = Z; g.ldc = NI; g.M = n; g.N = (int)NI; g.Kd = E;
    if ((rc = dr_launch_gemm<T>(h, g, false)) != DM_OK) return rc;
    DrtSoftmaxParams<T> sp{};
    sp.Z = Z; sp.paths = d_tgt; sp.B = n; sp.K = (int)NI; sp.D = 1; sp.partial = lp;
    if ((rc = LAUNCH(h, drt_softmax_ce_kernel<T>, dim3((unsigned)nbc, 1), dim3(256), 0, sp)) != DM_OK ||
        (rc = LAUNCH(h, drt_loss_sum_kernel, dim3(1), dim3(64), 0, lp, nbc, 1, 1, lp + nb)) != DM_OK) return rc;      // B = 1: the chunk's sum
    double part = 0;
    HIPCHK(h, hipMemcpyAsync(&part, lp + nb, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    total += part;
  }
  *out = total / (double)B;
  return DM_OK;
}

int dm_dr_rerank_full_loss(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t B, double *out) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_rerank_full_loss");
  int rc = drr_check(h, "dm_dr_rerank_full_loss", false);
  if (rc != DM_OK) return rc;
  if (B <= 0 || !seq_ids || !targets || !out) return fail(h, DM_ERR_INVALID, "dm_dr_rerank_full_loss: B must be positive and the arguments non-null");
  dm_dr_state *s = h->dr;
  if (s->num_item >= ((int64_t)1 << 31)) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_rerank_full_loss: num_item must be below 2^31");
  if ((rc = dr_check_ids(h, seq_ids, B * s->L)) != DM_OK) return rc;
  if ((rc = drr_check_items(h, targets, B, "target")) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return s->dtype == DM_F32 ? drr_full_loss_t<float>(h, seq_ids, targets, B, out) : drr_full_loss_t<double>(h, seq_ids, targets, B, out);
}
