// OTM beam search in the reference's own arithmetic type (fp64).
//
// The reference instantiates the OTM scorer as DIN[Double] (otm/src/main/scala/com/mass/otm/model/DIN.scala:12-39,
// examples/.../otm/OTMTrainDeepModel.scala:43) and runs CandidateSearcher.beamSearch (otm/.../model/CandidateSearcher.scala:
// 58-80, buildBeamNodes :109-122) / OTMTree.beamSearchNodes (otm/.../tree/OTMTree.scala:67-91,174-212) on it.  The persistent
// beam kernel scores in fp32 (throughput mode); this file is the parity mode: the same level fold as a short pipeline of
// kernels over a whole batch of users, every product on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, dr_gemm_kernel<double>).
//
// Per batch of U users (a complete tree: every user has the same candidate count n_l on level l):
//   setup   T1 = K att.W^T  ([U*L x E], history rows gathered by the GEMM),  G = T1 W1b^T + b1          (once per search)
//   level   prune + expand: stable sort by (Double.compare descending, position), take beam, children 2c+1, 2c+2
//           H1 = Q W1a^T     ([U*n_l x E], candidate rows gathered by the GEMM: the 2E^2 flops of a row)
//           attention + epilogue per row: s_j = q.k_j / sqrt(E), mask -> -FLT_MAX, softmax (exp, sum, * 1/sum),
//           logit = w2 . relu(H1 + sum_j p_j G_j) + b2        (the per-user restructuring of DESIGN.md §3, in fp64)
// Candidate rows are user-major, so row -> user is a division; nothing is replicated per row.

template <typename T>
struct Otm64Prune {
  const int32_t *codes;      // [U][stride] current candidates
  const T *scores;           // [U][stride]
  int32_t *next;             // [U][stride] children
  int n, nb, first, stride;  // current count, kept (beam) count, first level: no sort; row stride of the three arrays
  int64_t U;
  int pcap;                  // power of two >= n
};

// java.lang.Double.compare order as an unsigned key, descending: smaller key = larger score; one canonical NaN (greatest)
__device__ __forceinline__ unsigned long long otm64_desc_key(double s) {
  unsigned long long b = (unsigned long long)__double_as_longlong(s);
  if (s != s) b = 0x7ff8000000000000ull;
  const unsigned long long asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return ~asc;
}

// sortBy(score)(reverse).take(beam) is a STABLE sort (CandidateSearcher.scala:117-120), i.e. the order of (descending key, position)
// pairs, which are unique; bitonic network over LDS.  Every thread of the workgroup calls it (uniform n, pcap = a power of two >= n);
// on return pos[0 .. n) lists the positions of sc[0 .. n) in that order.  The ONE statement of the order: the fp64 / long-history
// pipeline below and the fused DeepFM kernel (dfm_otm.hip.inc) both prune through it.
template <typename T>
__device__ __forceinline__ void otm64_sort_positions(unsigned long long *key, unsigned *pos, const T *sc, int n, int pcap) {
  // a float widens to double exactly and in order (-0.0f < +0.0f, one NaN class): the fp64 key serves both score types
  for (int i = threadIdx.x; i < pcap; i += blockDim.x) { key[i] = i < n ? otm64_desc_key((double)sc[i]) : ~0ull; pos[i] = i < n ? (unsigned)i : 0xFFFFFFFFu; }
  __syncthreads();
  for (int k = 2; k <= pcap; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int c = threadIdx.x; c < pcap / 2; c += blockDim.x) {
        const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1)), l = i + j;
        const unsigned long long a = key[i], b = key[l];
        const unsigned pa = pos[i], pb = pos[l];
        const bool a_first = a < b || (a == b && pa < pb);
        const bool asc = (i & k) == 0;
        if (a_first != asc) { key[i] = b; key[l] = a; pos[i] = pb; pos[l] = pa; }
      }
      __syncthreads();
    }
}

// one workgroup per user
template <typename T>
__global__ __launch_bounds__(256) void otm64_prune_expand_kernel(Otm64Prune<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem_o[];
  unsigned long long *key = (unsigned long long *)smem_o;
  unsigned *pos = (unsigned *)(key + p.pcap);
  const int64_t u = blockIdx.x;
  const int32_t *codes = p.codes + u * p.stride;
  int32_t *next = p.next + u * p.stride;
  if (p.first) {
    for (int i = threadIdx.x; i < p.n; i += blockDim.x) { const int32_t c = codes[i]; next[2 * i] = 2 * c + 1; next[2 * i + 1] = 2 * c + 2; }
    return;
  }
  otm64_sort_positions<T>(key, pos, p.scores + u * p.stride, p.n, p.pcap);
  for (int i = threadIdx.x; i < p.nb; i += blockDim.x) { const int32_t c = codes[pos[i]]; next[2 * i] = 2 * c + 1; next[2 * i + 1] = 2 * c + 2; }
}

template <typename T>
struct Otm64Attn {
  const T *emb;              // [num_index][E]
  const T *H1;               // [U*n][E]  W1a q
  const T *G;                // [U*L][E]  W1b att.W k_j + b1
  const T *w2;               // [E]
  T b2, scale;
  const int32_t *codes;      // [U][stride]
  const int32_t *seq;        // [U][L] history node codes, -1 = padding (a zero key row)
  T *scores;                 // [U][stride]
  int n, stride, L, E;
  int64_t U;
  const int32_t *counts;     // [U] live candidates of a user (TDM: ragged frontiers), or null: all n
  int use_mask;              // 1: padded positions get -FLT_MAX before the softmax (Mask.scala:17-35); 0: they score 0 like any zero row
};
template <typename T> __device__ __forceinline__ T otm_pl_exp(T x);
template <> __device__ __forceinline__ double otm_pl_exp<double>(double x) { return exp(x); }
template <> __device__ __forceinline__ float otm_pl_exp<float>(float x) { return expf(x); }

// One workgroup per (user, 64 candidate rows): the user's L key rows and G rows are staged in LDS once — a row then reads 2 L E
// elements from LDS instead of from L2 (17 KB per row at L = 17: the first version, one row per 16 lanes straight from global
// memory, spent 80 % of a level there).  16 lanes per candidate row; lane t holds features t, t+16, ...
#define OTM_PL_ROWS 64
static inline size_t otm_pl_attn_lds(int L, int E, size_t esz) { return (size_t)2 * L * E * esz + (size_t)L * 4 + 16; }
// (NE = E / 16 and the history loops are compile-time shaped: q / hacc / s stay in registers — with run-time bounds the compiler put the
// three arrays into scratch memory and the kernel ran 8x slower)
template <typename T, int NE>
__global__ __launch_bounds__(256) void otm64_attn_kernel(Otm64Attn<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem_a[];
  constexpr int E = NE * 16;
  const int L = p.L;
  T *Ks = (T *)smem_a;
  T *Gs = Ks + L * E;
  int32_t *kcs = (int32_t *)(Gs + L * E);
  const int nch = (p.n + OTM_PL_ROWS - 1) / OTM_PL_ROWS;
  const int64_t u = blockIdx.x / nch;
  const int ch = (int)(blockIdx.x - u * nch);
  const int cnt = p.counts ? (p.counts[u] < p.n ? p.counts[u] : p.n) : p.n;
  if (ch * OTM_PL_ROWS >= cnt) return;                       // (uniform: a chunk past the user's frontier)
  for (int t = threadIdx.x; t < L; t += 256) kcs[t] = p.seq[u * L + t];
  __syncthreads();
  for (int t = threadIdx.x; t < L * E; t += 256) {
    const int j = t / E, e = t - j * E;
    const int32_t kc = kcs[j];
    Ks[t] = kc >= 0 ? p.emb[(int64_t)kc * E + e] : (T)0;
    Gs[t] = p.G[(u * L + j) * E + e];
  }
  __syncthreads();
  const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  for (int k = 0; k < OTM_PL_ROWS / 16; k++) {
    const int i_ = ch * OTM_PL_ROWS + k * 16 + grp;
    const bool live = i_ < cnt;
    const int i = live ? i_ : 0;               // (a dead group runs along on slot 0 and stores nothing)
    const int64_t rr = u * p.n + i;
    const int32_t code = p.codes[u * p.stride + i];
    T q[NE], hacc[NE];
#pragma unroll
    for (int e = 0; e < NE; e++) { q[e] = p.emb[(int64_t)code * E + sub + 16 * e]; hacc[e] = p.H1[rr * E + sub + 16 * e]; }
    T s[DM_PIPE_MAXL];
    T mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < DM_PIPE_MAXL; j++) {
      s[j] = (T)0;
      if (j < L) {
        T part = 0;
#pragma unroll
        for (int e = 0; e < NE; e++) part += q[e] * Ks[j * E + sub + 16 * e];
        for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o);
        T sv = part * p.scale;                    // MatMul(transB) then Mask: scale, then the mask value (Mask.scala:17-35)
        if (kcs[j] < 0 && p.use_mask) sv = (T)(-FLT_MAX);
        s[j] = sv;
        mx = sv > mx ? sv : mx;
      }
    }
    T sum = 0;
#pragma unroll
    for (int j = 0; j < DM_PIPE_MAXL; j++)
      if (j < L) { s[j] = otm_pl_exp<T>(s[j] - mx); sum += s[j]; }     // SoftMax.scala:28-42: exp(x - max), sum, * 1/sum
    const T inv = (T)1 / sum;
#pragma unroll
    for (int j = 0; j < DM_PIPE_MAXL; j++)
      if (j < L) {
        const T pj = s[j] * inv;
#pragma unroll
        for (int e = 0; e < NE; e++) hacc[e] += pj * Gs[j * E + sub + 16 * e];
      }
    T part = 0;
#pragma unroll
    for (int e = 0; e < NE; e++) { const T hv = hacc[e] > (T)0 ? hacc[e] : (T)0; part += hv * p.w2[sub + 16 * e]; }
    for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (live && sub == 0) p.scores[u * p.stride + i] = part + p.b2;
  }
}
template <typename T, int NE>
static int otm_pl_launch_attn_ne(dm_ctx *h, const Otm64Attn<T> &a) {
  const size_t lds = otm_pl_attn_lds(a.L, a.E, sizeof(T));
  const int64_t blocks = a.U * ((a.n + OTM_PL_ROWS - 1) / OTM_PL_ROWS);
  return LAUNCH_LDS(h, (otm64_attn_kernel<T, NE>), dim3((unsigned)blocks), dim3(256), lds, a);
}
template <typename T>
static int otm_pl_launch_attn(dm_ctx *h, const Otm64Attn<T> &a) {
  return dispatch_E(h, a.E, "unsupported embed size", [&](auto e) { return otm_pl_launch_attn_ne<T, decltype(e)::value / 16>(h, a); });
}

template <typename T>
__global__ void otm64_init_kernel(int32_t *codes, T *scores, int64_t U, int stride, int start) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < U * (start + 1); t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = t / (start + 1);
    const int i = (int)(t % (start + 1));
    codes[u * stride + i] = start + i; scores[u * stride + i] = (T)0;
  }
}

// G's padded history rows: a -1 code contributes k_j = 0, so T1 = 0 and G_j = b1 (the GEMM bias) — exactly what the formula
// gives; nothing to patch.

template <typename T>
struct Otm64Out {
  const int32_t *codes; const T *scores; int stride, n;
  int32_t *out_ids; double *out_sc64; float *out_sc32; int32_t *out_cnt; int out_stride;    // final (either score type)
  int32_t *tr_codes; double *tr_sc64; float *tr_sc32; int32_t *tr_cnt; int tr_levels, tr_cap, level;   // trace slot (or null)
  int64_t U, u0;
};
template <typename T>
__global__ void otm64_emit_kernel(Otm64Out<T> p) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < p.U * p.n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = t / p.n;
    const int i = (int)(t % p.n);
    const int32_t c = p.codes[u * p.stride + i];
    const double s = (double)p.scores[u * p.stride + i];
    const int64_t gu = p.u0 + u;
    if (p.tr_cnt) {
      const int64_t tb = gu * p.tr_levels + p.level;
      if (i < p.tr_cap) {
        p.tr_codes[tb * p.tr_cap + i] = c;
        if (p.tr_sc64) p.tr_sc64[tb * p.tr_cap + i] = s; else p.tr_sc32[tb * p.tr_cap + i] = (float)s;
      }
      if (i == 0) p.tr_cnt[tb] = p.n;
    }
    if (p.out_ids && i < p.out_stride) {
      p.out_ids[gu * p.out_stride + i] = c;
      if (p.out_sc64) p.out_sc64[gu * p.out_stride + i] = s; else p.out_sc32[gu * p.out_stride + i] = (float)s;
      if (i == 0) p.out_cnt[gu] = p.n;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// d_seq [U][L] on the device; outputs on the device ([U][2*beam] ids / scores of the requested type, [U] counts; trace
// [U][max_levels][cap]).  Exactly one of d_sc64 / d_sc32 (and of d_ts64 / d_ts32 when tracing) is non-null.
// ---- the fused persistent kernel (beam_kernel_f64.hip.inc): the default; the per-level pipeline below stays for frontiers that
// outgrow LDS, for searches with no level to score, and as a cross-check (DM_OTM64_PIPELINE=1 in the environment)
template <int E, int KQ, int KT = 1>
static int launch_beam64_EK(dm_ctx *h, const Beam64Params &p, int grid, int lds) {
  if (KT == 1) snprintf(h->last_kernel, sizeof(h->last_kernel), "dm_beam64_kernel<%d, %d>", E, KQ);
  else snprintf(h->last_kernel, sizeof(h->last_kernel), "dm_beam64_kernel<%d, %d, %d>", E, KQ, KT);
  HIPCHK(h, lds_opt_in(dm_beam64_kernel<E, KQ, KT>, lds));
  return timed(h, EV_MAIN, !(p.host_direct && !h->time_direct), [&] {      // single-request path: the launch and nothing else
    return LAUNCH(h, (dm_beam64_kernel<E, KQ, KT>), dim3(grid), dim3(DM64_BLOCK), lds, p);
  });
}
template <int E>
static int launch_beam64_E(dm_ctx *h, const Beam64Params &p, int grid, int lds) {
  if (p.L > DM_MAXL) return launch_beam64_EK<E, 4, 2>(h, p, grid, lds);          // 17 .. 32 history positions: two key tiles
  switch ((p.L + 3) / 4) {
    case 1: return launch_beam64_EK<E, 1>(h, p, grid, lds);
    case 2: return launch_beam64_EK<E, 2>(h, p, grid, lds);
    case 3: return launch_beam64_EK<E, 3>(h, p, grid, lds);
    default: return launch_beam64_EK<E, 4>(h, p, grid, lds);
  }
}

// returns DM_OK and *done = true when the fused kernel ran the search
static int beam64_search_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, int beam, int leaf_level, int32_t *d_ids,
                             double *d_sc64, float *d_sc32, int32_t *d_counts, int max_levels, int cap, int32_t *d_tc,
                             double *d_ts64, float *d_ts32, int32_t *d_tn, bool *done, bool host_direct = false) {
  *done = false;
  if (env_on("DM_OTM64_PIPELINE")) return DM_OK;
  int start, level0;
  level_start_int(beam, &start, &level0);
  if (leaf_level <= level0) return DM_OK;
  if (L > DM_PIPE_MAXL) return DM_OK;
  if (L > DM_MAXL && env_on("DM_LONG_PIPELINE")) return DM_OK;      // (A/B: 17 .. 32 positions on the per-level pipeline)
  const int kt = L > DM_MAXL ? 2 : 1;         // key tiles of 16 history positions
  const int E = h->embed;
  int fcap, pcap;
  frontier_caps(beam, &fcap, &pcap);
  if (pcap > 32768) return DM_OK;          // sort positions are 16-bit
  int nteams = 0, lds = 0, b_global = 0, v_global = 0;
  // Team shapes, best first.  Small frontiers (OTM.recommend's default beam 20): twelve one-wave teams with everything in LDS.  Up to 512
  // slots (beam <= 256): twelve one-wave teams again — no team barriers, no split of a level's tiles, twelve users in flight per CU — with the
  // beam's codes AND the candidates' scores in the team's global scratch (L2), which leaves 1.2 KB of LDS per team; then six two-wave teams
  // (codes in the scratch), then 4 / 2 / 1 teams with everything in LDS.
  const bool no12 = env_on("DM_OTM64_NO12G"), no6 = env_on("DM_OTM64_NO6");
  const int cands[6][3] = {{12, 0, 0}, {12, 1, 1}, {6, 1, 0}, {4, 0, 0}, {2, 0, 0}, {1, 0, 0}};
  for (int ci = 0; ci < 6; ci++) {
    if (ci == 0 && pcap > 128) continue;
    if (ci == 1 && (pcap > 512 || no12)) continue;
    if (ci == 2 && no6) continue;
    const Beam64Lds l = dm_beam64_lds(E, cands[ci][0], fcap, pcap, cands[ci][1], cands[ci][2]);
    if (l.total <= 160 * 1024) { nteams = cands[ci][0]; b_global = cands[ci][1]; v_global = cands[ci][2]; lds = l.total; break; }
  }
  if (!nteams) return DM_OK;
  int rc = ensure_frags64(h);
  if (rc != DM_OK) return rc;
  const int64_t groups = (U + nteams - 1) / nteams;
  const int grid = (int)(groups < h->n_cu ? groups : (int64_t)h->n_cu);
  const size_t per_team = ((size_t)kt * (E / 4) * 64 + (size_t)kt * 4 * (E / 16) * 64 + (size_t)fcap / 2 + (size_t)pcap) * 8;
  const size_t need = (size_t)h->n_cu * 12 * per_team;
  if ((rc = h->scratch64.reserve(h, need)) != DM_OK) return rc;
  const double *base = (const double *)h->d_compact;
  const size_t n = (size_t)E * E;
  const double *l1_b = base + h->num_index * E + 3 * n, *l2_w = l1_b + E;
  const double b2 = h->lazy.b2_64;
  Beam64Params p{};
  p.static_users = U <= (int64_t)grid * nteams ? 1 : 0;
  p.b_global = b_global; p.v_global = v_global;
  p.host_direct = (host_direct && p.static_users) ? 1 : 0;
  if (host_direct && !p.host_direct) return DM_OK;      // (the caller falls back to the staged path)
  p.force_lds_sort = env_on("DM_OTM64_LDS_SORT") ? 1 : 0;
  p.sm_scale = sm_scale64(h);
  p.phase_cycles = h->d_phase;
  if (!p.static_users || U > 64) HIPCHK(h, reset_search_counters(h, false));
  const double *f = (const double *)h->lazy.d_frag64;
  p.emb = base; p.num_index = h->num_index; p.w1aA = (const f64x2 *)f; p.attA = f + n; p.w1bB = f + 2 * n; p.b1 = l1_b; p.w2 = l2_w; p.b2 = b2;
  p.seq = d_seq; p.U = U; p.L = L; p.beam = beam; p.leaf_level = leaf_level; p.nteams = nteams; p.cap = fcap; p.pcap = pcap;
  p.out_ids = d_ids; p.out_sc64 = d_sc64; p.out_sc32 = d_sc32; p.out_counts = d_counts; p.out_stride = 2 * beam;
  p.tr_codes = d_tc; p.tr_sc64 = d_ts64; p.tr_sc32 = d_ts32; p.tr_counts = d_tn; p.tr_levels = d_tn ? max_levels : 0; p.tr_cap = cap;
  p.scratch = (double *)h->scratch64.p; p.next_user = &h->d_ctr->queue_head;
  p.scored_rows = (p.static_users && U <= 64) ? &h->d_ctr->rows_sink : &h->d_ctr->rows;
  rc = dispatch_E(h, E, "unsupported embed size", [&](auto e) { return launch_beam64_E<decltype(e)::value>(h, p, grid, lds); });
  if (rc == DM_OK) *done = true;
  return rc;
}

// The per-level pipeline in the model's own type: T = double for an f64 model (round 2's parity path, the fused kernel's fallback),
// T = float for an f32 model whose histories are longer than the fused kernels' 16 positions (L <= DM_PIPE_MAXL = 32).
template <typename T>
static int otm_pipeline_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, int beam, int leaf_level, int32_t *d_ids,
                            double *d_sc64, float *d_sc32, int32_t *d_counts, int max_levels, int cap, int32_t *d_tc,
                            double *d_ts64, float *d_ts32, int32_t *d_tn) {
  snprintf(h->last_kernel, sizeof(h->last_kernel), sizeof(T) == 8 ? "otm64 pipeline" : "otm level pipeline (f32, L > 16)");
  // the pipeline's emit kernel writes the live slots only (the fused kernel fills whole rows itself)
  HIPCHK(h, prefill_results(h, U, (size_t)2 * beam, d_ids, d_sc64 ? (void *)d_sc64 : (void *)d_sc32, d_sc64 ? 8 : 4, d_counts));
  const int E = h->embed;
  const T *base = (const T *)h->d_compact;
  const T *att_w = base + h->num_index * E, *l1_w = att_w + (int64_t)E * E, *l1_b = l1_w + (int64_t)2 * E * E;
  const T *l2_w = l1_b + E;
  T b2;
  HIPCHK(h, hipMemcpy(&b2, l2_w + E, sizeof(T), hipMemcpyDeviceToHost));
  int64_t rows_scored = 0;
  int start, level0;
  level_start_int(beam, &start, &level0);
  const int stride = 2 * (beam > start + 1 ? beam : start + 1);
  // users per pass: the [Uc * stride x E] H1 buffer stays below 1 GiB
  int64_t Uc = ((int64_t)1 << 30) / ((int64_t)stride * E * (int64_t)sizeof(T));
  if (Uc < 1) Uc = 1;
  if (Uc > U) Uc = U;
  const size_t b_codes = (size_t)Uc * stride * 4, b_sc = (size_t)Uc * stride * sizeof(T), b_h1 = (size_t)Uc * stride * E * sizeof(T);
  const size_t b_t1 = (size_t)Uc * L * E * sizeof(T);
  DevArena ar(h->ws);
  const size_t o_c0 = ar.add(b_codes), o_c1 = ar.add(b_codes), o_sc = ar.add(b_sc), o_h1 = ar.add(b_h1), o_t1 = ar.add(b_t1), o_g = ar.add(b_t1), o_zero = ar.add(256);
  int rc = ar.commit(h);
  if (rc != DM_OK) return rc;
  int32_t *c0 = ar.ptr<int32_t>(o_c0), *c1 = ar.ptr<int32_t>(o_c1);
  T *sc = ar.ptr<T>(o_sc), *H1 = ar.ptr<T>(o_h1), *T1 = ar.ptr<T>(o_t1), *G = ar.ptr<T>(o_g), *zero = ar.ptr<T>(o_zero);
  HIPCHK(h, hipMemsetAsync(zero, 0, 256, h->stream));
  int pcap = 2;
  while (pcap < stride) pcap <<= 1;
  const size_t lds_prune = (size_t)pcap * 12;
  if (lds_prune > 160 * 1024) return fail(h, DM_ERR_UNSUPPORTED, "fp64 OTM beam search: beam too large for the LDS sort");
  HIPCHK(h, lds_opt_in(otm64_prune_expand_kernel<T>, lds_prune));          // once for the launches of every level below
  for (int64_t u0 = 0; u0 < U; u0 += Uc) {
    const int64_t Un = U - u0 < Uc ? U - u0 : Uc;
    const int32_t *seq = d_seq + u0 * L;
    // setup: T1 = K att.W^T (history rows gathered; -1 -> zero row), G = T1 W1b^T + b1
    DrGemmParams<T> g{};
    g.A = base; g.lda = E; g.gidx = seq; g.Lg = 1; g.E = E; g.B = att_w; g.ldb = E; g.bias = nullptr; g.zero = zero;
    g.C = T1; g.ldc = E; g.M = Un * L; g.N = E; g.Kd = E;
    if ((rc = dr_launch_gemm<T>(h, g)) != DM_OK) return rc;
    g.A = T1; g.gidx = nullptr; g.B = l1_w + E; g.ldb = 2 * E; g.bias = l1_b; g.C = G;
    if ((rc = dr_launch_gemm<T>(h, g)) != DM_OK) return rc;
    LAUNCHCHK(h, otm64_init_kernel<T>, dim3(256), dim3(256), 0, c0, sc, Un, stride, start);
    int n = start + 1;
    int32_t *cur = c0, *nxt = c1;
    for (int level = level0; level < leaf_level; level++) {
      const bool first = level == level0;
      const int nb = first ? n : (n < beam ? n : beam);
      Otm64Prune<T> pp{cur, sc, nxt, n, nb, first ? 1 : 0, stride, Un, pcap};
      LAUNCHCHK(h, otm64_prune_expand_kernel<T>, dim3((unsigned)Un), dim3(256), first ? 0 : lds_prune, pp);
      n = 2 * nb;
      std::swap(cur, nxt);
      // H1 = Q W1a^T over the Un * n candidate rows.  Rows are addressed [u][stride]: one GEMM per user block would waste
      // launches, so the candidate codes are compacted on the fly by the gather index (row m -> codes[(m / n) * stride + m % n])
      // when n < stride; the GEMM takes a dense index, hence a compact copy.
      int32_t *dense = nxt;     // the buffer just consumed is free: reuse it for the dense [Un * n] code list
      if (n != stride) {
        HIPCHK(h, hipMemcpy2DAsync(dense, (size_t)n * 4, cur, (size_t)stride * 4, (size_t)n * 4, (size_t)Un, hipMemcpyDeviceToDevice, h->stream));
      } else dense = cur;
      DrGemmParams<T> q{};
      q.A = base; q.lda = E; q.gidx = dense; q.Lg = 1; q.E = E; q.B = l1_w; q.ldb = 2 * E; q.bias = nullptr; q.zero = zero;
      q.C = H1; q.ldc = E; q.M = Un * n; q.N = E; q.Kd = E;
      if ((rc = dr_launch_gemm<T>(h, q)) != DM_OK) return rc;
      Otm64Attn<T> a{base, H1, G, l2_w, b2, (T)sm_scale64(h), cur, seq, sc, n, stride, L, E, Un, nullptr, 1};
      rows_scored += Un * n;
      if ((rc = otm_pl_launch_attn<T>(h, a)) != DM_OK) return rc;
      const int it = level - level0;
      const bool last = level == leaf_level - 1;
      if ((d_tn && it < max_levels) || last) {
        Otm64Out<T> o{};
        o.codes = cur; o.scores = sc; o.stride = stride; o.n = n; o.U = Un; o.u0 = u0;
        if (last) { o.out_ids = d_ids; o.out_sc64 = d_sc64; o.out_sc32 = d_sc32; o.out_cnt = d_counts; o.out_stride = 2 * beam; }
        if (d_tn && it < max_levels) { o.tr_codes = d_tc; o.tr_sc64 = d_ts64; o.tr_sc32 = d_ts32; o.tr_cnt = d_tn; o.tr_levels = max_levels; o.tr_cap = cap; o.level = it; }
        LAUNCHCHK(h, otm64_emit_kernel<T>, dim3(512), dim3(256), 0, o);
      }
    }
    if (leaf_level <= level0) {     // no level to score: the initial frontier is the answer (scores 0), as in the reference
      Otm64Out<T> o{};
      o.codes = cur; o.scores = sc; o.stride = stride; o.n = n; o.U = Un; o.u0 = u0;
      o.out_ids = d_ids; o.out_sc64 = d_sc64; o.out_sc32 = d_sc32; o.out_cnt = d_counts; o.out_stride = 2 * beam;
      LAUNCHCHK(h, otm64_emit_kernel<T>, dim3(512), dim3(256), 0, o);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));      // the workspace is reused by the next pass
  }
  { const unsigned long long r_ = (unsigned long long)rows_scored; HIPCHK(h, hipMemcpy(&h->d_ctr->rows, &r_, 8, hipMemcpyHostToDevice)); }   // dm_last_scored_rows
  return DM_OK;
}

static int otm64_search_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, int beam, int leaf_level, int32_t *d_ids,
                            double *d_sc64, float *d_sc32, int32_t *d_counts, int max_levels, int cap, int32_t *d_tc,
                            double *d_ts64, float *d_ts32, int32_t *d_tn) {
  if (h->dtype != DM_F64)     // an f32 model comes here with L > DM_MAXL only (dm_otm_beam_search*)
    return otm_pipeline_dev<float>(h, d_seq, U, L, beam, leaf_level, d_ids, d_sc64, d_sc32, d_counts, max_levels, cap, d_tc, d_ts64, d_ts32, d_tn);
  {
    bool done = false;
    const int rc_ = beam64_search_dev(h, d_seq, U, L, beam, leaf_level, d_ids, d_sc64, d_sc32, d_counts, max_levels, cap, d_tc, d_ts64, d_ts32, d_tn, &done);
    if (rc_ != DM_OK || done) return rc_;
  }
  return otm_pipeline_dev<double>(h, d_seq, U, L, beam, leaf_level, d_ids, d_sc64, d_sc32, d_counts, max_levels, cap, d_tc, d_ts64, d_ts32, d_tn);
}

// host-buffer front end shared by dm_otm_beam_search[_trace][_f64]: scores come back as double (sc64) or float (sc32)
static int otm64_search_host(dm_ctx *h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                             int32_t *out_node_ids, double *out_sc64, float *out_sc32, int32_t *out_counts, int max_levels,
                             int32_t *tc, double *ts64, float *ts32, int32_t *tn) {
  int rc = otm_check(h, U, L, beam, leaf_level, "dm_otm_beam_search (fp64)");
  if (rc != DM_OK) return rc;
  if (h->dtype != DM_F64 && (L <= DM_MAXL || out_sc64 || ts64))
    return fail(h, DM_ERR_STATE, "fp64 OTM beam search needs f64 weights (dm_load_weights_din with DM_F64)");
  if (U == 0) return DM_OK;
  if (!seq_codes || !out_node_ids || !out_counts || (!out_sc64 && !out_sc32)) return fail(h, DM_ERR_INVALID, "dm_otm_beam_search (fp64): bad arguments");
  if ((rc = check_table_ids(h, "dm_otm_beam_search", "history code", seq_codes, U * L, -1)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  int cap;
  frontier_caps(beam, &cap, nullptr);
  ReqLayout lay(h, h->req, 2, U, (size_t)L * 4, (size_t)2 * beam, out_sc64 ? 8 : 4);
  if (tn) lay.trace(max_levels, cap, ts64 ? 8 : 4);
  if ((rc = lay.commit(out_node_ids, out_sc64 ? (void *)out_sc64 : (void *)out_sc32, out_counts, tc, ts64 ? (void *)ts64 : (void *)ts32, tn)) != DM_OK) return rc;
  int32_t *d_seq = lay.d<int32_t>(lay.SEQ), *d_ids = lay.d<int32_t>(lay.IDS), *d_cnt = lay.d<int32_t>(lay.COUNTS);
  char *d_sc = lay.d<char>(lay.SCORES), *d_ts = lay.d<char>(lay.TS);
  // small requests: OTM.recommend's one-user-per-call loop, examples/.../otm/package.scala:101-105
  if (lay.fits_stage() && (rc = lay.stage(seq_codes)) != DM_OK) return rc;
  if (lay.staged && h->direct_ok && U <= 8) {
    lay.arm_direct();
    bool done = false;
    void *k_sc = lay.stage_ptr(d_sc);
    rc = beam64_search_dev(h, lay.stage_ptr(d_seq), U, L, beam, leaf_level, lay.stage_ptr(d_ids), out_sc64 ? (double *)k_sc : nullptr,
                           out_sc64 ? nullptr : (float *)k_sc, lay.stage_ptr(d_cnt), 0, cap, nullptr, nullptr, nullptr, nullptr, &done, true);
    if (rc != DM_OK) return rc;
    if (done) return lay.wait_direct("fp64 OTM beam search");
    // the fused kernel did not take it (pipeline fallback): the staged path below
  }
  HIPCHK(h, lay.upload(seq_codes));
  if (tn) HIPCHK(h, lay.clear_trace());
  rc = otm64_search_dev(h, d_seq, U, L, beam, leaf_level, d_ids, out_sc64 ? (double *)d_sc : nullptr, out_sc64 ? nullptr : (float *)d_sc,
                        d_cnt, max_levels, cap, lay.d<int32_t>(lay.TC), ts64 ? (double *)d_ts : nullptr, (tn && !ts64) ? (float *)d_ts : nullptr, lay.d<int32_t>(lay.TN));
  if (rc != DM_OK) return rc;
  HIPCHK(h, lay.finish());
  return DM_OK;
}

int dm_otm_beam_search_f64(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                           int32_t *out_node_ids, double *out_scores, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  return otm64_search_host(h, seq_codes, U, L, beam, leaf_level, out_node_ids, out_scores, nullptr, out_counts, 0, nullptr, nullptr, nullptr, nullptr);
}

int dm_otm_beam_search_trace_f64(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                                 int32_t *out_node_ids, double *out_scores, int32_t *out_counts, int max_levels,
                                 int32_t *trace_codes, double *trace_scores, int32_t *trace_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (max_levels <= 0 || !trace_codes || !trace_scores || !trace_counts) return fail(h, DM_ERR_INVALID, "dm_otm_beam_search_trace_f64: bad trace arguments");
  return otm64_search_host(h, seq_codes, U, L, beam, leaf_level, out_node_ids, out_scores, nullptr, out_counts, max_levels, trace_codes,
                           trace_scores, nullptr, trace_counts);
}
