// Deep-Retrieval beam search, column-sliced (SURVEY.md row A13; CandidateSearcher.beamSearch, deep-retrieval/src/main/scala/com/mass/dr/
// model/CandidateSearcher.scala:22-60; LayerModel.inference, .../model/LayerModel.scala:68-84; softmax, .../package.scala:23-28).
//
// dr_beam_kernel (dr_kernel.hip.inc) gives a user to one workgroup that walks the D layers: per layer and live path it reads 1 + d table
// rows of K values, and two things of nearly equal size bound it (tools/dr_phase_probe.py): the 24 MB of node tables do not fit a 4 MB
// XCD L2, so the 1.2 MB of rows a user reads arrive at the cross-XCD rate (~7 TB/s over the whole chip), and the softmax denominators
// cost one fp64 exp per candidate (100 k per user).  This file takes both on:
//   * the K columns are cut into 8 slices of 128, slice x is processed by the workgroups with blockIdx % 8 == x — observed to run on
//     XCD x (a speed choice only, nothing depends on it) — so an XCD only ever touches columns [128x, 128x + 128) of every table:
//     3 MB, L2-resident, each row segment re-read ~800 times per launch from the local L2;
//   * the denominators are taken against an UPPER BOUND of a path's largest logit, Mhat = max_k S_d[u][k] + sum_t max_k T_{d,t}[n_t][k]
//     (row maxima tabulated at model load), and then FACTORISE:  exp(l - Mhat) = exp(S_d[u][k] - max S) prod_t exp(T_{d,t}[n_t][k] -
//     max T_{d,t}[n_t]).  The table factors are tabulated at model load (ET tables, same shape as T), the history factor costs K exps
//     per user and layer (ES rows, made by the layer-0 kernel) — so a candidate costs two multiplications instead of an exp: 2 000 exps
//     per user instead of 100 000.  prob = exp(l - Mhat) / sum exp(. - Mhat) is the same number as the reference's exp(l - max) / sum
//     exp(. - max) up to the last bits (both scaled by exp(max - Mhat)); the winners' probabilities are still exp() of their logits;
//   * a layer is two launches: drs_stats_kernel — 16 lanes per (user, path, slice), 8 columns per lane, partial sums of the products
//     and their maxima over 32-column blocks — and drs_select_kernel — one workgroup per user: combine the 8 partial sums in slice order, then
//     the cut of dr_beam_layer's fast path (beam-th largest block maximum as a lower bound, exact evaluation of the few candidate
//     blocks, composite-key sort; the exact radix select over everything as the fallback).  Layer 0 (one path, no tables) is
//     dr_beam_layer<T, 0> itself.  State (nodes, path probabilities) passes between the launches through global memory.
// Results: the same paths as dr_beam_kernel (bit-exact against the fp64 oracle in fp64), probabilities equal to rounding.

#ifndef DRS_STATS_WPS
#define DRS_STATS_WPS 4     // workgroups (= waves per SIMD) per CU the statistics kernel is compiled for
#endif
#ifndef DRS_SELW_WPS
#define DRS_SELW_WPS (sizeof(T) == 8 ? 3 : 4)      // ... and the one-wave cut: the fp64 instance spills 120-160 registers at 128 (0.51 -> 0.47 ms per layer at 170), the f32 one
#endif                                             //     is faster at four waves (0.31 against 0.39 ms); the statistics kernel is faster at four in both types
#ifndef DRS_L0W_WPS
#define DRS_L0W_WPS (sizeof(T) == 8 ? 4 : 2)      // workgroups per CU of the one-wave layer-0 kernel (fp64: 0.34 -> 0.27 ms at four; f32 indifferent)
#endif
#define DRS_W 128        // columns per slice
#define DRS_NS 8         // slices (K <= 1024)
#define DRS_BLK 16       // columns per block: 8 blocks per slice, 64 per path — more than the beam (<= 64), so that one dominant path can
                         // supply every block of the cut and the threshold never has to dip into the next path

template <typename T>
struct DrsParams {
  const T *S;                 // [U][D*K]
  const T *tabs[DR_MAXD * (DR_MAXD - 1) / 2];
  const T *rowmax[DR_MAXD * (DR_MAXD - 1) / 2];   // [K] max_k T_{d,t}[node][k]
  const T *etabs[DR_MAXD * (DR_MAXD - 1) / 2];    // ET_{d,t}[node][k] = exp(T_{d,t}[node][k] - rowmax[node])
  T *ES;                      // [U][D*K]: exp(S_d[u][k] - smax[u][d]) for d >= 1 (written by the layer-0 kernel)
  int K, D, beam, n2, nl;
  int64_t U;
  const int32_t *nodes;       // current state [U][beam][D]
  const T *pprob;             // [U][beam]
  const int32_t *np;          // [U]
  int32_t *nodes_n;           // next state (select kernel)
  T *pprob_n;
  int32_t *np_n;
  T *smax;                    // [U][D]: max_k S_d[u][k]
  T *part_s;                  // [U][beam][8]
  T *part_bmax;               // [U][beam][8][8]: block maxima of the products exp(l - Mhat)
  int last;                   // select kernel of the last layer: results go to out_*
  int32_t *out_paths; double *out_probs; int32_t *out_counts;
  unsigned long long *slow_count;
  int32_t *todo;              // [U]: users the one-wave cut hands to the block version (drs_select_kernel with only_todo)
  int only_todo;
};

// max_k of every row of a K x K table (model load)
template <typename T>
__global__ void drs_rowmax_kernel(const T *tab, int K, T *rowmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = blockIdx.x * (blockDim.x >> 6) + wave; r < K; r += gridDim.x * (blockDim.x >> 6)) {
    T m = -INFINITY;
    for (int k = lane; k < K; k += 64) { const T v = tab[(int64_t)r * K + k]; m = v > m ? v : m; }
    for (int o = 32; o > 0; o >>= 1) { const T v = __shfl_xor(m, o); m = v > m ? v : m; }
    if (lane == 0) rowmax[r] = m;
  }
}

// ET[node][k] = exp(T[node][k] - rowmax[node])  (model load; library exp)
template <typename T>
__global__ void drs_exptab_kernel(const T *tab, const T *rowmax, int K, T *etab) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)K * K; i += (int64_t)gridDim.x * blockDim.x)
    etab[i] = DrKey<T>::ex(tab[i] - rowmax[i / K]);
}

// ---- layer 0 + the per-user maxima of the later layers' history logits -------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(DR_NT, (sizeof(T) == 4 ? 4 : 2)) void drs_layer0_kernel(DrBeamParams<T> bp, DrsParams<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem_dr[];
  const DrLds<T> L = dr_beam_carve<T>(smem_dr, bp.K, bp.D, bp.n2, bp.fast != 0, bp.nl);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int srow_n = bp.fast ? 1024 : bp.K;
  unsigned long long dr_tlast = 0;
  for (int64_t u = blockIdx.x; u < p.U; u += gridDim.x) {
    if (p.only_todo && !p.todo[u]) continue;          // uniform
    __syncthreads();
    for (int k = tid; k < srow_n; k += DR_NT) L.Srow[k] = k < p.K ? p.S[u * ((int64_t)p.D * p.K) + k] : (T)0;
    if (tid == 0) L.pprob0[0] = (T)1;                 // initValue: probability = 1.0 (CandidateSearcher.scala:27-34)
    // smax[u][d], d >= 1: one wave per layer row
    for (int d = 1 + wave; d < p.D; d += DR_NW) {
      T m = -INFINITY;
      const T *row = p.S + u * ((int64_t)p.D * p.K) + (int64_t)d * p.K;
      for (int k = lane; k < p.K; k += 64) { const T v = row[k]; m = v > m ? v : m; }
      for (int o = 32; o > 0; o >>= 1) { const T v = __shfl_xor(m, o); m = v > m ? v : m; }
      if (lane == 0) p.smax[u * p.D + d] = m;
      for (int k = lane; k < p.K; k += 64) p.ES[u * ((int64_t)p.D * p.K) + (int64_t)d * p.K + k] = DrKey<T>::ex(row[k] - m);
    }
    __syncthreads();
    int np2 = 0;
    dr_beam_layer<T, 0>(bp, 0, 1, np2, L, L.pprob0, L.pprob1, L.nodes0, L.nodes1, dr_tlast);
    for (int q = tid; q < p.beam; q += DR_NT) {
      if (p.last) {
        for (int t = 0; t < p.D; t++) p.out_paths[(u * p.beam + q) * p.D + t] = q < np2 ? L.nodes1[q * p.D + t] : -1;
        p.out_probs[u * p.beam + q] = q < np2 ? (double)L.pprob1[q] : 0.0;
      } else if (q < np2) {
        for (int t = 0; t < p.D; t++) p.nodes_n[(u * p.beam + q) * p.D + t] = t == 0 ? L.nodes1[q * p.D] : 0;
        p.pprob_n[u * p.beam + q] = L.pprob1[q];
      }
    }
    if (tid == 0) { if (p.last) p.out_counts[u] = np2; else p.np_n[u] = np2; }
  }
}

// ---- layer 0, one WAVE per user (K <= 1024, beam <= 256): the K probabilities live in registers (16 per lane), the beam-th largest
// is bounded from below by bisection on the bits of the float-rounded probabilities (counts on the scalar unit), the survivors
// are rank-sorted through a few hundred bytes of LDS — exact ties by column, the stable sortBy of CandidateSearcher.scala:49-51.  No
// workgroup barrier, no histogram: 16384 users take tens of microseconds instead of 0.66 ms (fp64) of barrier-bound block code.
// Same arithmetic as dr_beam_layer<T, 0>: true maximum, library exp, exp / sum.
template <typename T>
__global__ __launch_bounds__(256, DRS_L0W_WPS) void drs_layer0_wave_kernel(DrsParams<T> p) {
  typedef typename DrKey<T>::K KeyT;
  constexpr int V = 16 / (int)sizeof(T), NLD = 16 / V;     // 16 elements per lane: element e = column (e / V) 64 V + lane V + e % V
  __shared__ KeyT wkey[4][256];
  __shared__ unsigned short wcol[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = p.K, D = p.D;
  auto col = [&](int e) { return (e / V) * 64 * V + lane * V + (e % V); };
  typedef T vec_t __attribute__((ext_vector_type(V)));
  auto wave_sum_i = [&](int c) { for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o); return c; };
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < p.U; u += (int64_t)gridDim.x * 4) {
    const T *srow = p.S + u * ((int64_t)D * K);
    // smax[u][d], d >= 1
    for (int d = 1; d < D; d++) {
      T m = -INFINITY;
      for (int k = lane; k < K; k += 64) { const T v = srow[(int64_t)d * K + k]; m = v > m ? v : m; }
      m = dr_wave_max<T>(m);
      if (lane == 0) p.smax[u * D + d] = m;
      for (int k = lane; k < K; k += 64) p.ES[u * ((int64_t)D * K) + (int64_t)d * K + k] = DrKey<T>::ex(srow[(int64_t)d * K + k] - m);     // the history factor of exp(l - Mhat)
    }
    T lg[16];
#pragma unroll
    for (int c = 0; c < NLD; c++) {
      const int kc = col(c * V) < K ? col(c * V) : 0;
      vec_t v;
      __builtin_memcpy(&v, __builtin_assume_aligned(srow + kc, sizeof(T)), 16);
#pragma unroll
      for (int i = 0; i < V; i++) lg[c * V + i] = col(c * V + i) < K ? v[i] : (T)-INFINITY;
    }
    T m = lg[0];
#pragma unroll
    for (int e = 1; e < 16; e++) m = lg[e] > m ? lg[e] : m;
    m = dr_wave_max<T>(m);
    T s = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) { lg[e] = DrKey<T>::ex(lg[e] - m); s += lg[e]; }     // exp(-inf) = 0 for the missing columns
    s = dr_wave_sum<T>(s);
    KeyT key[16];
#pragma unroll
    for (int e = 0; e < 16; e++) key[e] = col(e) < K ? DrKey<T>::enc((T)1 * (lg[e] / s)) : (KeyT)0;      // initValue 1.0 * prob; 0 = below every real key
    const int ksel = K < p.beam ? K : p.beam;
    // a lower bound of the ksel-th largest probability (as floats rounded toward zero: monotone, so the true top ksel all lie at or
    // above it), the survivors compacted into LDS, and the rank sort below settles the order — exact ties by column, like the stable
    // sortBy of the reference — and keeps the first ksel
    float pf[16];
#pragma unroll
    for (int e = 0; e < 16; e++) { const T pv = col(e) < K ? DrKey<T>::dec(key[e]) : (T)0; pf[e] = sizeof(T) == 8 ? __double2float_rz((double)pv) : (float)pv; }
    unsigned tb0 = 0;
    for (int bit = 30; bit > 6; bit--) {                    // v_cmp + s_bcnt1 per element: the counts live on the scalar unit
      const unsigned cand = tb0 | (1u << bit);
      int c = 0;
#pragma unroll
      for (int e = 0; e < 16; e++) c += __popcll(__ballot(__float_as_uint(pf[e]) >= cand));
      if (c >= ksel) tb0 = cand;
    }
    const float tau_f = __uint_as_float(tb0);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int ns = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const bool keep = col(e) < K && pf[e] >= tau_f;
      const unsigned long long m = __ballot(keep);
      if (keep) { const int sl = ns + __popcll(m & below); if (sl < 256) { wkey[wave][sl] = key[e]; wcol[wave][sl] = (unsigned short)col(e); } }
      ns += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!(tau_f > 0.0f) || ns > 256 || ns < ksel) {         // probabilities spread over > 32 binades, or mass ties: the block version
      if (lane == 0) p.todo[u] = 1;
      continue;
    }
    for (int w = lane; w < ns; w += 64) {
      const KeyT kw = wkey[wave][w];
      const int cw = wcol[wave][w];
      int r = 0;
      for (int o = 0; o < ns; o++) { const KeyT ko = wkey[wave][o]; r += (ko > kw || (ko == kw && (int)wcol[wave][o] < cw)) ? 1 : 0; }
      if (r >= ksel) continue;
      const T pr = DrKey<T>::dec(kw);
      if (p.last) {
        for (int t = 0; t < D; t++) p.out_paths[(u * p.beam + r) * D + t] = t == 0 ? cw : 0;
        p.out_probs[u * p.beam + r] = (double)pr;
      } else {
        for (int t = 0; t < D; t++) p.nodes_n[(u * p.beam + r) * D + t] = t == 0 ? cw : 0;
        p.pprob_n[u * p.beam + r] = pr;
      }
    }
    if (p.last) for (int w = ksel + lane; w < p.beam; w += 64) {
      for (int t = 0; t < D; t++) p.out_paths[(u * p.beam + w) * D + t] = -1;
      p.out_probs[u * p.beam + w] = 0.0;
    }
    if (lane == 0) { if (p.last) p.out_counts[u] = ksel; else p.np_n[u] = ksel; }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- statistics of layer d >= 1: 16 lanes per (user, path, slice) ---------------------------------------------------------------
template <typename T, int NTAB>
__global__ __launch_bounds__(256, DRS_STATS_WPS) void drs_stats_kernel(DrsParams<T> p, int d) {
  const int x = blockIdx.x & (DRS_NS - 1);          // slice; block b is observed on XCD b % 8: the slice's table columns stay in that L2
  const int g = blockIdx.x >> 3, G = gridDim.x >> 3;
  const int row = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int K = p.K, D = p.D;
  __shared__ int32_t nid_lds[16 * 64 * (NTAB > 0 ? NTAB : 1)];
  // Column mapping.  A 16-byte load holds V = 2 doubles / 4 floats; load c of a lane reads bytes [256 c + 16 j, + 16) of the row's
  // 1 KB (fp64) / 512 B (f32) slice segment, so ONE load instruction covers 256 contiguous bytes per (user, path) row — two cache
  // lines — instead of sixteen 16-byte pieces spread over the whole segment (the L1 processes lines, not bytes: 4x fewer per load).
  // Element e of lane j is column  x 128 + (e / V) 16 V + j V + e % V;  a lane pair holds four (two) runs of 32 bytes: one block.
  constexpr int V = 16 / (int)sizeof(T), NLD = 8 / V;
  const int kbase = x * DRS_W + j * V;
  auto col = [&](int e) { return kbase + (e / V) * 16 * V + (e % V); };
  typedef T vec_t __attribute__((ext_vector_type(V)));
  // a load whose first column lies past K reads column 0 instead (its elements are masked): K < 1024 leaves loads, lanes, even slices
  // empty; a load that straddles K runs on into the next row / the slack behind the buffers
  int kc[NLD];
  bool on[8];
#pragma unroll
  for (int c = 0; c < NLD; c++) kc[c] = col(c * V) < K ? col(c * V) : 0;
#pragma unroll
  for (int e = 0; e < 8; e++) on[e] = col(e) < K;
  // A 16-lane row takes a USER and walks the user's paths: the history factors of the slice (ES, the same for every path) are read
  // once and stay in registers — a third to a half of the bytes a per-(user, path) row would read — and only the table rows change.
  // The next path's nodes and table rows are fetched while the current path is reduced.
  const int n_users = (int)p.U;
  for (int u = g * 16 + row; u < n_users; u += G * 16) {
    const int np = p.np[u];
    if (np <= 0) continue;
    const T *srow = p.ES + (int64_t)u * ((int64_t)D * K) + (int64_t)d * K;
    vec_t sv[NLD];
#pragma unroll
    for (int c = 0; c < NLD; c++) __builtin_memcpy(&sv[c], __builtin_assume_aligned(srow + kc[c], sizeof(T)), 16);
    const int32_t *nrow = p.nodes + (int64_t)u * p.beam * D;
    vec_t tv[2][NTAB > 0 ? NTAB : 1][NLD];
    // The paths' node ids are staged in LDS per 16-lane row, 64 paths at a time (lane j fetches paths j, j + 16, j + 32, j + 48 of the
    // chunk).  Round 5 read the ids of path q + 1 from global memory inside the loop: the table-row addresses hung on a 4-byte load
    // issued BEHIND the previous path's row loads, and vmcnt retires in order — every path cost two dependent round trips and drained
    // whatever was in flight.  An LDS read waits on lgkmcnt only: the one load a path waits for is its own table rows, one path ahead.
    int32_t *ids = nid_lds + row * (64 * (NTAB > 0 ? NTAB : 1));
    auto stage_ids = [&](int q0) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int qq = q0 + 16 * k + j;
#pragma unroll
        for (int t = 0; t < NTAB; t++) ids[(16 * k + j) * NTAB + t] = nrow[(qq < np ? qq : np - 1) * D + t];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    stage_ids(0);
    auto load_rows = [&](int q, vec_t (&dst)[NTAB > 0 ? NTAB : 1][NLD]) {
#pragma unroll
      for (int t = 0; t < NTAB; t++) {
        const T *trow = p.etabs[d * (d - 1) / 2 + t] + (int64_t)ids[(q & 63) * NTAB + t] * K;
#pragma unroll
        for (int c = 0; c < NLD; c++) __builtin_memcpy(&dst[t][c], __builtin_assume_aligned(trow + kc[c], sizeof(T)), 16);
      }
    };
    load_rows(0, tv[0]);
    for (int q = 0; q < np; q++) {
      if (q + 1 < np) {
        if (((q + 1) & 63) == 0) stage_ids(q + 1);        // beams beyond 64 paths: the next chunk (the ids of chunk q / 64 are dead: path q's rows are in registers)
        if (q & 1) load_rows(q + 1, tv[0]); else load_rows(q + 1, tv[1]);
      }
      // exp(l - Mhat) of the lane's 8 columns as a product of tabulated factors; their sum and the block's maximum
      T s = 0, bm = 0;
#pragma unroll
      for (int c = 0; c < NLD; c++)
#pragma unroll
        for (int i = 0; i < V; i++) {
          T pr = sv[c][i];
#pragma unroll
          for (int t = 0; t < NTAB; t++) pr *= (q & 1) ? tv[1][t][c][i] : tv[0][t][c][i];
          pr = on[c * V + i] ? pr : (T)0;
          s += pr;
          bm = pr > bm ? pr : bm;
        }
      T v;
      v = dr_dpp<0xB1>(bm); bm = v > bm ? v : bm;       // maximum of the lane pair = of a 16-column block (its 32-byte runs)
      s += dr_dpp<0xB1>(s); s += dr_dpp<0x4E>(s); s += dr_dpp<0x141>(s); s += dr_dpp<0x140>(s);     // sum over the row's 16 lanes
      const int64_t o = ((int64_t)u * p.beam + q) * DRS_NS + x;
      if (j == 0) p.part_s[o] = s;
      if ((j & 1) == 0) p.part_bmax[o * 8 + (j >> 1)] = bm;
    }
  }
}

// ---- the cut of layer d >= 1: one workgroup per user ----------------------------------------------------------------------------
template <typename T>
struct DrsLds {
  typedef typename DrKey<T>::K KeyT;
  unsigned *hist; int *wtot, *cnt; DrSel<KeyT> *st;
  T *mhat, *ps, *cp, *pprob, *bmax;
  KeyT *lhi; unsigned *llo;
  int32_t *nodes, *blist;
};
static size_t drs_select_lds(int esz, int D, int n2, int nl) {
  return DR_BINS * 4 + 64 + 64 + (size_t)n2 * esz * 4 + (size_t)n2 * 64 * esz + (size_t)nl * esz + (size_t)nl * 4 + (size_t)n2 * D * 4 + (size_t)nl * 4 + 64;
}
template <typename T>
__device__ __forceinline__ DrsLds<T> drs_carve(char *base, int D, int n2, int nl) {
  DrsLds<T> l;
  l.hist = (unsigned *)base;
  l.wtot = (int *)(l.hist + DR_BINS);
  l.cnt = l.wtot + 8;
  l.st = (DrSel<typename DrKey<T>::K> *)(l.wtot + 16);
  l.mhat = (T *)((char *)l.st + 64);
  l.ps = l.mhat + n2; l.cp = l.ps + n2; l.pprob = l.cp + n2;
  l.bmax = l.pprob + n2;
  l.lhi = (typename DrKey<T>::K *)(l.bmax + n2 * 64);
  l.nodes = (int32_t *)(l.lhi + nl);
  l.llo = (unsigned *)(l.nodes + n2 * D);
  l.blist = (int32_t *)(l.llo + nl);
  return l;
}

// Relative margin of the cut; smallest score it is trusted at; and the two limits below which the PRODUCTS exp(l - Mhat) are no longer
// trusted.  Mhat is an upper bound, so a path's products can all sit in the underflow range while its scores cp * product (cp = parent
// probability / sum) look perfectly normal — floor_ never sees that.  With tiny = numeric_limits<T>::min(): a product of <= 4 tabulated
// factors, each <= 1, is off by at most 4 tiny absolutely once a factor or a partial product is subnormal or flushed to zero.
//   * pmax_min: a path's sum s has K <= 1024 terms, so |s - true| <= 4096 tiny, and s >= the path's largest product pmax.  For a
//     relative error of rel / 4:  pmax >= 4 * 4096 tiny / rel.
//   * prod_min: a candidate at the cut has the product thr / cp; for a relative error of rel / 8:  thr / cp >= 8 * 4 tiny / rel.
// Together with the rounding of normal products (1e-6 in f32, 1e-15 in fp64) every score at or above the cut is then within rel / 2 of
// the true one, which is what thr = tau (1 - rel) allows for (tau <= (1 + rel / 2) true beam-th, a winner's score >= (1 - rel / 2) of it);
// and a survivor's exp(l - Mhat) >= prod_min is a normal number divided by an accurate sum.  A user-layer with a live path outside
// either limit takes the exact path.  (f32: 1.9e-31 = exp(-70.7), 3.8e-34;  fp64: 3.6e-295 = exp(-677.7), 7.1e-298.)
template <typename T> struct DrsTol;
template <> struct DrsTol<float> {
  static constexpr float rel = 1e-3f, floor_ = 1e-30f;
  static constexpr float pmax_min = 16384.f * std::numeric_limits<float>::min() / rel, prod_min = 32.f * std::numeric_limits<float>::min() / rel;
};
template <> struct DrsTol<double> {
  static constexpr double rel = 1e-9, floor_ = 1e-290;
  static constexpr double pmax_min = 16384. * std::numeric_limits<double>::min() / rel, prod_min = 32. * std::numeric_limits<double>::min() / rel;
};

template <typename T, int NTAB>
__global__ __launch_bounds__(DR_NT, 4) void drs_select_kernel(DrsParams<T> p, int d) {
  typedef typename DrKey<T>::K KeyT;
  extern __shared__ __attribute__((aligned(16))) char smem_dr[];
  const DrsLds<T> L = drs_carve<T>(smem_dr, p.D, p.n2, p.nl);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, D = p.D;
  for (int64_t u = blockIdx.x; u < p.U; u += gridDim.x) {
    if (p.only_todo && !p.todo[u]) continue;          // uniform
    __syncthreads();
    const int np = p.np[u];
    const T *Srow = p.S + u * ((int64_t)D * K) + (int64_t)d * K;
    const T *ESrow = p.ES + u * ((int64_t)D * K) + (int64_t)d * K;
    for (int i = tid; i < np * D; i += DR_NT) L.nodes[i] = p.nodes[u * p.beam * D + i];
    if (tid == 0) { L.cnt[2] = 0; L.cnt[3] = 0; }
    __syncthreads();
    // per path: Mhat, the sum in slice order, c = log(parent prob) - Mhat - log(sum); then every block's log-space maximum
    for (int q = tid; q < np; q += DR_NT) {
      T mh = p.smax[u * D + d];
#pragma unroll
      for (int t = 0; t < NTAB; t++) mh += p.rowmax[d * (d - 1) / 2 + t][L.nodes[q * D + t]];
      const T *ps_ = p.part_s + (u * p.beam + q) * DRS_NS;
      T s = ps_[0];
#pragma unroll
      for (int x = 1; x < DRS_NS; x++) s += ps_[x];
      const T pp = p.pprob[u * p.beam + q];
      L.mhat[q] = mh; L.ps[q] = s; L.pprob[q] = pp;
      L.cp[q] = pp / s;                              // candidate probability ~ cp * exp(l - Mhat): the (linear) score of the cut
      // sum == 0 (every exp underflowed: the bound sits hundreds of units above the logits) or a non-finite sum: this user recomputes
      // its statistics against the true maxima on the exact path
      if (!(s > (T)0) || !(s < (T)INFINITY)) atomicOr(L.cnt + 2, 1);
    }
    __syncthreads();
    const int nb = np * 64;
    for (int b = tid; b < nb; b += DR_NT) {           // a wave holds the 64 blocks of ONE path (nb = 64 np, DR_NT = 4 x 64)
      const T raw = p.part_bmax[u * p.beam * 64 + b];
      L.bmax[b] = raw * L.cp[b >> 6];
      // the path's largest product below DrsTol::pmax_min: its sum has lost terms or bits to underflow, exact path (as for s == 0)
      if (__ballot(raw >= DrsTol<T>::pmax_min) == 0ull && lane == 0) atomicOr(L.cnt + 2, 1);
    }
    __syncthreads();
    const bool degenerate = L.cnt[2] != 0;
    const long long n = (long long)np * K;
    const int ksel = n < p.beam ? (int)n : p.beam;
    bool done = false;
    if (!degenerate) {
      const int kb = nb < p.beam ? nb : p.beam;
      auto bsweep = [&](auto f) {
        for (int b = tid; b < nb; b += DR_NT) f((unsigned)b, DrKey<T>::enc(L.bmax[b]));
      };
      dr_radix_select<KeyT>(bsweep, kb, L.hist, L.wtot, L.st, 2);      // two digits: a lower bound of the kb-th largest block maximum
      // tau: a lower bound of the kb-th largest block maximum, hence of the beam-th largest candidate; the relative margin covers the
      // rounding gap between the product of tabulated factors and the exp() of the winners' logits (<= 1e-15 in fp64, 1e-6 in f32).
      // Scores so small that products may have lost bits to underflow send the user to the exact path.
      const T tau = DrKey<T>::dec(L.st->pre_hi);
      const T thr = tau * ((T)1 - DrsTol<T>::rel);
      if (tid == 0) { L.cnt[0] = 0; L.cnt[1] = 0; }
      // the cut in product space, thr / cp, of some path below DrsTol::prod_min: candidates next to it may have lost bits
      for (int q = tid; q < np; q += DR_NT) if (!(thr >= DrsTol<T>::prod_min * L.cp[q])) atomicOr(L.cnt + 3, 1);
      __syncthreads();
      const bool usable = (tau == tau) && thr >= DrsTol<T>::floor_ && thr < (T)INFINITY && L.cnt[3] == 0;    // uniform
      if (usable) {
        for (int b = tid; b < nb; b += DR_NT)
          if (L.bmax[b] >= thr) { const int sl = atomicAdd(L.cnt + 1, 1); if (sl < p.nl) L.blist[sl] = b; }
        __syncthreads();
        const int nblk = L.cnt[1];
        if (nblk <= p.nl) {
          // (block, element) pairs, two per thread and round
          for (int i0 = tid; i0 < nblk * DRS_BLK; i0 += 2 * DR_NT) {
            int qq[2], kk[2];
            T ll[2];
#pragma unroll
            for (int r = 0; r < 2; r++) {
              const int i = i0 + r * DR_NT;
              const bool on = i < nblk * DRS_BLK;
              const int b = on ? L.blist[i >> 4] : 0;
              // block (slice x, lane pair g) = NLD runs of 2 V consecutive columns (the statistics kernel's lane mapping)
              constexpr int V = 16 / (int)sizeof(T);
              const int blk = b & 63, ei = i & 15;
              qq[r] = b >> 6; kk[r] = on ? (blk >> 3) * DRS_W + (ei / (2 * V)) * 16 * V + (blk & 7) * 2 * V + ei % (2 * V) : K;
              const int kc = kk[r] < K ? kk[r] : 0;
              T pr = ESrow[kc];
#pragma unroll
              for (int t = 0; t < NTAB; t++) pr *= p.etabs[d * (d - 1) / 2 + t][(int64_t)L.nodes[qq[r] * D + t] * K + kc];
              ll[r] = pr * L.cp[qq[r]];
            }
#pragma unroll
            for (int r = 0; r < 2; r++) {
              if (kk[r] >= K) continue;
              const int q = qq[r], k = kk[r];
              if (ll[r] >= thr) {
                T l = Srow[k];                              // a survivor: its logit, and the reference's probability from it
#pragma unroll
                for (int t = 0; t < NTAB; t++) l += p.tabs[d * (d - 1) / 2 + t][(int64_t)L.nodes[q * D + t] * K + k];
                const T pr = DrKey<T>::ex(l - L.mhat[q]) / L.ps[q];     // exps.map(_ / sumExps), both scaled by exp(max - Mhat)
                const int slot = atomicAdd(L.cnt, 1);
                if (slot < p.nl) { L.lhi[slot] = DrKey<T>::enc(L.pprob[q] * pr); L.llo[slot] = ~(unsigned)(q * K + k); }
              }
            }
          }
        } else if (tid == 0) *L.cnt = p.nl + 1;       // too many blocks: exact path
        __syncthreads();
        const int nc = *L.cnt;
        if (nc >= ksel && nc <= p.nl) {
          if (nc <= 2 * DR_NT) {
            dr_rank_sort_desc<KeyT>(L.lhi, L.llo, nc);
          } else {
            int n2c = 1;
            while (n2c < nc) n2c <<= 1;
            for (int i = nc + tid; i < n2c; i += DR_NT) { L.lhi[i] = 0; L.llo[i] = 0; }
            __syncthreads();
            dr_sort_desc<KeyT>(L.lhi, L.llo, n2c);
          }
          done = true;
        }
      }
      __syncthreads();
    }
    if (!done) {
      // exact path: statistics against the TRUE maxima (one wave per path, online), then the radix select over every candidate
      for (int q = wave; q < np; q += DR_NW) {
        const T *rp[NTAB > 0 ? NTAB : 1];
#pragma unroll
        for (int t = 0; t < NTAB; t++) rp[t] = p.tabs[d * (d - 1) / 2 + t] + (int64_t)L.nodes[q * D + t] * K;
        T m = -INFINITY, s = 0;
        for (int k = lane; k < K; k += 64) {
          T l = Srow[k];
#pragma unroll
          for (int t = 0; t < NTAB; t++) l += rp[t][k];
          if (l > m) { s = s * DrKey<T>::ex(m - l); m = l; }
          s += DrKey<T>::ex(l - m);
        }
        T mm = m;
        for (int o = 32; o > 0; o >>= 1) { const T v = __shfl_xor(mm, o); mm = v > mm ? v : mm; }
        s = (m == mm) ? s : s * DrKey<T>::ex(m - mm);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) { L.mhat[q] = mm; L.ps[q] = s; }
      }
      __syncthreads();
      auto sweep = [&](auto f) {
        for (int q = wave; q < np; q += DR_NW) {
          const T *rp[NTAB > 0 ? NTAB : 1];
#pragma unroll
          for (int t = 0; t < NTAB; t++) rp[t] = p.tabs[d * (d - 1) / 2 + t] + (int64_t)L.nodes[q * D + t] * K;
          const T m = L.mhat[q], s = L.ps[q], pp = L.pprob[q];
          for (int k = lane; k < K; k += 64) {
            T l = Srow[k];
#pragma unroll
            for (int t = 0; t < NTAB; t++) l += rp[t][k];
            const T pr = DrKey<T>::ex(l - m) / s;
            f((unsigned)(q * K + k), DrKey<T>::enc(pp * pr));       // pi.probability * prob  (CandidateSearcher.scala:45)
          }
        }
      };
      // lhi / llo hold nl >= n2 slots
      dr_topk<KeyT>(sweep, ksel, p.n2, L.hist, L.wtot, L.st, L.cnt, L.lhi, L.llo);
      if (tid == 0 && p.slow_count) atomicAdd(p.slow_count, 1ull);
    }
    // CandidateSearcher.scala:52-57: the winners become the next layer's paths (or the result)
    for (int qn = tid; qn < p.beam; qn += DR_NT) {
      const bool live = qn < ksel;
      int par = 0, node = 0;
      if (live) {
        const unsigned idx = ~L.llo[qn];
        par = (int)(idx / (unsigned)K); node = (int)(idx - (unsigned)par * (unsigned)K);
      }
      if (p.last) {
        for (int t = 0; t < D; t++) p.out_paths[(u * p.beam + qn) * D + t] = live ? (t < d ? L.nodes[par * D + t] : (t == d ? node : 0)) : -1;
        p.out_probs[u * p.beam + qn] = live ? (double)DrKey<T>::dec(L.lhi[qn]) : 0.0;
      } else if (live) {
        for (int t = 0; t < D; t++) p.nodes_n[(u * p.beam + qn) * D + t] = t < d ? L.nodes[par * D + t] : (t == d ? node : 0);
        p.pprob_n[u * p.beam + qn] = DrKey<T>::dec(L.lhi[qn]);
      }
    }
    if (tid == 0) { if (p.last) p.out_counts[u] = ksel; else p.np_n[u] = ksel; }
  }
}

// ---- the cut of layer d >= 1, one WAVE per user (beam <= 64: the 64 np <= 4096 block scores live in registers as floats) ---------
// The same cut as drs_select_kernel without a single workgroup barrier or LDS atomic: the lower bound tau of the beam-th largest
// block score by bisection on the leading 24 bits of the (positive, float-rounded) scores — one wave-wide count per bit —, candidate blocks and
// surviving elements compacted with ballots, the winners rank-sorted.  Twenty waves per CU each carry their own user; the block
// version's 0.8 ms per layer was barrier and atomic latency (120 k cycles per user and workgroup).  Users whose lists overflow, whose
// scores sit in the underflow range, whose sums degenerated or whose products sit below the limits of DrsTol are flagged in todo[] and
// redone by drs_select_kernel.  Reason bytes of dm_debug_dr_wave_fallbacks: 1 sum zero / non-finite, 2 score floor, 3 too many blocks,
// 4 too few survivors, 5 too many survivors, 6 products in the underflow range (pmax_min, prod_min).
__host__ __device__ static inline size_t drs_selw_lds_per_wave(int esz, int D, int n2, int nl) {
  return (size_t)n2 * esz * 4 + (size_t)n2 * D * 4 + (size_t)nl * (esz + 4) + (size_t)nl * 4 + 32;
}

template <typename T, int NTAB>
__global__ __launch_bounds__(256, DRS_SELW_WPS) void drs_select_wave_kernel(DrsParams<T> p, int d) {
  typedef typename DrKey<T>::K KeyT;
  extern __shared__ __attribute__((aligned(16))) char smem_dr[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = p.K, D = p.D, n2 = p.n2, nl = p.nl;
  char *wb = smem_dr + (size_t)wave * ((drs_selw_lds_per_wave((int)sizeof(T), D, n2, nl) + 15) & ~(size_t)15);
  T *Lmhat = (T *)wb, *Lps = Lmhat + n2, *Lcp = Lps + n2, *Lpp = Lcp + n2;
  KeyT *Lhi = (KeyT *)(Lpp + n2);
  int32_t *Lnodes = (int32_t *)(Lhi + nl);
  unsigned *Llo = (unsigned *)(Lnodes + n2 * D);
  int32_t *Lblist = (int32_t *)(Llo + nl);
  constexpr int V = 16 / (int)sizeof(T);
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  auto wave_sum_i = [&](int c) { for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o); return c; };
  auto lds_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < p.U; u += (int64_t)gridDim.x * 4) {
    const int np = p.np[u];
    const T *Srow = p.S + u * ((int64_t)D * K) + (int64_t)d * K;
    const T *ESrow = p.ES + u * ((int64_t)D * K) + (int64_t)d * K;
    lds_sync();
    for (int i = lane; i < np * D; i += 64) Lnodes[i] = p.nodes[u * p.beam * D + i];
    bool bad = false;
    for (int q = lane; q < np; q += 64) {
      T mh = p.smax[u * D + d];
#pragma unroll
      for (int t = 0; t < NTAB; t++) mh += p.rowmax[d * (d - 1) / 2 + t][p.nodes[(u * p.beam + q) * D + t]];
      const T *ps_ = p.part_s + (u * p.beam + q) * DRS_NS;
      T s = ps_[0];
#pragma unroll
      for (int x = 1; x < DRS_NS; x++) s += ps_[x];
      const T pp = p.pprob[u * p.beam + q];
      Lmhat[q] = mh; Lps[q] = s; Lpp[q] = pp; Lcp[q] = pp / s;
      if (!(s > (T)0) || !(s < (T)INFINITY)) bad = true;
    }
    lds_sync();
    const int nb = np * 64;
    const long long n = (long long)np * K;
    const int ksel = n < p.beam ? (int)n : p.beam;
    const int kb = nb < p.beam ? nb : p.beam;
    // block scores: lane holds blocks lane + 64 i, i.e. block `lane` of path i — as FLOATS rounded toward zero (64 registers; the
    // cut needs a lower bound of the kb-th largest score and a superset of the blocks above it, not the scores themselves)
    float sc[64];
    bool thin = false;                                  // (uniform) a path whose largest product is below DrsTol::pmax_min: its sum is not trusted
#pragma unroll
    for (int i = 0; i < 64; i++) {
      const T raw = i < np ? p.part_bmax[(u * p.beam + i) * 64 + lane] : (T)0;
      const T v = i < np ? raw * Lcp[i] : (T)0;
      if (!(v >= (T)0)) bad = true;                     // NaN
      if (i < np && __ballot(raw >= DrsTol<T>::pmax_min) == 0ull) thin = true;
      sc[i] = sizeof(T) == 8 ? __double2float_rz((double)v) : (float)v;
    }
    bool fallback = __ballot(bad) != 0ull || thin;
    int nc = 0, why = __ballot(bad) != 0ull ? 1 : (thin ? 6 : 0);
    if (!fallback) {
      // bisection on the float bits (sign 0; exponent and 16 mantissa bits: tau within 2^-16 below the kb-th largest).  The count of a
      // candidate is 64 compares whose lane masks are popcounted on the SCALAR unit (v_cmp + s_bcnt1): no per-lane adds, no wave reduction
      unsigned tb = 0;
      for (int bit = 30; bit > 6; bit--) {
        const unsigned cand = tb | (1u << bit);
        int c = 0;
#pragma unroll
        for (int i = 0; i < 64; i++) c += __popcll(__ballot(__float_as_uint(sc[i]) >= cand));
        if (c >= kb) tb = cand;
      }
      const T tau = (T)__uint_as_float(tb);
      const T thr = tau * ((T)1 - DrsTol<T>::rel);
      // blocks whose (exact) score reaches thr: the float is at most one ulp below the score
      const float thr_f = (float)((double)thr * (1.0 - 1.2e-7));
      if (!(thr >= DrsTol<T>::floor_) || !(thr < (T)INFINITY) || !(tau >= (T)1e-30)) { fallback = true; why = 2; }         // uniform
      // the cut in product space, thr / cp, of some path below DrsTol::prod_min (np <= 64: one path per lane)
      else if (__ballot(lane < np && !(thr >= DrsTol<T>::prod_min * Lcp[lane < np ? lane : 0])) != 0ull) { fallback = true; why = 6; }
      if (!fallback) {
        int nblk = 0;
#pragma unroll
        for (int i = 0; i < 64; i++) {
          const bool in = sc[i] >= thr_f && i < np;
          const unsigned long long m = __ballot(in);
          if (in) { const int sl = nblk + __popcll(m & below); if (sl < nl) Lblist[sl] = i * 64 + lane; }
          nblk += __popcll(m);
        }
        lds_sync();
        if (nblk > nl) { fallback = true; why = 3; }
        else {
          // Each lane takes ONE candidate block and walks its 16 elements (NLD runs of 32 bytes per source row: independent 16-byte
          // loads, issued back to back — a wave walking (block, element) pairs in lock step would pay one memory round trip per 64
          // pairs).  Survivors of the cut are compacted by ballots into Llo (as ~index); a second pass gives each survivor a lane
          // for its logit and the reference's probability.
          constexpr int NLD = 8 / V;
          typedef T vec_t __attribute__((ext_vector_type(V)));
          int ns = 0;
          for (int w0 = 0; w0 < nblk; w0 += 64) {
            const bool on = w0 + lane < nblk;
            const int b = on ? Lblist[w0 + lane] : 0;
            const int q = b >> 6, blk = b & 63;
            const T cq = Lcp[q];
            T pr[16];
#pragma unroll
            for (int c = 0; c < NLD; c++) {
              const int kr = (blk >> 3) * DRS_W + c * 16 * V + (blk & 7) * 2 * V;      // a run of 2 V columns
#pragma unroll
              for (int v2 = 0; v2 < 2; v2++) {
                vec_t x;
                __builtin_memcpy(&x, __builtin_assume_aligned(ESrow + kr + v2 * V, sizeof(T)), 16);
#pragma unroll
                for (int i = 0; i < V; i++) pr[c * 2 * V + v2 * V + i] = x[i];
              }
            }
#pragma unroll
            for (int t = 0; t < NTAB; t++) {
              const T *er = p.etabs[d * (d - 1) / 2 + t] + (int64_t)Lnodes[q * D + t] * K;
#pragma unroll
              for (int c = 0; c < NLD; c++) {
                const int kr = (blk >> 3) * DRS_W + c * 16 * V + (blk & 7) * 2 * V;
#pragma unroll
                for (int v2 = 0; v2 < 2; v2++) {
                  vec_t x;
                  __builtin_memcpy(&x, __builtin_assume_aligned(er + kr + v2 * V, sizeof(T)), 16);
#pragma unroll
                  for (int i = 0; i < V; i++) pr[c * 2 * V + v2 * V + i] *= x[i];
                }
              }
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
              const int k = (blk >> 3) * DRS_W + (e / (2 * V)) * 16 * V + (blk & 7) * 2 * V + e % (2 * V);
              const bool keep = on && k < K && pr[e] * cq >= thr;
              const unsigned long long m = __ballot(keep);
              if (keep) { const int sl = ns + __popcll(m & below); if (sl < nl) Llo[sl] = ~(unsigned)(q * K + k); }
              ns += __popcll(m);
            }
          }
          lds_sync();
          nc = ns;
          for (int w = lane; w < ns && w < nl; w += 64) {
            const unsigned idx = ~Llo[w];
            const int q = (int)(idx / (unsigned)K), k = (int)(idx - (unsigned)q * (unsigned)K);
            T l = Srow[k];                                  // a survivor: its logit, and the reference's probability from it
#pragma unroll
            for (int t = 0; t < NTAB; t++) l += p.tabs[d * (d - 1) / 2 + t][(int64_t)Lnodes[q * D + t] * K + k];
            Lhi[w] = DrKey<T>::enc(Lpp[q] * (DrKey<T>::ex(l - Lmhat[q]) / Lps[q]));     // pi.probability * (exp / sumExps)
          }
          lds_sync();
          if (nc < ksel || nc > nl) { fallback = true; why = nc < ksel ? 4 : 5; }
        }
      }
    }
    if (fallback) {
      if (lane == 0) { p.todo[u] = 1; if (p.slow_count) { atomicAdd(p.slow_count + 3, 1ull); atomicAdd(p.slow_count + 4, 1ull << (8 * why)); } }      // (SearchCounters::dr_wave_count, dr_wave_reasons: dm_debug_dr_wave_fallbacks)
      continue;
    }
    // rank sort of the nc candidates by (probability key, lower index first); the first ksel are the new paths (CandidateSearcher.scala:49-57)
    for (int w = lane; w < nc; w += 64) {
      const KeyT hw = Lhi[w];
      const unsigned lw = Llo[w];
      int r = 0;
      for (int o = 0; o < nc; o++) { const KeyT ho = Lhi[o]; const unsigned lo_ = Llo[o]; r += (ho > hw || (ho == hw && lo_ > lw)) ? 1 : 0; }
      if (r < ksel) {
        const unsigned idx = ~lw;
        const int par = (int)(idx / (unsigned)K), node = (int)(idx - (unsigned)par * (unsigned)K);
        const T pr = DrKey<T>::dec(hw);
        if (p.last) {
          for (int t = 0; t < D; t++) p.out_paths[(u * p.beam + r) * D + t] = t < d ? Lnodes[par * D + t] : (t == d ? node : 0);
          p.out_probs[u * p.beam + r] = (double)pr;
        } else {
          for (int t = 0; t < D; t++) p.nodes_n[(u * p.beam + r) * D + t] = t < d ? Lnodes[par * D + t] : (t == d ? node : 0);
          p.pprob_n[u * p.beam + r] = pr;
        }
      }
    }
    if (p.last) for (int w = ksel + lane; w < p.beam; w += 64) {
      for (int t = 0; t < D; t++) p.out_paths[(u * p.beam + w) * D + t] = -1;
      p.out_probs[u * p.beam + w] = 0.0;
    }
    if (lane == 0) { if (p.last) p.out_counts[u] = ksel; else p.np_n[u] = ksel; }
  }
}
