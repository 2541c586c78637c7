// Deep-Retrieval M-step, the greedy penalised path assignment on the device (DESIGN.md §23): the coordinate-descent loop of
// CoordinateDescent.optimize (deep-retrieval/.../optim/CoordinateDescent.scala:48-82) over the per-item CSR that dr_mstep.hip.inc and
// dr_mstep_stream.hip.inc hand out.  The loop is sequential over the hit items (one shared path-size table), so the chain is ONE wave;
// everything around it is parallel: dense path indices (a stable sort of the codes, heads, ranks), the hit list, the validation, the random
// paths of the items that never occur as a target, the decode of the chosen positions.
//
// Order contract: iterations t = 1 .. T, hit items in ascending id, rounds j = J - 1 .. 0; a round's gain is
//   g = nv * (log1p(prob + partial) - log1p(partial)) - penalty_factor * ((s + 1)^p / p - s^p / p)
// in fp64, every operation rounded on its own (contract(off)), the integer power by repeated multiplication in a fixed order; the largest
// gain wins, among equal gains the lowest candidate position.  No floating-point atomics: the sizes are integers and one wave owns them.

#define DRA_CMAX 2048                // candidates of one hit item at most: 32 register slots per lane
#define DRA_NB 64                    // hit items of one staged batch at most (one lane plans one item)
#define DRA_CAPE_MIN 1024            // entries of one staging buffer at least (and never fewer than the longest list)
#define DRA_RETRY 64                 // draws per random node before the bounded retry gives up
enum { DRA_BAD_OFFSETS = 1, DRA_BAD_COUNT = 2, DRA_BAD_CODE = 3, DRA_BAD_SCORE = 4, DRA_BAD_DUP = 5 };
// the status block, unsigned 64-bit words
enum { DRA_ST_PATHS = 0, DRA_ST_HITS = 1, DRA_ST_BAD = 2, DRA_ST_STOP = 3, DRA_ST_ITEM = 4, DRA_ST_ITER = 5, DRA_ST_ROUND = 6, DRA_ST_MAXCNT = 7 };

// ---- validation: one thread per item.  The first offending item wins (an integer minimum over (item, kind)); the flags of the hit list and
// the longest list of a hit item ride along
__global__ __launch_bounds__(256) void dra_check_kernel(const long long *off, const long long *codes, const double *scores, const long long *occ, int64_t num_item, int64_t total,
                                                        long long space, int J, uint8_t *hit_flag, unsigned long long *status) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < num_item; v += (int64_t)gridDim.x * blockDim.x) {
    const long long a = off[v], b = off[v + 1];
    const bool hit = occ[v] > 0;
    hit_flag[v] = hit ? 1 : 0;
    int bad = 0;
    if (a < 0 || b < a || b > total || (v == 0 && a != 0) || (v == num_item - 1 && b != total)) bad = DRA_BAD_OFFSETS;
    else {
      if (hit && (b - a < J || b - a > DRA_CMAX)) bad = DRA_BAD_COUNT;
      for (long long e = a; e < b && !bad; e++) {
        const long long c = codes[e];
        const double s = scores[e];
        if (c < 0 || c >= space) bad = DRA_BAD_CODE;
        else if (!(s >= 0.0 && s <= 1.7976931348623157e308)) bad = DRA_BAD_SCORE;
      }
      if (hit && !bad) atomicMax(&status[DRA_ST_MAXCNT], (unsigned long long)(b - a));
    }
    if (bad) atomicMin(&status[DRA_ST_BAD], ((unsigned long long)v << 3) | (unsigned long long)bad);
  }
}
// ---- dense path indices: (code, entry) pairs, sorted by code (stable: equal codes in ascending entry)
__global__ __launch_bounds__(256) void dra_keys_kernel(const long long *codes, int64_t m, unsigned long long *keys, int32_t *vals) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
    keys[e] = (unsigned long long)codes[e];
    vals[e] = (int32_t)e;
  }
}
// sorted position j: its rank among the heads is the entry's dense index; a head leaves its code.  A code that follows itself inside one
// hit item's range is that item's duplicate (equal codes ascend with the entry, so both lie in [off[v], off[v + 1]) of the first one's item)
__global__ __launch_bounds__(256) void dra_pidx_kernel(const unsigned long long *ks, const int32_t *vs, const uint8_t *flag, const int32_t *head, const unsigned long long *n_head,
                                                       int64_t m, const long long *off, const long long *occ, int64_t num_item, int32_t *pidx, long long *pcodes,
                                                       unsigned long long *status) {
  const int64_t P = (int64_t)*n_head;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = P;                               // the first head behind j
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)head[mid] <= j) lo = mid + 1; else hi = mid;
    }
    const int64_t r = lo > 0 ? lo - 1 : 0;
    pidx[vs[j]] = (int32_t)r;
    if (flag[j]) pcodes[r] = (long long)ks[j];
    else {
      const long long e1 = vs[j - 1], e2 = vs[j];
      int64_t a = 0, b = num_item;                        // the last item whose range starts at or before e1
      while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (off[mid] <= e1) a = mid + 1; else b = mid;
      }
      const int64_t v = a > 0 ? a - 1 : 0;
      if (off[v + 1] > e2 && occ[v] > 0) atomicMin(&status[DRA_ST_BAD], ((unsigned long long)v << 3) | (unsigned long long)DRA_BAD_DUP);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the chain
struct DraChainParams {
  const long long *off, *occ; const double *scores; const int32_t *pidx, *hit;
  int64_t n_hit; int J, pw, t, cape; double pf;           // t: this launch's iteration, from 1
  int32_t *size, *last; unsigned long long *status;
  int32_t *trace_sel; double *trace_gain;                 // [T][n_hit][J] or null
};
// One staging buffer in LDS: the candidates of up to DRA_NB consecutive hit items, `cape` entries in all, and what the executor needs to
// know of each item.  Two of them alternate (the ring): the executor reads one while the other waves fill the next
struct DraBuf { double *sc; int32_t *px, *la, *m_start, *m_cnt, *m_item; double *m_nv; int32_t *m_n; };
__host__ __device__ static inline size_t dra_buf_bytes(int cape) { return (size_t)cape * 16 + DRA_NB * 4 * 3 + DRA_NB * 8 + 16; }
__device__ __forceinline__ DraBuf dra_buf(char *base, int cape) {
  DraBuf b;
  b.sc = (double *)base; b.px = (int32_t *)(base + (size_t)cape * 8); b.la = b.px + cape;
  b.m_start = b.la + cape; b.m_cnt = b.m_start + DRA_NB; b.m_item = b.m_cnt + DRA_NB;
  b.m_nv = (double *)(b.m_item + DRA_NB); b.m_n = (int32_t *)(b.m_nv + DRA_NB);
  return b;
}
// waves wrel = 0 .. nw - 1 stage the batch that starts at hit item g0: as many of the next DRA_NB items as fit in `cape` entries (at least
// one: no list is longer than cape), their (pidx, score), and for t > 1 the positions the previous iteration chose.  Every wave computes the
// same plan from the same loads; wave 0 of the set writes it down
__device__ __forceinline__ void dra_stage(const DraChainParams &p, const DraBuf &B, int64_t g0, int wrel, int nw, int lane) {
  const int64_t g = g0 + lane;
  long long a = 0; int cnt = 0, item = 0; double nv = 0.0;
  if (g < p.n_hit) { item = p.hit[g]; a = p.off[item]; cnt = (int)(p.off[item + 1] - a); nv = (double)p.occ[item]; }
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  const int n = __popcll(__ballot(g < p.n_hit && inc <= p.cape));      // (a prefix of the lanes: inc does not decrease)
  const int start = inc - cnt;
  if (wrel == 0) {
    B.m_start[lane] = start; B.m_cnt[lane] = cnt; B.m_item[lane] = item; B.m_nv[lane] = nv;
    if (lane == 0) *B.m_n = n;
  }
  for (int k = 0; k < n; k++) {
    const long long ak = __shfl(a, k);
    const int ck = __shfl(cnt, k), sk = __shfl(start, k);
    for (int c = wrel * 64 + lane; c < ck; c += nw * 64) { B.sc[sk + c] = p.scores[ak + c]; B.px[sk + c] = p.pidx[ak + c]; }
    if (p.t > 1)
      for (int j = wrel * 64 + lane; j < p.J; j += nw * 64) B.la[sk + j] = p.last[(g0 + k) * p.J + j];      // (J <= the item's entries)
  }
}
__device__ __forceinline__ double dra_ipow(double x, int pw) { double r = x; for (int i = 1; i < pw; i++) r *= x; return r; }

// The executor: one wave, one staged batch.  Lane l holds candidates l, l + 64, ... of the current item in registers (score, dense index,
// size); the J rounds run there.  -> false when the chain stopped (the status block says where)
template <int NS>
__device__ __forceinline__ bool dra_exec_batch(const DraChainParams &p, const DraBuf &B, int32_t *chg, int64_t g0, int lane) {
#pragma clang fp contract(off)   // plain operators, each product and each difference rounded on its own, as the host route computes them
  const int n = *B.m_n;
  const double pd = (double)p.pw, ninf = -__longlong_as_double(0x7ff0000000000000ll);
  int32_t npx[NS], nsz[NS];
  {                                                        // the batch's first item: the one size load per batch that is waited for
    const int start = B.m_start[0], cnt = B.m_cnt[0];
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int c = s * 64 + lane;
      npx[s] = c < cnt ? B.px[start + c] : 0;
      nsz[s] = c < cnt ? p.size[npx[s]] : 0;
    }
  }
  for (int k = 0; k < n; k++) {
    const int start = B.m_start[k], cnt = B.m_cnt[k];
    const double nv = B.m_nv[k];
    const int64_t g = g0 + k;
    double sc[NS]; int32_t px[NS], sz[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int c = s * 64 + lane;
      px[s] = npx[s]; sz[s] = nsz[s];
      sc[s] = c < cnt ? B.sc[start + c] : 0.0;
    }
    // The sizes of item k + 1 are asked for NOW and used after item k.  Only this wave writes `size` while the kernel runs, its memory
    // operations reach the one L1 of its CU in the order it issued them, and its stores for items .. k - 1 were issued before these loads:
    // what the loads can miss is exactly what item k itself changes, at most 2 J words by +-1, and those changes are kept (chg) and
    // applied to the loaded values below.  Nobody else can have written the words between the loads' issue and their use.
    const bool more = k + 1 < n;
    const int nstart = more ? B.m_start[k + 1] : 0, ncnt = more ? B.m_cnt[k + 1] : 0;
#pragma unroll
    for (int s = 0; s < NS; s++)
      if (s * 64 < ncnt) {
        const int c = s * 64 + lane;
        npx[s] = c < ncnt ? B.px[nstart + c] : -1;
        nsz[s] = c < ncnt ? p.size[npx[s]] : 0;
      }
    unsigned sel = 0, touched = 0;
    int nchg = 0;                                          // (chg: plain LDS words, written by one lane each, read by all behind the fence below)
    double partial = 0.0;
    for (int j = p.J - 1; j >= 0; j--) {
      bool stop = !(partial > -1.0);                       // log1p(partial) has no value: the host route raises here
      double wg = 0.0; int wc = 0x7fffffff;
      if (!stop) {
        if (p.t > 1) {                                     // the path this slot held after the previous iteration gives its place back
          const int lp = B.la[start + j];
          if (lane == (lp & 63)) {
#pragma unroll
            for (int s = 0; s < NS; s++)
              if (s == (lp >> 6)) { sz[s]--; touched |= 1u << s; chg[nchg] = (px[s] << 1) | 1; }
          }
          nchg++;
        }
        const double l1p = log1p(partial);
        double bg = ninf; int bc = 0x7fffffff;
#pragma unroll
        for (int s = 0; s < NS; s++)
          if (s * 64 < cnt) {
            const int c = s * 64 + lane;
            if (c < cnt && !((sel >> s) & 1u)) {
              const double sd = (double)sz[s];
              const double pen = p.pf * (dra_ipow(sd + 1.0, p.pw) / pd - dra_ipow(sd, p.pw) / pd);
              const double gn = nv * (log1p(sc[s] + partial) - l1p) - pen;
              if (gn > bg) { bg = gn; bc = c; }            // (ascending position inside a lane: the first maximum stays)
            }
          }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double og = __shfl_xor(bg, o);
          const int oc = __shfl_xor(bc, o);
          if (og > bg || (og == bg && oc < bc)) { bg = og; bc = oc; }
        }
        wg = bg; wc = bc;
        stop = wc == 0x7fffffff || !(wg >= -1.7976931348623157e308 && wg <= 1.7976931348623157e308);
      }
      if (stop) {
        if (lane == 0) {
          p.status[DRA_ST_ITEM] = (unsigned long long)B.m_item[k]; p.status[DRA_ST_ITER] = (unsigned long long)p.t;
          p.status[DRA_ST_ROUND] = (unsigned long long)j; p.status[DRA_ST_STOP] = 1ull;
        }
        return false;
      }
      if (lane == (wc & 63)) {
#pragma unroll
        for (int s = 0; s < NS; s++)
          if (s == (wc >> 6)) { sz[s]++; sel |= 1u << s; touched |= 1u << s; chg[nchg] = px[s] << 1; }
      }
      nchg++;
      partial = partial + wg;                              // the GAIN is accumulated (CoordinateDescent.scala:76)
      if (lane == 0) {
        p.last[g * p.J + j] = wc;
        if (p.trace_sel) {
          const int64_t at = ((int64_t)(p.t - 1) * p.n_hit + g) * p.J + j;
          p.trace_sel[at] = wc; p.trace_gain[at] = wg;
        }
      }
    }
    // the net changes: every touched word once, its final value
#pragma unroll
    for (int s = 0; s < NS; s++)
      if ((touched >> s) & 1u) p.size[px[s]] = sz[s];
    if (more) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int q = 0; q < nchg; q++) {
        const int e = chg[q];
        const int idx = e >> 1, d = (e & 1) ? -1 : 1;
#pragma unroll
        for (int s = 0; s < NS; s++)
          if (s * 64 < ncnt && npx[s] == idx) nsz[s] += d;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  return true;
}

// One iteration over the hit items, one workgroup: wave 0 executes, waves 1 .. 3 stage the next batch into the other buffer of the ring, so
// the executor finds (pidx, score, nv, last) in LDS and never waits for an index load in front of a gather.  A workgroup barrier per batch
// hands the buffers over; a stop is a flag in LDS that every wave reads behind the same barrier.
template <int NS>
__global__ __launch_bounds__(256) void dra_chain_kernel(DraChainParams p) {
  extern __shared__ __attribute__((aligned(16))) char dra_sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t bb = dra_buf_bytes(p.cape);
  const DraBuf B0 = dra_buf(dra_sm, p.cape), B1 = dra_buf(dra_sm + bb, p.cape);
  int32_t *chg = (int32_t *)(dra_sm + 2 * bb);
  int32_t *s_stop = chg + 2 * p.J;
  if (p.status[DRA_ST_STOP]) return;                      // an earlier iteration stopped: its launch order stands, its work does not
  if (threadIdx.x == 0) *s_stop = 0;
  dra_stage(p, B0, 0, wave, 4, lane);
  __syncthreads();
  int64_t g0 = 0;
  for (int b = 0; g0 < p.n_hit; b ^= 1) {
    const DraBuf &cur = b ? B1 : B0, &nxt = b ? B0 : B1;
    const int n = *cur.m_n;
    if (n <= 0) break;                                     // (cannot happen: no list is longer than a buffer)
    if (wave == 0) {
      if (!dra_exec_batch<NS>(p, cur, chg, g0, lane) && lane == 0) *s_stop = 1;
    } else if (g0 + n < p.n_hit) {
      dra_stage(p, nxt, g0 + n, wave - 1, 3, lane);
    }
    __syncthreads();
    if (*s_stop) break;
    g0 += n;
  }
}

// hit item g, slot j: the code at the position the last iteration chose
__global__ __launch_bounds__(256) void dra_emit_kernel(const int32_t *hit, const long long *off, const long long *codes, const int32_t *last, int64_t n_hit, int J, long long *out) {
  const int64_t n = n_hit * J;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = i / J;
    const int64_t v = hit[g];
    out[v * J + (i - g * J)] = codes[off[v] + last[i]];
  }
}

// ---- random paths of the items that never occur as a target: node d of path j of item v is uniform in [0, K), from the sampler's
// counter-based splitmix64 keyed by (seed, v, j, d); a draw at or above the largest multiple of K is drawn again (counter + 1), DRA_RETRY
// times at most, so no node is favoured by a modulo
__device__ __forceinline__ unsigned long long dra_random_node(unsigned long long seed, int64_t v, int j, int d, unsigned long long K) {
  const unsigned long long key = dm_dev_splitmix(dm_dev_splitmix(seed ^ dm_dev_splitmix((unsigned long long)v)) ^ (((unsigned long long)j << 8) | (unsigned long long)d));
  const unsigned long long lim = ~0ull - (~0ull % K + 1ull) % K;       // the last value of the last whole block of K
  unsigned long long r = 0;
  for (unsigned long long ctr = 0; ctr < DRA_RETRY; ctr++) {
    r = dm_dev_splitmix(key ^ (ctr * 0xD6E8FEB86659FD93ull));
    if (r <= lim) break;
  }
  return r % K;
}
__global__ __launch_bounds__(256) void dra_random_kernel(const long long *occ, int64_t num_item, int J, int K, int D, unsigned long long seed, long long *out) {
  const int64_t n = num_item * J;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / J;
    if (occ[v] > 0) continue;
    const int j = (int)(i - v * J);
    unsigned long long code = 0;
    for (int d = 0; d < D; d++) code = code * (unsigned long long)K + dra_random_node(seed, v, j, d, (unsigned long long)K);
    out[i] = (long long)code;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct DraArgs { int64_t num_item, total; int K, D, J, T, pw; double pf; unsigned long long seed; };
struct DraResult { const long long *pcodes = nullptr; const int32_t *sizes = nullptr; int64_t P = 0, n_hit = 0; };

// every refusal that needs neither the arrays' contents nor memory; *space = num_node^num_layer
static int dra_check_args(dm_ctx *h, const char *who, const DraArgs &a, bool ptrs_ok, int n_paths_out, int n_trace, long long *space) {
  const std::string w(who);
  if (a.J < 1) return fail(h, DM_ERR_INVALID, w + ": num_path_per_item must be at least 1");
  if (a.T < 1) return fail(h, DM_ERR_INVALID, w + ": num_iteration must be at least 1");
  if (a.pw < 1 || a.pw > 8) return fail(h, DM_ERR_INVALID, w + ": penalty_poly_order must be in [1, 8]");
  if (!(a.pf >= 0.0 && a.pf <= 1.7976931348623157e308)) return fail(h, DM_ERR_INVALID, w + ": penalty_factor must be finite and not negative");
  if (a.K < 1 || a.D < 1) return fail(h, DM_ERR_INVALID, w + ": num_node and num_layer must be at least 1");
  long long sp = 1;
  for (int d = 0; d < a.D; d++) {
    if (sp > (((long long)1 << 62) - 1) / a.K) return fail(h, DM_ERR_INVALID, w + ": num_node^num_layer must be below 2^62");
    sp *= a.K;
  }
  *space = sp;
  if (a.num_item < 0 || a.total < 0) return fail(h, DM_ERR_INVALID, w + ": num_item and total must not be negative");
  if (!ptrs_ok) return fail(h, DM_ERR_INVALID, w + ": null argument");
  if (n_paths_out != 0 && n_paths_out != 3) return fail(h, DM_ERR_INVALID, w + ": give out_path_codes, out_path_sizes and out_num_paths together or none of them");
  if (n_trace != 0 && n_trace != 2) return fail(h, DM_ERR_INVALID, w + ": give both trace arrays or neither");
  if (a.total >= ((int64_t)1 << 31)) return fail(h, DM_ERR_UNSUPPORTED, w + ": total must be below 2^31 (entry positions are the sort's 32-bit values)");
  if (a.num_item >= ((int64_t)1 << 31) / a.J) return fail(h, DM_ERR_UNSUPPORTED, w + ": num_item * num_path_per_item must be below 2^31");
  return DM_OK;
}
static const char *dra_bad_text(int kind) {
  switch (kind) {
    case DRA_BAD_OFFSETS: return "its offsets decrease or leave [0, total] (item_off[0] must be 0, item_off[num_item] total)";
    case DRA_BAD_COUNT: return "a hit item needs at least num_path_per_item and at most 2048 candidates";
    case DRA_BAD_CODE: return "a path code outside [0, num_node^num_layer)";
    case DRA_BAD_SCORE: return "a score that is not finite or is negative";
    default: return "a path listed twice";
  }
}

template <int NS>
static int dra_launch_chain(dm_ctx *h, const DraChainParams &p, size_t lds) { return LAUNCH_LDS(h, dra_chain_kernel<NS>, dim3(1), dim3(256), lds, p); }

// All arrays are device arrays; d_out [num_item x J], d_trace_* [T x n_hit x J] or null.  Everything else lies in the handle's grow-only
// block h->dra (hit_cap: room for that many hit items' positions).  Returns with the results in place (the stream is idle).
static int dra_run(dm_ctx *h, const char *who, const DraArgs &a, long long space, const long long *d_off, const long long *d_codes, const double *d_scores, const long long *d_occ,
                   int64_t hit_cap, long long *d_out, int32_t *d_trace_sel, double *d_trace_gain, DraResult *res) {
  const int64_t m = a.total, ni = a.num_item;
  const bool detail = dr_time_launches();
  int rc;
  *res = DraResult();
  if (ni == 0) return DM_OK;
  const int64_t big = std::max<int64_t>(std::max(m, ni), 1);
  DevArena ar(h->dra, 8);
  size_t o_k[2], o_v[2];
  for (int i = 0; i < 2; i++) { o_k[i] = ar.add((size_t)m * 8); o_v[i] = ar.add((size_t)m * 4); }
  const size_t o_flag = ar.add((size_t)big), o_head = ar.add((size_t)m * 4), o_pidx = ar.add((size_t)m * 4), o_pc = ar.add((size_t)m * 8), o_size = ar.add((size_t)m * 4);
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(big)), o_hit = ar.add((size_t)ni * 4), o_last = ar.add((size_t)hit_cap * a.J * 4), o_st = ar.add(64);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  unsigned long long *kb[2] = {ar.ptr<unsigned long long>(o_k[0]), ar.ptr<unsigned long long>(o_k[1])};
  int32_t *vb[2] = {ar.ptr<int32_t>(o_v[0]), ar.ptr<int32_t>(o_v[1])};
  uint8_t *flag = ar.ptr<uint8_t>(o_flag);
  int32_t *head = ar.ptr<int32_t>(o_head), *pidx = ar.ptr<int32_t>(o_pidx), *size = ar.ptr<int32_t>(o_size), *hit = ar.ptr<int32_t>(o_hit), *last = ar.ptr<int32_t>(o_last);
  long long *pcodes = ar.ptr<long long>(o_pc);
  uint32_t *tmp = ar.ptr<uint32_t>(o_tmp);
  unsigned long long *status = ar.ptr<unsigned long long>(o_st);
  HIPCHK(h, hipMemsetAsync(status, 0, 64, h->stream));
  HIPCHK(h, hipMemsetAsync(status + DRA_ST_BAD, 0xff, 8, h->stream));
  // ---- validation and the hit list (ascending id)
  rc = timed(h, EV_DRA_CHECK, detail, [&]() -> int {
    int r;
    if ((r = LAUNCH(h, dra_check_kernel, dim3(drt_blocks(h, ni, 256)), dim3(256), 0, d_off, d_codes, d_scores, d_occ, ni, m, space, a.J, flag, status)) != DM_OK) return r;
    HIPCHK(h, (dev_select_flagged<int32_t>(h->stream, (const int32_t *)nullptr, (const char *)nullptr, (const uint8_t *)flag, hit, (char *)nullptr, status + DRA_ST_HITS, ni, tmp)));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  // ---- dense path indices: entries by code, heads, ranks
  if (m > 0) {
    rc = timed(h, EV_DRA_INDEX, detail, [&]() -> int {
      int r, where = 0;
      if ((r = LAUNCH(h, dra_keys_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, d_codes, m, kb[0], vb[0])) != DM_OK) return r;
      HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[0], vb[0], kb[1], vb[1], m, 0, std::max(1, drm_ceil_log2(space)), tmp, &where));
      if ((r = LAUNCH(h, drm_heads_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, kb[where], m, ~0ull, flag)) != DM_OK) return r;
      HIPCHK(h, (dev_select_flagged<int32_t>(h->stream, (const int32_t *)nullptr, (const char *)nullptr, (const uint8_t *)flag, head, (char *)nullptr, status + DRA_ST_PATHS, m, tmp)));
      if ((r = LAUNCH(h, dra_pidx_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, kb[where], vb[where], flag, head, status + DRA_ST_PATHS, m, d_off, d_occ, ni, pidx, pcodes,
                      status)) != DM_OK) return r;
      HIPCHK(h, hipMemsetAsync(size, 0, (size_t)m * 4, h->stream));
      return DM_OK;
    });
    if (rc != DM_OK) return rc;
  }
  unsigned long long st[8];
  HIPCHK(h, hipMemcpyAsync(st, status, 64, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (st[DRA_ST_BAD] != ~0ull)
    return fail(h, DM_ERR_INVALID, std::string(who) + ": item " + std::to_string((long long)(st[DRA_ST_BAD] >> 3)) + ": " + dra_bad_text((int)(st[DRA_ST_BAD] & 7)));
  const int64_t n_hit = (int64_t)st[DRA_ST_HITS], P = (int64_t)st[DRA_ST_PATHS], max_cnt = (int64_t)st[DRA_ST_MAXCNT];
  if (n_hit > hit_cap) return fail(h, DM_ERR_INVALID, std::string(who) + ": more hit items than the caller's arrays hold");
  // ---- the chain: one launch per iteration (the positions of iteration t - 1 reach iteration t through memory)
  if (n_hit > 0) {
    DraChainParams p{};
    p.off = d_off; p.occ = d_occ; p.scores = d_scores; p.pidx = pidx; p.hit = hit; p.n_hit = n_hit; p.J = a.J; p.pw = a.pw; p.pf = a.pf;
    p.cape = (int)std::max<int64_t>((max_cnt + 63) / 64 * 64, DRA_CAPE_MIN);
    p.size = size; p.last = last; p.status = status; p.trace_sel = d_trace_sel; p.trace_gain = d_trace_gain;
    const size_t lds = 2 * dra_buf_bytes(p.cape) + (size_t)2 * a.J * 4 + 16;
    for (int t = 1; t <= a.T; t++) {
      p.t = t;
      rc = timed(h, EV_DRA_CHAIN, detail, [&] {
        return max_cnt <= 64 ? dra_launch_chain<1>(h, p, lds) : max_cnt <= 256 ? dra_launch_chain<4>(h, p, lds) : dra_launch_chain<DRA_CMAX / 64>(h, p, lds);
      });
      if (rc != DM_OK) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(st, status, 64, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (st[DRA_ST_STOP])
      return fail(h, DM_ERR_INVALID, std::string(who) + ": item " + std::to_string((long long)st[DRA_ST_ITEM]) + ": the accumulated gain left the domain of log1p (iteration " +
                                         std::to_string((long long)st[DRA_ST_ITER]) + ", round " + std::to_string((long long)st[DRA_ST_ROUND]) + ")");
  }
  // ---- the codes: the chosen positions of the hit items, one draw for the others
  rc = timed(h, EV_DRA_RANDOM, detail, [&]() -> int {
    int r;
    if (n_hit > 0 && (r = LAUNCH(h, dra_emit_kernel, dim3(drt_blocks(h, n_hit * a.J, 256)), dim3(256), 0, hit, d_off, d_codes, last, n_hit, a.J, d_out)) != DM_OK) return r;
    return LAUNCH(h, dra_random_kernel, dim3(drt_blocks(h, ni * a.J, 256)), dim3(256), 0, d_occ, ni, a.J, a.K, a.D, a.seed, d_out);
  });
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  res->pcodes = pcodes; res->sizes = size; res->P = P; res->n_hit = n_hit;
  return DM_OK;
}

#define DRA_ARGS(a) DraArgs a{num_item, total, num_node, num_layer, num_path_per_item, num_iteration, penalty_poly_order, penalty_factor, (unsigned long long)seed}

int dm_dr_mstep_assign_paths_dev(dm_handle_t h, const int64_t *d_item_off, const int64_t *d_codes, const double *d_scores, const int64_t *d_occurrence, int64_t num_item,
                                 int64_t total, int num_node, int num_layer, int num_path_per_item, int num_iteration, double penalty_factor, int penalty_poly_order, uint64_t seed,
                                 int64_t *d_out_codes, int64_t *d_out_path_codes, int32_t *d_out_path_sizes, int64_t *out_num_paths, int32_t *d_trace_sel, double *d_trace_gain) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_mstep_assign_paths";
  DRA_ARGS(a);
  const bool ptrs_ok = d_item_off && (num_item <= 0 || (d_occurrence && d_out_codes)) && (total <= 0 || (d_codes && d_scores));
  long long space = 0;
  int rc = dra_check_args(h, who, a, ptrs_ok, (d_out_path_codes ? 1 : 0) + (d_out_path_sizes ? 1 : 0) + (out_num_paths ? 1 : 0), (d_trace_sel ? 1 : 0) + (d_trace_gain ? 1 : 0), &space);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  DraResult r;
  if ((rc = dra_run(h, who, a, space, (const long long *)d_item_off, (const long long *)d_codes, d_scores, (const long long *)d_occurrence, num_item, (long long *)d_out_codes,
                    d_trace_sel, d_trace_gain, &r)) != DM_OK) return rc;
  if (out_num_paths) {
    *out_num_paths = r.P;
    if (r.P) {
      HIPCHK(h, hipMemcpyAsync(d_out_path_codes, r.pcodes, (size_t)r.P * 8, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(d_out_path_sizes, r.sizes, (size_t)r.P * 4, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  }
  return DM_OK;
}

int dm_dr_mstep_assign_paths(dm_handle_t h, const int64_t *item_off, const int64_t *codes, const double *scores, const int64_t *occurrence, int64_t num_item, int64_t total,
                             int num_node, int num_layer, int num_path_per_item, int num_iteration, double penalty_factor, int penalty_poly_order, uint64_t seed,
                             int64_t *out_codes, int64_t *out_path_codes, int32_t *out_path_sizes, int64_t *out_num_paths, int32_t *trace_sel, double *trace_gain) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_mstep_assign_paths";
  DRA_ARGS(a);
  const bool ptrs_ok = item_off && (num_item <= 0 || (occurrence && out_codes)) && (total <= 0 || (codes && scores));
  long long space = 0;
  int rc = dra_check_args(h, who, a, ptrs_ok, (out_path_codes ? 1 : 0) + (out_path_sizes ? 1 : 0) + (out_num_paths ? 1 : 0), (trace_sel ? 1 : 0) + (trace_gain ? 1 : 0), &space);
  if (rc != DM_OK) return rc;
  if (out_num_paths) *out_num_paths = 0;
  if (num_item == 0) return DM_OK;
  int64_t n_hit = 0;
  for (int64_t v = 0; v < num_item; v++) n_hit += occurrence[v] > 0 ? 1 : 0;
  HIPCHK(h, hipSetDevice(h->device));
  const int J = num_path_per_item;
  const size_t n_tr = trace_sel ? (size_t)num_iteration * n_hit * J : 0;
  DevArena io(h->dra_io, 8);
  const size_t o_off = io.add((size_t)(num_item + 1) * 8), o_codes = io.add((size_t)total * 8), o_scores = io.add((size_t)total * 8), o_occ = io.add((size_t)num_item * 8);
  const size_t o_out = io.add((size_t)num_item * J * 8), o_ts = io.add(n_tr * 4), o_tg = io.add(n_tr * 8);
  if ((rc = io.commit(h)) != DM_OK) return rc;
  long long *d_off = io.ptr<long long>(o_off), *d_codes = io.ptr<long long>(o_codes), *d_occ = io.ptr<long long>(o_occ), *d_out = io.ptr<long long>(o_out);
  double *d_scores = io.ptr<double>(o_scores), *d_tg = n_tr ? io.ptr<double>(o_tg) : nullptr;
  int32_t *d_ts = n_tr ? io.ptr<int32_t>(o_ts) : nullptr;
  const hipMemcpyKind hd = hipMemcpyHostToDevice, dh = hipMemcpyDeviceToHost;
  HIPCHK(h, hipMemcpyAsync(d_off, item_off, (size_t)(num_item + 1) * 8, hd, h->stream));
  if (total) {
    HIPCHK(h, hipMemcpyAsync(d_codes, codes, (size_t)total * 8, hd, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_scores, scores, (size_t)total * 8, hd, h->stream));
  }
  HIPCHK(h, hipMemcpyAsync(d_occ, occurrence, (size_t)num_item * 8, hd, h->stream));
  DraResult r;
  if ((rc = dra_run(h, who, a, space, d_off, d_codes, d_scores, d_occ, n_hit, d_out, d_ts, d_tg, &r)) != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(out_codes, d_out, (size_t)num_item * J * 8, dh, h->stream));
  if (n_tr) {
    HIPCHK(h, hipMemcpyAsync(trace_sel, d_ts, n_tr * 4, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(trace_gain, d_tg, n_tr * 8, dh, h->stream));
  }
  if (out_num_paths) {
    *out_num_paths = r.P;
    if (r.P) {
      HIPCHK(h, hipMemcpyAsync(out_path_codes, r.pcodes, (size_t)r.P * 8, dh, h->stream));
      HIPCHK(h, hipMemcpyAsync(out_path_sizes, r.sizes, (size_t)r.P * 4, dh, h->stream));
    }
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

// batchPathScore / streamingPathScore + the assignment: the candidates and the CSR stay on the device (the path scores in the model's block,
// the assignment in the handle's)
int dm_dr_mstep_optimize(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N, int num_candidate_path, int mode, double decay_factor, int num_path_per_item,
                         int num_iteration, double penalty_factor, int penalty_poly_order, uint64_t seed, int64_t *out_codes) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_mstep_optimize";
  const int C = num_candidate_path;
  int rc = drm_check(h, out_codes && (N <= 0 || (seq_ids && targets)), N, C, nullptr, nullptr, nullptr, who);
  if (rc != DM_OK) return rc;
  if (mode != 0 && mode != 1) return fail(h, DM_ERR_INVALID, std::string(who) + ": mode must be 0 (batch) or 1 (streaming)");
  if (mode == 1 && (rc = dms_check_decay(h, who, &decay_factor)) != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  const int64_t num_item = s->num_item, total = 0;
  const int num_node = s->K, num_layer = s->D;
  DRA_ARGS(a);
  long long space = 0;
  if ((rc = dra_check_args(h, who, a, true, 0, 0, &space)) != DM_OK) return rc;
  if ((rc = dr_check_ids(h, seq_ids, N * s->L)) != DM_OK) return rc;
  for (int64_t i = 0; i < N; i++)
    if (targets[i] < 0 || targets[i] >= s->num_item) return fail(h, DM_ERR_INDEX, std::string(who) + ": target outside [0, num_item)");
  if ((rc = dr_check_search(h, who, N, C, false)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const int J = num_path_per_item;
  DevArena io(h->dra_io, 8);
  const size_t o_out = io.add((size_t)num_item * J * 8), o_zero = io.add((size_t)(num_item + 1) * 8);
  if ((rc = io.commit(h)) != DM_OK) return rc;
  long long *d_out = io.ptr<long long>(o_out);
  DrmResult r;
  if (N > 0) {
    const size_t b_seq = DevArena::up((size_t)N * s->L * 4);
    if ((rc = s->ms_io.reserve(h, b_seq + DevArena::up((size_t)N * 4))) != DM_OK) return rc;
    int32_t *d_seq = (int32_t *)s->ms_io.p, *d_tgt = (int32_t *)((char *)s->ms_io.p + b_seq);
    HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids, (size_t)N * s->L * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tgt, targets, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = mode == 0 ? drm_run_any(h, d_seq, d_tgt, N, C, nullptr, &r) : dms_run(h, d_seq, d_tgt, N, C, decay_factor, nullptr, &r)) != DM_OK) return rc;
  } else {                                                 // no sample: every offset and every occurrence 0, every item draws its paths
    long long *z = io.ptr<long long>(o_zero);
    HIPCHK(h, hipMemsetAsync(z, 0, (size_t)(num_item + 1) * 8, h->stream));
    r.item_off = z; r.occ = (const unsigned long long *)z; r.total = 0;
  }
  a.total = r.total;
  DraResult q;
  if ((rc = dra_run(h, who, a, space, r.item_off, r.codes, r.scores, (const long long *)r.occ, std::min<int64_t>(std::max<int64_t>(N, 0), num_item), d_out, nullptr, nullptr, &q)) != DM_OK)
    return rc;
  if (num_item) HIPCHK(h, hipMemcpyAsync(out_codes, d_out, (size_t)num_item * J * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}
