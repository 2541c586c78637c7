// Deep-Retrieval M-step, streaming mode: the exponentially decayed running path scores of every target item, folded on the device
// (DESIGN.md §20).  streamingPathScore (deep-retrieval/.../optim/CoordinateDescent.scala:162-212) is sequential only inside an item: an
// item's running list depends on that item's samples, in sample order, and on nothing else.  So: one beam search per sample chunk (as
// dr_mstep.hip.inc), the samples ordered by item, one worker per item that walks the item's chain with the running list in registers
// (C <= 32: a wave) or in LDS (a workgroup), and a compaction of the final lists into the CSR the batch route hands out.
//
// Order contract: the (target, sample index) pairs are sorted by target with the STABLE radix sort of dev_sort.hip.inc, the values
// enter in ascending sample index, so inside an item's run the sample indices ascend: a chain is folded in ascending sample index.  A
// merge is, with m = the smallest score of the running list, decay * old + new (in both), decay * m + new (in the beam only),
// decay * old (in the list only): fp64, every product and every sum rounded on its own (contract(off) below), then the first C of
// (score descending, code ascending).  The first sample's beam is the list as it is, in the beam's order.  Scores are >= +0 (decay in
// [0, 1], probabilities >= 0), so the order of the scores is the order of their bit patterns and "equal" is bit equality.  No
// floating-point atomics; the queue counter is an integer and only decides which worker folds which item.

#define DMS_DEAD (~0ull)                     // the sort key of a dead entry: behind every score key (those have the top bit clear)
#define DMS_WAVE_C 32                        // up to this many candidates the chain of an item is one wave's

__device__ __forceinline__ unsigned long long dms_score_key(double s) { return (~(unsigned long long)__double_as_longlong(s)) & (~0ull >> 1); }
__device__ __forceinline__ double dms_key_score(unsigned long long k) { return __longlong_as_double((long long)((~k) & (~0ull >> 1))); }
__device__ __forceinline__ unsigned long long dms_readlane64(unsigned long long v, int j) {        // j is the same on every lane
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), j);
  return ((unsigned long long)hi << 32) | lo;
}

// slot (i, c) of samples [i0, i0 + n): the path code (the packing of drm_pairs_kernel), -1 at or past the sample's count
__global__ __launch_bounds__(256) void dms_codes_kernel(const int32_t *paths /* [n][C][D], this chunk */, const int32_t *counts, int64_t i0, int64_t n, int C, int D, int K,
                                                        long long *code) {
  const int64_t slots = n * C;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < slots; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = j / C;
    const int c = (int)(j - i * C);
    long long v = -1;
    if (c < counts[i0 + i]) {
      unsigned long long x = 0;
      for (int d = 0; d < D; d++) x = x * (unsigned long long)K + (unsigned long long)paths[j * D + d];
      v = (long long)x;
    }
    code[(i0 + i) * C + c] = v;
  }
}
// the pairs of the order sort: (target, sample index)
__global__ __launch_bounds__(256) void dms_order_keys_kernel(const int32_t *tgt, int64_t N, unsigned long long *keys, int32_t *vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    keys[i] = (unsigned long long)(unsigned)tgt[i];
    vals[i] = (int32_t)i;
  }
}
// hit item g (the g-th run of the sorted targets, so the hit items ascend with g): its id, its occurrence = the length of its run, and
// its pair of the queue sort: key = N - length (ascending = longest chain first), value = g; positions past the last run get key N
__global__ __launch_bounds__(256) void dms_runs_kernel(const unsigned long long *ks, const int32_t *first, const unsigned long long *n_hit, int64_t N, int64_t hmax, int64_t num_item,
                                                       unsigned long long *hit_item, unsigned long long *occ, unsigned long long *qkey, int32_t *qval) {
  const int64_t H = min((int64_t)*n_hit, hmax);
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < hmax; g += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long key = (unsigned long long)N;
    if (g < H) {
      const int64_t a = first[g], e = g + 1 < H ? (int64_t)first[g + 1] : N;
      const unsigned long long item = ks[a];
      hit_item[g] = item;
      if (item < (unsigned long long)num_item) occ[item] = (unsigned long long)(e - a);      // (the device entry does not range-check: stay inside)
      key = (unsigned long long)(N - (e - a));
    }
    qkey[g] = key;
    qval[g] = (int32_t)g;
  }
}

struct DmsFoldParams {
  const int32_t *queue, *first; const unsigned long long *n_hit;      // hit items in queue order; first sorted position of a hit item; their number
  const int32_t *vs;                                                  // sample indices, sorted by item (ascending inside an item)
  const int32_t *counts; const long long *code; const double *prob;   // the beams: [N], [N][C], [N][C]
  int64_t N, G; int C, P; double decay;                               // G: room for hit items; P: the workgroup form's padded union, a power of two >= 2 C
  unsigned int *head;                                                 // the queue's counter
  long long *pad_code; double *pad_score; int32_t *pad_len;           // [hit items][C], [hit items]
};

// ---- C <= 32: one wave per item.  Lanes 0 .. 31 hold the running list, lanes 32 .. 63 the sample's beam; after a merge the 64 lanes
// hold the union (a list entry that is also in the beam dies, the beam's lane carries the sum), a cross-lane bitonic network orders it by
// (dead last, score descending, code ascending) and lanes 0 .. C - 1 are the new list.  The beam of the NEXT sample is loaded before the
// merge of the current one (the sample index two ahead as well), so that a merge never opens with a global round trip.
__global__ __launch_bounds__(256) void dms_fold_wave_kernel(DmsFoldParams p) {
#pragma clang fp contract(off)   // plain operators, each product and each sum rounded on its own (train_kernel.hip.inc: dm_adam_elem)
  const int lane = threadIdx.x & 63, b = lane & 31;
  const bool is_beam = lane >= 32;
  const int64_t H = min((int64_t)*p.n_hit, p.G);      // (more runs than items: targets out of range on the device entry; stay inside)
  const int C = p.C;
  for (;;) {
    // every lane takes part in the pop (lane 0 adds 1, the others 0) and in the store of the length below: a branch on "lane == 0" at
    // both ends of this loop let the compiler send lanes 1 .. 63 round the loop without lane 0, and the broadcast then read lane 1
    const unsigned q = (unsigned)__builtin_amdgcn_readfirstlane((int)atomicAdd(p.head, lane == 0 ? 1u : 0u));
    if ((int64_t)q >= H) break;
    const int64_t g = p.queue[q];
    const int64_t a = p.first[g], e = g + 1 < H ? (int64_t)p.first[g + 1] : p.N;
    // the first sample: its beam, verbatim
    const int64_t i0 = p.vs[a];
    int slen = __builtin_amdgcn_readfirstlane(min(max(p.counts[i0], 0), C));
    unsigned long long st_code = 0; double st_score = 0.0;
    if (!is_beam && b < slen) { st_code = (unsigned long long)p.code[i0 * C + b]; st_score = p.prob[i0 * C + b]; }
    // (the index two ahead stays an unsigned 32-bit value until it is used: widened with its sign at once, it made every merge open with
    // a wait for it and, the load counter being in order, for the beam loads issued just before it)
    unsigned i2 = a + 2 < e ? (unsigned)p.vs[a + 2] : 0u;
    int n_cnt = 0; unsigned long long n_code = 0; double n_prob = 0.0;
    if (a + 1 < e) {
      const int64_t i1 = p.vs[a + 1];
      n_cnt = p.counts[i1];
      if (is_beam && b < C) { n_code = (unsigned long long)p.code[i1 * C + b]; n_prob = p.prob[i1 * C + b]; }
    }
    for (int64_t t = a + 1; t < e; t++) {
      const int cnt = __builtin_amdgcn_readfirstlane(min(max(n_cnt, 0), C));
      const unsigned long long cd = is_beam ? n_code : st_code;
      const double v = is_beam ? n_prob : st_score;
      if (t + 1 < e) {                                   // the next sample's beam is on its way while this one is merged
        n_cnt = p.counts[i2];
        const uint64_t at = (uint64_t)i2 * (unsigned)C + (unsigned)b;
        if (is_beam && b < C) { n_code = (unsigned long long)p.code[at]; n_prob = p.prob[at]; }
      }
      i2 = t + 2 < e ? (unsigned)p.vs[t + 2] : 0u;
      bool live = is_beam ? b < cnt : b < slen;
      double mn = (!is_beam && live) ? v : __longlong_as_double(0x7ff0000000000000ll);
      for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_xor(mn, o); mn = y < mn ? y : mn; }
      // a beam lane looks for its code in the list, a list lane for its code in the beam: entry j of both, broadcast, per round
      bool both = false; double old = 0.0;
      const int lim = slen > cnt ? slen : cnt;
      for (int j = 0; j < lim; j++) {
        const unsigned long long xs = dms_readlane64(cd, j), xb = dms_readlane64(cd, 32 + j);
        const double os = __longlong_as_double((long long)dms_readlane64((unsigned long long)__double_as_longlong(v), j));
        if (is_beam) { if (j < slen && live && cd == xs) { both = true; old = os; } }
        else if (j < cnt && live && cd == xb) both = true;
      }
      double ns;
      if (is_beam) { const double t1 = p.decay * (both ? old : mn); ns = t1 + v; }
      else { ns = p.decay * v; live = live && !both; }
      unsigned long long k1 = live ? dms_score_key(ns) : DMS_DEAD, k2 = cd;
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          const unsigned long long o1 = __shfl_xor(k1, j), o2 = __shfl_xor(k2, j);
          const bool want_min = ((lane & k) == 0) == ((lane & j) == 0);
          const bool o_less = o1 < k1 || (o1 == k1 && o2 < k2), o_more = o1 > k1 || (o1 == k1 && o2 > k2);
          if (want_min ? o_less : o_more) { k1 = o1; k2 = o2; }
        }
      const int n_live = __popcll(__ballot(k1 != DMS_DEAD));
      slen = n_live < C ? n_live : C;
      st_code = k2; st_score = dms_key_score(k1);        // (lanes 0 .. slen - 1 are read)
    }
    if (!is_beam && b < slen) { p.pad_code[g * C + b] = (long long)st_code; p.pad_score[g * C + b] = st_score; }
    p.pad_len[g] = slen;                                 // (the same value from every lane)
  }
}

// ---- 33 <= C <= 2048: one 256-thread workgroup per item, the union in LDS: key[P], val[P].  Between merges the list is entries
// [0, slen): key = code << 1 (| a stale origin bit), val = the score's sort key.  A merge: the list's entries become (code << 1, score),
// the beam's (code << 1 | 1, probability), the rest (DMS_DEAD, -); a bitonic sort on key brings a code's list entry right in front of
// its beam entry; the beam entries take their new score (A), then the list entries theirs or die (B) — each pass writes only what no
// other thread reads in it; a second sort on (score key, key) leaves the new list in front.  Path codes are below 2^62 (dm_dr_load_model).
template <bool BY_VAL>
__device__ __forceinline__ void dms_lds_sort(unsigned long long *key, unsigned long long *val, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const bool up = (i & k) == 0;
        const unsigned long long ka = key[i], kb = key[l], va = val[i], vb = val[l];
        const bool more = BY_VAL ? (va > vb || (va == vb && ka > kb)) : ka > kb;
        const bool same = BY_VAL ? (va == vb && ka == kb) : ka == kb;
        if (!same && more == up) { key[i] = kb; key[l] = ka; val[i] = vb; val[l] = va; }
      }
      __syncthreads();
    }
}
#define DMS_WG_REGS 8                        // 2048 candidates / 256 threads
__global__ __launch_bounds__(256) void dms_fold_wg_kernel(DmsFoldParams p) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long dms_sm[];
  __shared__ unsigned long long red[4];
  __shared__ unsigned s_q;
  __shared__ int s_match;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = p.C, P = p.P;
  unsigned long long *key = dms_sm, *val = dms_sm + P;
  const int64_t H = min((int64_t)*p.n_hit, p.G);      // (more runs than items: targets out of range on the device entry; stay inside)
  for (;;) {
    __syncthreads();
    if (tid == 0) s_q = atomicAdd(p.head, 1u);
    __syncthreads();
    const unsigned q = s_q;
    if ((int64_t)q >= H) break;
    const int64_t g = p.queue[q];
    const int64_t a = p.first[g], e = g + 1 < H ? (int64_t)p.first[g + 1] : p.N;
    const int64_t i0 = p.vs[a];
    int slen = min(max(p.counts[i0], 0), C);
    for (int c = tid; c < slen; c += 256) { key[c] = (unsigned long long)p.code[i0 * C + c] << 1; val[c] = dms_score_key(p.prob[i0 * C + c]); }
    unsigned i2 = a + 2 < e ? (unsigned)p.vs[a + 2] : 0u;     // (unsigned until it is used, as in the wave form)
    int n_cnt = 0; unsigned long long n_code[DMS_WG_REGS]; double n_prob[DMS_WG_REGS];
#pragma unroll
    for (int r = 0; r < DMS_WG_REGS; r++) { n_code[r] = 0; n_prob[r] = 0.0; }
    if (a + 1 < e) {
      const int64_t i1 = p.vs[a + 1];
      n_cnt = p.counts[i1];
#pragma unroll
      for (int r = 0; r < DMS_WG_REGS; r++)
        if (r * 256 + tid < C) { n_code[r] = (unsigned long long)p.code[i1 * C + r * 256 + tid]; n_prob[r] = p.prob[i1 * C + r * 256 + tid]; }
    }
    for (int64_t t = a + 1; t < e; t++) {
      const int cnt = min(max(n_cnt, 0), C);
      __syncthreads();                                   // the list is in place; s_match and red are free
      // the smallest score = the largest score key; the list's entries turn into (code << 1, score)
      unsigned long long mx = 0;
      for (int c = tid; c < slen; c += 256) {
        const unsigned long long k1 = val[c];
        mx = k1 > mx ? k1 : mx;
        key[c] &= ~1ull;
        val[c] = (unsigned long long)__double_as_longlong(dms_key_score(k1));
      }
      for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(mx, o); mx = y > mx ? y : mx; }
      if (lane == 0) red[wave] = mx;
      if (tid == 0) s_match = 0;
#pragma unroll
      for (int r = 0; r < DMS_WG_REGS; r++) {
        const int c = r * 256 + tid;
        if (c < cnt) { key[slen + c] = (n_code[r] << 1) | 1ull; val[slen + c] = (unsigned long long)__double_as_longlong(n_prob[r]); }
      }
      for (int c = slen + cnt + tid; c < P; c += 256) { key[c] = DMS_DEAD; val[c] = 0; }
      if (t + 1 < e) {                                   // the next sample's beam travels under the two sorts
        n_cnt = p.counts[i2];
#pragma unroll
        for (int r = 0; r < DMS_WG_REGS; r++)
          if (r * 256 + tid < C) { n_code[r] = (unsigned long long)p.code[(uint64_t)i2 * (unsigned)C + (unsigned)(r * 256 + tid)]; n_prob[r] = p.prob[(uint64_t)i2 * (unsigned)C + (unsigned)(r * 256 + tid)]; }
      }
      i2 = t + 2 < e ? (unsigned)p.vs[t + 2] : 0u;
      __syncthreads();
      unsigned long long m4 = red[0];
#pragma unroll
      for (int w = 1; w < 4; w++) m4 = red[w] > m4 ? red[w] : m4;
      const double mn = slen ? dms_key_score(m4) : __longlong_as_double(0x7ff0000000000000ll);
      dms_lds_sort<false>(key, val, P);
      int matched = 0;
      for (int c = tid; c < P; c += 256) {               // (A) beam entries: the sum with the list's entry right in front, or with decay * m
        const unsigned long long kc = key[c];
        if (kc != DMS_DEAD && (kc & 1ull)) {
          const bool both = c > 0 && key[c - 1] == kc - 1;
          matched += both ? 1 : 0;
          const double t1 = p.decay * (both ? __longlong_as_double((long long)val[c - 1]) : mn);
          const double ns = t1 + __longlong_as_double((long long)val[c]);
          val[c] = dms_score_key(ns);
        }
      }
      if (matched) atomicAdd(&s_match, matched);
      __syncthreads();
      for (int c = tid; c < P; c += 256) {               // (B) list entries: decayed, or dead where the beam's entry carries the sum
        const unsigned long long kc = key[c];
        if (kc == DMS_DEAD) val[c] = DMS_DEAD;
        else if (!(kc & 1ull)) {
          const bool both = c + 1 < P && key[c + 1] == kc + 1;
          const double ns = p.decay * __longlong_as_double((long long)val[c]);
          val[c] = both ? DMS_DEAD : dms_score_key(ns);
        }
      }
      __syncthreads();
      dms_lds_sort<true>(key, val, P);
      const int n_live = slen + cnt - s_match;
      slen = n_live < C ? n_live : C;
    }
    __syncthreads();
    for (int c = tid; c < slen; c += 256) { p.pad_code[g * C + c] = (long long)(key[c] >> 1); p.pad_score[g * C + c] = dms_key_score(val[c]); }
    p.pad_len[g] = slen;                                 // (the same value from every thread: no branch on one thread next to the loop's end)
  }
}

// slot (g, c) of the padded block is kept when hit item g has more than c entries
__global__ __launch_bounds__(256) void dms_keep_kernel(const int32_t *pad_len, const unsigned long long *n_hit, int64_t slots, int C, uint8_t *flag) {
  const int64_t H = min((int64_t)*n_hit, slots / C);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < slots; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = j / C;
    flag[j] = (g < H && (int)(j - g * C) < pad_len[g]) ? 1 : 0;
  }
}
// kept entry t: code, score and the item of its slot (hit items ascend with g, so the kept items ascend: drm_offsets_kernel)
__global__ __launch_bounds__(256) void dms_emit_kernel(const int32_t *kept_slot, const unsigned long long *n_kept, const long long *pad_code, const double *pad_score,
                                                       const unsigned long long *hit_item, int64_t slots, int C, long long *codes, double *scores, unsigned long long *kept_item) {
  const int64_t T = (int64_t)*n_kept;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T && t < slots; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = kept_slot[t];
    codes[t] = pad_code[j];
    scores[t] = pad_score[j];
    kept_item[t] = hit_item[j / C];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int dms_pow2_ge(int v) { int n = 1; while (n < v) n <<= 1; return n; }

// d_paths_all: as drm_run.  Everything lies in the state's grow-only block; per call (m = N * C slots, G = min(N, num_item) possible hit
// items): 17 B per slot (probability, code, flag) + the sort scratch, 32 B per sample (count, two pairs of the order sort, first position
// of a run), and per possible hit item 36 B (two pairs of the queue sort, id, length) + 44 B * C (padded list, kept slot, kept item, output)
static int dms_run(dm_ctx *h, const int32_t *d_seq, const int32_t *d_tgt, int64_t N, int C, double decay, int32_t *d_paths_all, DrmResult *res) {
  dm_dr_state *s = h->dr;
  const int K = s->K, D = s->D, L = s->L;
  const int64_t num_item = s->num_item, m = N * C, G = std::min<int64_t>(N, num_item), slots = G * C;
  const int ibits = drm_bits_above(num_item), qbits = drm_bits_above(N);
  const int64_t chunk = std::min<int64_t>(drm_chunk(), N);
  const bool detail = dr_time_launches();
  const bool f32 = s->dtype == DM_F32;
  int rc;
  DevArena ar(s->ms, 8);
  size_t o_k[4], o_v[4];
  for (int i = 0; i < 2; i++) { o_k[i] = ar.add((size_t)N * 8); o_v[i] = ar.add((size_t)N * 4); }
  for (int i = 2; i < 4; i++) { o_k[i] = ar.add((size_t)G * 8); o_v[i] = ar.add((size_t)G * 4); }
  const size_t o_prob = ar.add((size_t)m * 8), o_code = ar.add((size_t)m * 8), o_cnt = ar.add((size_t)N * 4), o_flag = ar.add((size_t)m);
  const size_t o_first = ar.add((size_t)N * 4), o_hit = ar.add((size_t)G * 8), o_len = ar.add((size_t)G * 4);
  const size_t o_pc = ar.add((size_t)slots * 8), o_ps = ar.add((size_t)slots * 8), o_slot = ar.add((size_t)slots * 4), o_kitem = ar.add((size_t)slots * 8);
  const size_t o_oc = ar.add((size_t)slots * 8), o_os = ar.add((size_t)slots * 8), o_tmp = ar.add(dev_sort_scratch_bytes(m));
  const size_t o_off = ar.add((size_t)(num_item + 1) * 8), o_occ = ar.add((size_t)num_item * 8), o_n = ar.add(64);
  const size_t o_paths = d_paths_all ? 0 : ar.add((size_t)chunk * C * D * 4);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  unsigned long long *kb[4]; int32_t *vb[4];
  for (int i = 0; i < 4; i++) { kb[i] = ar.ptr<unsigned long long>(o_k[i]); vb[i] = ar.ptr<int32_t>(o_v[i]); }
  double *prob = ar.ptr<double>(o_prob), *pad_score = ar.ptr<double>(o_ps), *out_scores = ar.ptr<double>(o_os);
  long long *code = ar.ptr<long long>(o_code), *pad_code = ar.ptr<long long>(o_pc), *out_codes = ar.ptr<long long>(o_oc), *item_off = ar.ptr<long long>(o_off);
  int32_t *counts = ar.ptr<int32_t>(o_cnt), *first = ar.ptr<int32_t>(o_first), *pad_len = ar.ptr<int32_t>(o_len), *kept_slot = ar.ptr<int32_t>(o_slot);
  uint8_t *flag = ar.ptr<uint8_t>(o_flag);
  uint32_t *tmp = ar.ptr<uint32_t>(o_tmp);
  unsigned long long *hit_item = ar.ptr<unsigned long long>(o_hit), *kept_item = ar.ptr<unsigned long long>(o_kitem), *occ = ar.ptr<unsigned long long>(o_occ);
  unsigned long long *n_hit = ar.ptr<unsigned long long>(o_n), *n_kept = n_hit + 1;
  unsigned int *head = (unsigned int *)(n_hit + 2);
  HIPCHK(h, hipMemsetAsync(occ, 0, (size_t)num_item * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(n_hit, 0, 64, h->stream));
  // ---- the search, chunk by chunk, and the codes of each chunk
  for (int64_t i0 = 0; i0 < N; i0 += chunk) {
    const int64_t n = std::min<int64_t>(chunk, N - i0);
    int32_t *paths = d_paths_all ? d_paths_all + i0 * C * D : ar.ptr<int32_t>(o_paths);
    rc = f32 ? dr_beam_dev_t<float>(h, d_seq + i0 * L, n, C, paths, prob + i0 * C, counts + i0) : dr_beam_dev_t<double>(h, d_seq + i0 * L, n, C, paths, prob + i0 * C, counts + i0);
    if (rc != DM_OK) return rc;
    rc = timed(h, EV_DMS_CODES, detail, [&] { return LAUNCH(h, dms_codes_kernel, dim3(drt_blocks(h, n * C, 256)), dim3(256), 0, paths, counts, i0, n, C, D, K, code); });
    if (rc != DM_OK) return rc;
  }
  // ---- the samples by item (stable: ascending sample index inside an item), the runs, the queue: longest chain first
  int w1 = 0, w2 = 0;
  rc = timed(h, EV_DMS_ORDER, detail, [&]() -> int {
    int r;
    if ((r = LAUNCH(h, dms_order_keys_kernel, dim3(drt_blocks(h, N, 256)), dim3(256), 0, d_tgt, N, kb[0], vb[0])) != DM_OK) return r;
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[0], vb[0], kb[1], vb[1], N, 0, ibits, tmp, &w1));
    if ((r = LAUNCH(h, drm_heads_kernel, dim3(drt_blocks(h, N, 256)), dim3(256), 0, kb[w1], N, DMS_DEAD, flag)) != DM_OK) return r;
    HIPCHK(h, (dev_select_flagged<int32_t>(h->stream, (const int32_t *)nullptr, (const char *)nullptr, (const uint8_t *)flag, first, (char *)nullptr, n_hit, N, tmp)));
    if ((r = LAUNCH(h, dms_runs_kernel, dim3(drt_blocks(h, G, 256)), dim3(256), 0, kb[w1], first, n_hit, N, G, num_item, hit_item, occ, kb[2], vb[2])) != DM_OK) return r;
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[2], vb[2], kb[3], vb[3], G, 0, qbits, tmp, &w2));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  // ---- the fold: one worker per item, handed out by the counter
  {
    DmsFoldParams p{};
    p.queue = vb[2 + w2]; p.first = first; p.n_hit = n_hit; p.vs = vb[w1]; p.counts = counts; p.code = code; p.prob = prob;
    p.N = N; p.G = G; p.C = C; p.P = dms_pow2_ge(2 * C); p.decay = decay; p.head = head;
    p.pad_code = pad_code; p.pad_score = pad_score; p.pad_len = pad_len;
    if (C <= DMS_WAVE_C) {
      const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((G + 3) / 4, (int64_t)h->n_cu * 4));
      rc = timed(h, EV_DMS_FOLD, detail, [&] { return LAUNCH(h, dms_fold_wave_kernel, dim3(grid), dim3(256), 0, p); });
    } else {
      const size_t lds = (size_t)p.P * 16;
      const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (int64_t)(128 * 1024) / (int64_t)lds));
      const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(G, (int64_t)h->n_cu * per_cu));
      rc = timed(h, EV_DMS_FOLD, detail, [&] { return LAUNCH_LDS(h, dms_fold_wg_kernel, dim3(grid), dim3(256), lds, p); });
    }
    if (rc != DM_OK) return rc;
  }
  // ---- the lists, compacted into the CSR in ascending item id
  rc = timed(h, EV_DMS_EMIT, detail, [&]() -> int {
    int r;
    if ((r = LAUNCH(h, dms_keep_kernel, dim3(drt_blocks(h, slots, 256)), dim3(256), 0, pad_len, n_hit, slots, C, flag)) != DM_OK) return r;
    HIPCHK(h, (dev_select_flagged<int32_t>(h->stream, (const int32_t *)nullptr, (const char *)nullptr, (const uint8_t *)flag, kept_slot, (char *)nullptr, n_kept, slots, tmp)));
    if ((r = LAUNCH(h, dms_emit_kernel, dim3(drt_blocks(h, slots, 256)), dim3(256), 0, kept_slot, n_kept, pad_code, pad_score, hit_item, slots, C, out_codes, out_scores,
                    kept_item)) != DM_OK) return r;
    return LAUNCH(h, drm_offsets_kernel, dim3(drt_blocks(h, num_item + 1, 256)), dim3(256), 0, kept_item, n_kept, num_item, item_off);
  });
  if (rc != DM_OK) return rc;
  unsigned long long total = 0;
  HIPCHK(h, hipMemcpyAsync(&total, n_kept, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));            // the call's one wait before its results move
  res->item_off = item_off; res->codes = out_codes; res->scores = out_scores; res->occ = occ; res->prob = prob; res->counts = counts;
  res->total = (int64_t)total;
  return DM_OK;
}

static int dms_check_decay(dm_ctx *h, const char *who, double *decay) {
  if (!(*decay >= 0.0 && *decay <= 1.0)) return fail(h, DM_ERR_INVALID, std::string(who) + ": decay_factor must be finite and in [0, 1]");
  *decay = *decay + 0.0;                                 // (-0 -> +0: scores stay >= +0)
  return DM_OK;
}

int dm_dr_mstep_streaming_path_scores_dev(dm_handle_t h, const int32_t *d_seq_ids, const int32_t *d_targets, int64_t N, int num_candidate_path, double decay_factor, int64_t cap,
                                          int64_t *d_out_item_off, int64_t *d_out_codes, double *d_out_scores, int64_t *d_out_occurrence, int64_t *out_total,
                                          int32_t *d_trace_paths, double *d_trace_probs, int32_t *d_trace_counts) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_mstep_streaming_path_scores";
  const int C = num_candidate_path;
  const bool ptrs_ok = d_out_item_off && out_total && cap >= 0 && (N <= 0 || (d_seq_ids && d_targets)) && (cap == 0 || (d_out_codes && d_out_scores));
  int rc = drm_check(h, ptrs_ok, N, C, d_trace_paths, d_trace_probs, d_trace_counts, who);
  if (rc != DM_OK || (rc = dms_check_decay(h, who, &decay_factor)) != DM_OK || (rc = dr_check_search(h, who, N, C, false)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  dm_dr_state *s = h->dr;
  if (N == 0) {
    HIPCHK(h, hipMemsetAsync(d_out_item_off, 0, (size_t)(s->num_item + 1) * 8, h->stream));
    if (d_out_occurrence) HIPCHK(h, hipMemsetAsync(d_out_occurrence, 0, (size_t)s->num_item * 8, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *out_total = 0;
    return DM_OK;
  }
  DrmResult r;
  if ((rc = dms_run(h, d_seq_ids, d_targets, N, C, decay_factor, d_trace_paths, &r)) != DM_OK) return rc;
  *out_total = r.total;
  if (r.total > cap) return drm_short_cap(h, cap, r.total, who);
  const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
  HIPCHK(h, hipMemcpyAsync(d_out_item_off, r.item_off, (size_t)(s->num_item + 1) * 8, dd, h->stream));
  if (r.total) {
    HIPCHK(h, hipMemcpyAsync(d_out_codes, r.codes, (size_t)r.total * 8, dd, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_out_scores, r.scores, (size_t)r.total * 8, dd, h->stream));
  }
  if (d_out_occurrence) HIPCHK(h, hipMemcpyAsync(d_out_occurrence, r.occ, (size_t)s->num_item * 8, dd, h->stream));
  if (d_trace_paths) {
    HIPCHK(h, hipMemcpyAsync(d_trace_probs, r.prob, (size_t)N * C * 8, dd, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_trace_counts, r.counts, (size_t)N * 4, dd, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_dr_mstep_streaming_path_scores(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N, int num_candidate_path, double decay_factor, int64_t cap,
                                      int64_t *out_item_off, int64_t *out_codes, double *out_scores, int64_t *out_occurrence, int64_t *out_total, int32_t *trace_paths,
                                      double *trace_probs, int32_t *trace_counts) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_mstep_streaming_path_scores";
  const int C = num_candidate_path;
  const bool ptrs_ok = out_item_off && out_total && cap >= 0 && (N <= 0 || (seq_ids && targets)) && (cap == 0 || (out_codes && out_scores));
  int rc = drm_check(h, ptrs_ok, N, C, trace_paths, trace_probs, trace_counts, who);
  if (rc != DM_OK || (rc = dms_check_decay(h, who, &decay_factor)) != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, N * s->L)) != DM_OK) return rc;
  for (int64_t i = 0; i < N; i++)
    if (targets[i] < 0 || targets[i] >= s->num_item) return fail(h, DM_ERR_INDEX, std::string(who) + ": target outside [0, num_item)");
  if ((rc = dr_check_search(h, who, N, C, false)) != DM_OK) return rc;
  if (N == 0) {
    memset(out_item_off, 0, (size_t)(s->num_item + 1) * 8);
    if (out_occurrence) memset(out_occurrence, 0, (size_t)s->num_item * 8);
    *out_total = 0;
    return DM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t b_seq = DevArena::up((size_t)N * s->L * 4);
  if ((rc = s->ms_io.reserve(h, b_seq + DevArena::up((size_t)N * 4))) != DM_OK) return rc;
  int32_t *d_seq = (int32_t *)s->ms_io.p, *d_tgt = (int32_t *)((char *)s->ms_io.p + b_seq);
  HIPCHK(h, hipMemcpyAsync(d_seq, seq_ids, (size_t)N * s->L * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_tgt, targets, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
  DevTemps tmp(h);
  int32_t *d_paths_all = nullptr;
  if (trace_paths && (rc = tmp.alloc(d_paths_all, (size_t)N * C * s->D * 4)) != DM_OK) return rc;
  DrmResult r;
  if ((rc = dms_run(h, d_seq, d_tgt, N, C, decay_factor, d_paths_all, &r)) != DM_OK) return rc;
  *out_total = r.total;
  if (r.total > cap) return drm_short_cap(h, cap, r.total, who);
  const hipMemcpyKind dh = hipMemcpyDeviceToHost;
  HIPCHK(h, hipMemcpyAsync(out_item_off, r.item_off, (size_t)(s->num_item + 1) * 8, dh, h->stream));
  if (r.total) {
    HIPCHK(h, hipMemcpyAsync(out_codes, r.codes, (size_t)r.total * 8, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(out_scores, r.scores, (size_t)r.total * 8, dh, h->stream));
  }
  if (out_occurrence) HIPCHK(h, hipMemcpyAsync(out_occurrence, r.occ, (size_t)s->num_item * 8, dh, h->stream));
  if (trace_paths) {
    HIPCHK(h, hipMemcpyAsync(trace_paths, d_paths_all, (size_t)N * C * s->D * 4, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(trace_probs, r.prob, (size_t)N * C * 8, dh, h->stream));
    HIPCHK(h, hipMemcpyAsync(trace_counts, r.counts, (size_t)N * 4, dh, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}
