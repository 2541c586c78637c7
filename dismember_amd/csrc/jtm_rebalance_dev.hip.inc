// The greedy capacity-bounded re-balance of JTM tree learning (getChildrenProjection after scoring: sortNodeWeights + first
// choice + reBalance, jtm/src/main/scala/com/mass/jtm/optim/TreeLearning.scala:137-150, 58-97, 217-265) for EVERY parent
// node of a level at once, on the device.  jtm_rebalance_t (jtm_host.hip.inc) is the same logic per parent on the host; the
// two are bit-identical (tests/test_gpu_edges.py) and the host one remains for tiny inputs.  W = float (JTM) or double (OTM's
// TreeConstruction.reBalance, otm/src/main/scala/com/mass/otm/tree/TreeConstruction.scala:304-352: the same logic on Double
// weights); gaps up to 8 (256 children per parent: the processed set is a 256-bit mask per parent).
//
// Per parent the reference repeats: take the fullest not-yet-processed child list; if it holds more than max_assign items,
// sort it stably by (moved out of its old subtree?, weight descending by Float.compare), keep the first max_assign and hand
// each overflow item, in sorted order, to its next-best child that has not been processed.  Parents are independent, and in
// one ROUND every parent processes at most one child, so a round is data-parallel over all items of the level:
//   * `order` holds the items so that the members of any one child list appear in their list order (initially item order;
//     after a round: everything that stayed, in the previous order, then the overflow items in their sorted order — exactly
//     "append to the destination list");
//   * the items of the lists being processed are compacted (stable) and sorted by ONE stable 64-bit radix sort (dev_sort.hip.inc) on
//     (parent | moved | descending weight key): stability supplies the reference's tie order (list position); double weights
//     need 64 key bits of their own, so they take two stable passes (descending weight key, then parent | moved);
//   * rank inside the parent's segment >= max_assign  <=>  overflow.
// Rounds end when no parent has an over-full list: at most 2^gap rounds, one 8-byte read-back each.
#include "dev_sort.hip.inc"

// Node codes are int32_t everywhere (the ABI's out_node included): the last code of level 30 is 2^31 - 2, a level-31 code does not fit.
// Every re-balance route refuses such a level by name before it allocates anything.
static const int JTM_MAX_LEVEL = 30;
static int jtm_level_refused(dm_ctx *h, int level, const char *who) {
  return fail(h, DM_ERR_INVALID, std::string(who) + ": level " + std::to_string(level) + " is above " + std::to_string(JTM_MAX_LEVEL) + " (its node codes do not fit int32)");
}

template <typename W>
struct JtmRbState {
  const W *w;                // [n][C]
  const int32_t *old_node;   // [n] ancestor of the item's CURRENT leaf at `level`
  const int32_t *item_node;  // [n] parent code at old_level
  int64_t n;
  int C, gap, cap;
  int32_t lo;                // first code of old_level
  int64_t P;                 // parents of the level
  int PW;                    // 32-bit words of a parent's processed mask
  uint8_t *cand;             // [n][C]
  int16_t *cur;              // [n] current child, -1 = dropped
  uint16_t *kidx;            // [n] next candidate index
  int32_t *sizes;            // [P][C]
  uint32_t *processed;       // [P][PW]
  int16_t *bc;               // [P] child processed this round, -1 = parent idle
  unsigned long long *counters;   // [0] active parents, [1] selected items, [2] overflow items
};

__device__ __forceinline__ uint32_t jtm_asc_key(float w) {      // Float.compare order, ascending (one canonical NaN, greatest)
  uint32_t b = (w != w) ? 0x7fc00000u : __float_as_uint(w);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint64_t jtm_asc_key(double w) {     // Double.compare order
  uint64_t b = (w != w) ? 0x7ff8000000000000ull : (uint64_t)__double_as_longlong(w);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
template <typename W> struct JtmAsc;
template <> struct JtmAsc<float> { typedef uint32_t K; };
template <> struct JtmAsc<double> { typedef uint64_t K; };

// sortNodeWeights (stable, descending) + first choice
template <typename W, int CMAX>
__global__ void jtm_rb_init_kernel(JtmRbState<W> s, int32_t *order) {
  typedef typename JtmAsc<W>::K K;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * blockDim.x) {
    K key[CMAX]; uint8_t c[CMAX];
    const W *w = s.w + i * s.C;
    for (int k = 0; k < s.C; k++) { key[k] = jtm_asc_key(w[k]); c[k] = (uint8_t)k; }
    for (int a = 1; a < s.C; a++) {            // stable insertion sort, descending
      const K kv = key[a]; const uint8_t cv = c[a];
      int b = a - 1;
      while (b >= 0 && key[b] < kv) { key[b + 1] = key[b]; c[b + 1] = c[b]; b--; }
      key[b + 1] = kv; c[b + 1] = cv;
    }
    for (int k = 0; k < s.C; k++) s.cand[i * s.C + k] = c[k];
    // an item that does not sit in a node of old_level (dropped by the greedy loop of an earlier gap step when the catalogue exceeds
    // 2^max_level) takes no part: the reference only visits getAllNodesAtLevel(oldLevel) and `oldProjection ++ new` keeps its entry
    const bool in_level = s.item_node[i] >= s.lo && (int64_t)s.item_node[i] - s.lo < s.P;
    s.cur[i] = in_level ? (int16_t)c[0] : (int16_t)-1; s.kidx[i] = in_level ? 1 : 0xFFFF;
    order[i] = (int32_t)i;
  }
}

template <typename W>
__global__ void jtm_rb_sizes_kernel(JtmRbState<W> s) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = s.cur[i];
    if (c >= 0) atomicAdd(&s.sizes[(int64_t)(s.item_node[i] - s.lo) * s.C + c], 1);
  }
}
// few parents (top of the tree): per-block LDS histogram first, or every item of the level hits the same handful of counters
template <typename W>
__global__ void jtm_rb_sizes_small_kernel(JtmRbState<W> s) {
  extern __shared__ int hist[];
  const int nb = (int)(s.P * s.C);
  for (int t = threadIdx.x; t < nb; t += blockDim.x) hist[t] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = s.cur[i];
    if (c >= 0) atomicAdd(&hist[(s.item_node[i] - s.lo) * s.C + c], 1);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nb; t += blockDim.x) if (hist[t]) atomicAdd(&s.sizes[t], hist[t]);
}

// getMaxNode (first maximum in child order among the unprocessed, non-empty lists) and the loop condition
template <typename W>
__global__ void jtm_rb_choose_kernel(JtmRbState<W> s) {
  unsigned long long act = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < s.P; p += (int64_t)gridDim.x * blockDim.x) {
    uint32_t *pr = s.processed + p * s.PW;
    int best = -1, b = 0;
    for (int c = 0; c < s.C; c++) {
      const int sz = s.sizes[p * s.C + c];
      const int v = (!((pr[c >> 5] >> (c & 31)) & 1u) && sz > 0) ? sz : -1;
      if (c == 0 || v > best) { best = v; b = c; }
    }
    if (best > s.cap) { s.bc[p] = (int16_t)b; pr[b >> 5] |= 1u << (b & 31); act++; }
    else s.bc[p] = -1;
  }
  for (int o = 32; o > 0; o >>= 1) act += __shfl_xor(act, o);
  if ((threadIdx.x & 63) == 0 && act) atomicAdd(&s.counters[0], act);
}

// members of the lists being processed this round, in list order: flag + sort key(s).  float: one word (parent | moved | ~weight key);
// double: key = ~weight key (first pass), key2 = parent | moved (second, stable pass)
template <typename W>
__global__ void jtm_rb_flag_kernel(JtmRbState<W> s, const int32_t *order, uint8_t *flag, unsigned long long *key) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < s.n; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t it = order[j];
    const int c = s.cur[it];
    if (c < 0) { flag[j] = 0; continue; }         // dropped, or outside the level: never a member of a list
    const int64_t p = s.item_node[it] - s.lo;
    const int b = s.bc[p];
    const bool f = b >= 0 && c == b;
    flag[j] = f;
    if (f) {
      if (sizeof(W) == 4) {
        const int32_t this_code = (int32_t)((((int64_t)s.item_node[it]) << s.gap) + s.C - 1 + b);
        const unsigned long long moved = s.old_node[it] != this_code;
        key[j] = ((unsigned long long)p << 33) | (moved << 32) | (unsigned long long)(uint32_t)(~jtm_asc_key(s.w[(int64_t)it * s.C + b]));
      } else {
        key[j] = ~(unsigned long long)jtm_asc_key(s.w[(int64_t)it * s.C + b]);
      }
    }
  }
}
// double weights, second pass: (parent | moved) of the items in weight order
template <typename W>
__global__ void jtm_rb_key2_kernel(JtmRbState<W> s, const int32_t *sitem, int64_t m, unsigned long long *key2) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t it = sitem[j];
    const int64_t p = s.item_node[it] - s.lo;
    const int b = s.bc[p];
    const int32_t this_code = (int32_t)((((int64_t)s.item_node[it]) << s.gap) + s.C - 1 + b);
    const unsigned long long moved = s.old_node[it] != this_code;
    key2[j] = ((unsigned long long)p << 33) | (moved << 32);
  }
}

// first sorted position of every parent's segment
__global__ void jtm_rb_segstart_kernel(const unsigned long long *skey, int64_t m, int64_t *seg_start) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = (int64_t)(skey[j] >> 33);
    if (j == 0 || (int64_t)(skey[j - 1] >> 33) != p) seg_start[p] = j;
  }
}

// the cut: rank >= max_assign leaves for the next unprocessed candidate (or drops out when none is left)
template <typename W>
__global__ void jtm_rb_cut_kernel(JtmRbState<W> s, const unsigned long long *skey, const int32_t *sitem, int64_t m, const int64_t *seg_start,
                                  uint8_t *oflag_sorted, uint8_t *stay /* [n] by item */) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = (int64_t)(skey[j] >> 33);
    const bool ovf = j - seg_start[p] >= (int64_t)s.cap;
    oflag_sorted[j] = ovf;
    if (ovf) {
      const int32_t it = sitem[j];
      const uint32_t *pr = s.processed + p * s.PW;
      int nc = -1, k = s.kidx[it];
      for (; k < s.C; k++) {
        const int c = s.cand[(int64_t)it * s.C + k];
        if (!((pr[c >> 5] >> (c & 31)) & 1u)) { nc = c; break; }
      }
      s.cur[it] = (int16_t)nc; s.kidx[it] = (uint16_t)(k + 1 < 0xFFFF ? k + 1 : 0xFFFF);
      stay[it] = 0;
    }
  }
}
__global__ void jtm_rb_stayflag_kernel(const int32_t *order, const uint8_t *stay, int64_t n, uint8_t *flag) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) flag[j] = stay[order[j]];
}
template <typename W>
__global__ void jtm_rb_out_kernel(JtmRbState<W> s, int32_t *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = s.cur[i];
    out[i] = c >= 0 ? (int32_t)((((int64_t)s.item_node[i]) << s.gap) + s.C - 1 + c) : s.item_node[i];
  }
}

// device buffers in, device buffer out; asynchronous except for one small read-back per round.  Returns DM_ERR_UNSUPPORTED
// (without a message) when the shape is outside what the device version covers: the caller falls back to the host logic.
template <typename W>
static int jtm_rebalance_all_dev(dm_ctx *h, const W *d_w, const int32_t *d_old_node, const int32_t *d_item_node, int64_t n,
                                 int old_level, int level, int max_assign, int32_t *d_out) {
  if (level > JTM_MAX_LEVEL) return jtm_level_refused(h, level, sizeof(W) == 8 ? "dm_otm_rebalance_all" : "dm_jtm_rebalance_all");
  const int gap = level - old_level, C = 1 << gap;
  const bool two_pass = sizeof(W) == 8;
  if (C > 256 || old_level > 24 || n >= ((int64_t)1 << 31) || n <= 0) return DM_ERR_UNSUPPORTED;
  HIPCHK(h, hipSetDevice(h->device));
  JtmRbState<W> s;
  s.PW = (C + 31) / 32;
  s.w = d_w; s.old_node = d_old_node; s.item_node = d_item_node; s.n = n; s.C = C; s.gap = gap; s.cap = max_assign;
  s.lo = (int32_t)(((int64_t)1 << old_level) - 1); s.P = (int64_t)1 << old_level;
  // one arena: state + double-buffered order / keys / flags + the count arrays of the select / sort passes
  size_t tmp_bytes = dev_sort_scratch_bytes(n);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += DevArena::up(bytes); return o; };
  const size_t o_cand = take((size_t)n * C), o_cur = take((size_t)n * 2), o_kidx = take((size_t)n * 2), o_sizes = take((size_t)s.P * C * 4),
               o_proc = take((size_t)s.P * s.PW * 4), o_bc = take((size_t)s.P * 2), o_cnt = take(64), o_ord0 = take((size_t)n * 4), o_ord1 = take((size_t)n * 4),
               o_flag = take((size_t)n), o_key = take((size_t)n * 8), o_ckey = take((size_t)n * 8), o_citem = take((size_t)n * 4),
               o_skey = take((size_t)n * 8), o_sitem = take((size_t)n * 4), o_seg = take((size_t)s.P * 8), o_oflag = take((size_t)n),
               o_stay = take((size_t)n), o_ovf = take((size_t)n * 4), o_tmp = take(tmp_bytes);
  char *A = nullptr;
  DevTemps t(h);
  int rc = t.alloc(A, off);
  if (rc != DM_OK) return rc;
  auto fin = [&](int r) { (void)hipStreamSynchronize(h->stream); return r; };
  s.cand = (uint8_t *)(A + o_cand); s.cur = (int16_t *)(A + o_cur); s.kidx = (uint16_t *)(A + o_kidx); s.sizes = (int32_t *)(A + o_sizes);
  s.processed = (uint32_t *)(A + o_proc); s.bc = (int16_t *)(A + o_bc); s.counters = (unsigned long long *)(A + o_cnt);
  int32_t *ord[2] = {(int32_t *)(A + o_ord0), (int32_t *)(A + o_ord1)};
  uint8_t *flag = (uint8_t *)(A + o_flag), *oflag = (uint8_t *)(A + o_oflag), *stay = (uint8_t *)(A + o_stay);
  unsigned long long *key = (unsigned long long *)(A + o_key), *ckey = (unsigned long long *)(A + o_ckey), *skey = (unsigned long long *)(A + o_skey);
  int32_t *citem = (int32_t *)(A + o_citem), *sitem = (int32_t *)(A + o_sitem), *ovf = (int32_t *)(A + o_ovf);
  int64_t *seg = (int64_t *)(A + o_seg);
  uint32_t *tmp = (uint32_t *)(A + o_tmp);
  const unsigned GB = 2048, TB = 256;
  hipError_t e = hipMemsetAsync(s.processed, 0, (size_t)s.P * s.PW * 4, h->stream);
  if (e != hipSuccess) return fin(fail(h, DM_ERR_HIP, "dm_jtm_rebalance_all: memset failed"));
  rc = C <= 32 ? LAUNCH(h, (jtm_rb_init_kernel<W, 32>), dim3(GB), dim3(TB), 0, s, ord[0]) : LAUNCH(h, (jtm_rb_init_kernel<W, 256>), dim3(GB), dim3(TB), 0, s, ord[0]);
  if (rc != DM_OK) return fin(rc);
  const int end_bit = 33 + (old_level > 0 ? old_level : 1);
  int curo = 0;
  hipError_t ce = hipSuccess;          // first error of a select / sort pass
  auto ck = [&](hipError_t r) { if (ce == hipSuccess && r != hipSuccess) ce = r; };
  for (int round = 0; round <= C; round++) {
    (void)hipMemsetAsync(s.sizes, 0, (size_t)s.P * C * 4, h->stream);
    (void)hipMemsetAsync(s.counters, 0, 24, h->stream);
    rc = s.P * C <= 8192 ? LAUNCH(h, jtm_rb_sizes_small_kernel<W>, dim3(512), dim3(TB), (size_t)s.P * C * 4, s) : LAUNCH(h, jtm_rb_sizes_kernel<W>, dim3(GB), dim3(TB), 0, s);
    if (rc != DM_OK) return fin(rc);
    if ((rc = LAUNCH(h, jtm_rb_choose_kernel<W>, dim3((unsigned)std::min<int64_t>((s.P + TB - 1) / TB, 4096)), dim3(TB), 0, s)) != DM_OK) return fin(rc);
    if ((rc = LAUNCH(h, jtm_rb_flag_kernel<W>, dim3(GB), dim3(TB), 0, s, ord[curo], flag, key)) != DM_OK) return fin(rc);
    ck(dev_select_flagged<int32_t, unsigned long long>(h->stream, ord[curo], key, flag, citem, ckey, s.counters + 1, n, tmp));      // items and keys in one pass
    unsigned long long hc[2] = {0, 0};
    if (hipMemcpyAsync(hc, s.counters, 16, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
      return fin(fail(h, DM_ERR_HIP, "dm_jtm_rebalance_all: device pass failed"));
    if (ce != hipSuccess) return fin(fail(h, DM_ERR_HIP, std::string("dm_jtm_rebalance_all: ") + hipGetErrorString(ce)));
    if (hc[0] == 0) break;                                   // no parent has an over-full list left
    const int64_t m = (int64_t)hc[1];
    // (skey, sitem) name the sorted pair afterwards; the buffers are scratch of equal size, so the names follow the data
    int wh = 0;
    if (!two_pass) {
      ck(dev_radix_sort_pairs(h->stream, ckey, citem, skey, sitem, m, 0, end_bit, tmp, &wh));
      if (wh == 0) { std::swap(ckey, skey); std::swap(citem, sitem); }
    } else {
      // double weights: stable sort by the descending weight key (all 64 bits), then by (parent | moved) — LSD order, both passes stable.
      // `key` (the uncompacted keys) is dead after the compaction and serves as the second pass's key buffer
      ck(dev_radix_sort_pairs(h->stream, ckey, citem, skey, sitem, m, 0, 64, tmp, &wh));
      if (wh == 0) { std::swap(ckey, skey); std::swap(citem, sitem); }
      if ((rc = LAUNCH(h, jtm_rb_key2_kernel<W>, dim3(GB), dim3(TB), 0, s, sitem, m, key)) != DM_OK) return fin(rc);
      ck(dev_radix_sort_pairs(h->stream, key, sitem, skey, citem, m, 32, end_bit, tmp, &wh));
      if (wh == 0) { std::swap(key, skey); } else { std::swap(citem, sitem); }
    }
    if ((rc = LAUNCH(h, jtm_rb_segstart_kernel, dim3(GB), dim3(TB), 0, skey, m, seg)) != DM_OK) return fin(rc);
    (void)hipMemsetAsync(stay, 1, (size_t)n, h->stream);
    if ((rc = LAUNCH(h, jtm_rb_cut_kernel<W>, dim3(GB), dim3(TB), 0, s, skey, sitem, m, seg, oflag, stay)) != DM_OK) return fin(rc);
    // new list order: everything that stayed (previous order), then the overflow in sorted order
    if ((rc = LAUNCH(h, jtm_rb_stayflag_kernel, dim3(GB), dim3(TB), 0, ord[curo], stay, n, flag)) != DM_OK) return fin(rc);
    ck(dev_select_flagged<int32_t>(h->stream, ord[curo], (const char *)nullptr, flag, ord[curo ^ 1], (char *)nullptr, s.counters + 1, n, tmp));
    ck(dev_select_flagged<int32_t>(h->stream, sitem, (const char *)nullptr, oflag, ovf, (char *)nullptr, s.counters + 2, m, tmp));
    unsigned long long hk[3] = {0, 0, 0};
    if (hipMemcpyAsync(hk, s.counters, 24, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
      return fin(fail(h, DM_ERR_HIP, "dm_jtm_rebalance_all: device pass failed"));
    if (ce != hipSuccess) return fin(fail(h, DM_ERR_HIP, std::string("dm_jtm_rebalance_all: ") + hipGetErrorString(ce)));
    if ((int64_t)(hk[1] + hk[2]) != n) return fin(fail(h, DM_ERR_HIP, "dm_jtm_rebalance_all: internal count mismatch"));
    if (hk[2] && hipMemcpyAsync(ord[curo ^ 1] + hk[1], ovf, (size_t)hk[2] * 4, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
      return fin(fail(h, DM_ERR_HIP, "dm_jtm_rebalance_all: copy failed"));
    curo ^= 1;
  }
  return fin(LAUNCH(h, jtm_rb_out_kernel<W>, dim3(GB), dim3(TB), 0, s, d_out));
}
