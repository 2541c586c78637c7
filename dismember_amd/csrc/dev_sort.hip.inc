// Device-wide stable compaction and stable LSD radix sort of (64-bit key, 32-bit value) pairs, written for gfx950 (round 6: replaces the
// hipCUB DeviceSelect / DeviceRadixSort calls of the JTM re-balance, jtm_rebalance_dev.hip.inc — the one place the product used a
// device library).  Both are "count, scan, scatter" over tiles of 4 096 elements, one 256-thread workgroup (four 64-lane waves) per tile:
//   * a tile is visited in 16 rounds of 256 consecutive elements, element e * 256 + tid by thread tid, so that global reads are coalesced
//     and the order inside a tile is (round, wave, lane);
//   * a round ranks its elements with wave ballots: the peers of a lane are the lanes of its wave holding the same digit (eight ballots,
//     one per digit bit), its rank among them the population count of the peers below it; the wave totals meet in LDS ([wave][digit]) and
//     the running per-digit bases of the tile are advanced once per round.  The order of equal digits is therefore the input order: every
//     pass is stable, which is what the LSD sort and the reference's tie order (TreeLearning.scala:230-246: list position) need;
//   * the per-tile digit counts of a pass ([256 digits][tiles]) are scanned row by row, one workgroup per digit, coalesced; the scatter
//     kernel adds the scan of the 256 row totals.
// Nothing here is tuned beyond that: the re-balance is 6 % of JTM.optimize.
#define DSORT_TB 256
#define DSORT_ITEMS 16
#define DSORT_TILE (DSORT_TB * DSORT_ITEMS)

// scratch (carved from the caller's arena): [256 x tiles] pass counts + [256] digit totals (sort) / [tiles] (select)
static inline size_t dev_sort_scratch_bytes(int64_t n) {
  const int64_t tiles = (n + DSORT_TILE - 1) / DSORT_TILE;
  return (size_t)(256 * (tiles > 0 ? tiles : 1) + 1024) * sizeof(uint32_t);
}

// workgroup-wide exclusive scan of one value per thread (NT threads, NT / 64 <= 16 waves); returns the exclusive prefix, *total = the sum
template <int NT>
__device__ __forceinline__ uint32_t dsort_block_scan(uint32_t v, uint32_t *wsum /* [NT / 64] LDS */, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  __syncthreads();                                 // (wsum may still be read from a previous call)
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) { const uint32_t x = wsum[w]; before += w < wave ? x : 0u; tot += x; }
  *total = tot;
  return before + inc - v;
}
// exclusive scan of T 32-bit counts in place by ONE workgroup of 1 024 threads, coalesced chunks of 1 024 with a running carry (the
// compaction's per-tile counts: 2 442 entries for 10 M elements); the grand total goes to *total (may be null)
__global__ __launch_bounds__(1024) void dsort_scan_kernel(uint32_t *c, int64_t T, unsigned long long *total) {
  __shared__ uint32_t wsum[16];
  uint32_t carry = 0;
  for (int64_t base = 0; base < T; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < T ? c[i] : 0u;
    uint32_t tot;
    const uint32_t ex = dsort_block_scan<1024>(v, wsum, &tot);
    if (i < T) c[i] = carry + ex;
    carry += tot;
  }
  if (total && threadIdx.x == 0) *total = carry;
}
// a sort pass's counts are digit-major [256][tiles]: workgroup d scans digit d's row over the tiles (coalesced) and leaves the row total in
// totals[d]; the scatter kernel adds the exclusive scan of the 256 totals (done in LDS by every tile: 256 values)
__global__ __launch_bounds__(256) void dsort_digit_scan_kernel(uint32_t *counts, int64_t tiles, uint32_t *totals) {
  __shared__ uint32_t wsum[4];
  uint32_t *c = counts + (int64_t)blockIdx.x * tiles;
  uint32_t carry = 0;
  for (int64_t base = 0; base < tiles; base += 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < tiles ? c[i] : 0u;
    uint32_t tot;
    const uint32_t ex = dsort_block_scan<256>(v, wsum, &tot);
    if (i < tiles) c[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- compaction: out[k] = in[i] (or i itself when in == nullptr) for the k-th set flag, in index order; a second (in2, out2) pair rides along
template <typename A, typename B>
__global__ __launch_bounds__(DSORT_TB) void dsel_count_kernel(const uint8_t *flag, int64_t n, uint32_t *counts) {
  __shared__ uint32_t wsum[DSORT_TB / 64];
  const int64_t base = (int64_t)blockIdx.x * DSORT_TILE;
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < DSORT_ITEMS; e++) {
    const int64_t i = base + e * DSORT_TB + threadIdx.x;
    c += (i < n && flag[i]) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
template <typename A, typename B>
__global__ __launch_bounds__(DSORT_TB) void dsel_scatter_kernel(const A *in, const B *in2, const uint8_t *flag, int64_t n, const uint32_t *offs, A *out, B *out2) {
  __shared__ uint32_t wcnt[DSORT_TB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * DSORT_TILE;
  uint32_t run = offs[blockIdx.x];
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int e = 0; e < DSORT_ITEMS; e++) {
    const int64_t i = base + e * DSORT_TB + threadIdx.x;
    const bool f = i < n && flag[i];
    const unsigned long long m = __ballot(f);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < DSORT_TB / 64; w++) { const uint32_t v = wcnt[w]; before += w < wave ? v : 0u; tot += v; }
    if (f) {
      const uint32_t k = run + before + (uint32_t)__popcll(m & below);
      if constexpr (!std::is_same<A, void>::value) out[k] = in ? in[i] : (A)i;
      if constexpr (!std::is_same<B, char>::value) out2[k] = in2[i];
    }
    run += tot;
    __syncthreads();
  }
}
// in == nullptr: the indices themselves (a counting iterator).  d_count receives the number selected (unsigned long long, on the device).
template <typename A, typename B = char>
static hipError_t dev_select_flagged(hipStream_t st, const A *in, const B *in2, const uint8_t *flag, A *out, B *out2, unsigned long long *d_count, int64_t n,
                                     uint32_t *scratch) {
  if (n <= 0) return hipMemsetAsync(d_count, 0, 8, st);
  const int64_t tiles = (n + DSORT_TILE - 1) / DSORT_TILE;
  hipError_t e = launch_on(st, dsel_count_kernel<A, B>, dim3((unsigned)tiles), dim3(DSORT_TB), 0, flag, n, scratch);
  if (e == hipSuccess) e = launch_on(st, dsort_scan_kernel, dim3(1), dim3(1024), 0, scratch, tiles, d_count);
  if (e == hipSuccess) e = launch_on(st, dsel_scatter_kernel<A, B>, dim3((unsigned)tiles), dim3(DSORT_TB), 0, in, in2, flag, n, scratch, out, out2);
  return e;
}

// ---- radix sort, 8 bits per pass
__device__ __forceinline__ unsigned long long dsort_peers(unsigned digit, bool valid) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const unsigned long long m = __ballot((digit >> b) & 1u);
    peers &= ((digit >> b) & 1u) ? m : ~m;
  }
  return peers;
}
__global__ __launch_bounds__(DSORT_TB) void dsort_hist_kernel(const unsigned long long *keys, int64_t n, int shift, unsigned mask, int64_t tiles, uint32_t *counts) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)blockIdx.x * DSORT_TILE;
  for (int e = 0; e < DSORT_ITEMS; e++) {
    const int64_t i = base + e * DSORT_TB + threadIdx.x;
    const bool valid = i < n;
    const unsigned d = valid ? (unsigned)(keys[i] >> shift) & mask : 0u;
    const unsigned long long peers = dsort_peers(d, valid);
    if (valid && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&hist[d], (uint32_t)__popcll(peers));     // the lowest peer adds for all
  }
  __syncthreads();
  counts[(int64_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];          // digit-major: the scan order of a stable pass
}
__global__ __launch_bounds__(DSORT_TB) void dsort_scatter_kernel(const unsigned long long *keys, const int32_t *vals, int64_t n, int shift, unsigned mask, int64_t tiles,
                                                                 const uint32_t *offs, const uint32_t *totals, unsigned long long *okeys, int32_t *ovals) {
  __shared__ uint32_t base_[256];
  __shared__ uint32_t wcnt[DSORT_TB / 64][256];
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    uint32_t tot;
    const uint32_t dbase = dsort_block_scan<256>(totals[threadIdx.x], wsum, &tot);        // keys with smaller digits, whole array
    base_[threadIdx.x] = dbase + offs[(int64_t)threadIdx.x * tiles + blockIdx.x];          // + this digit's keys in earlier tiles
  }
#pragma unroll
  for (int w = 0; w < DSORT_TB / 64; w++) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  const int64_t tb = (int64_t)blockIdx.x * DSORT_TILE;
  for (int e = 0; e < DSORT_ITEMS; e++) {
    const int64_t i = tb + e * DSORT_TB + threadIdx.x;
    const bool valid = i < n;
    const unsigned long long k = valid ? keys[i] : 0ull;
    const int32_t v = valid ? vals[i] : 0;
    const unsigned d = valid ? (unsigned)(k >> shift) & mask : 0u;
    const unsigned long long peers = dsort_peers(d, valid);
    const unsigned long long lower = peers & ((1ull << lane) - 1);
    if (valid && lower == 0) wcnt[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t pos = base_[d] + (uint32_t)__popcll(lower);
#pragma unroll
      for (int w = 0; w < DSORT_TB / 64; w++) pos += w < wave ? wcnt[w][d] : 0u;
      okeys[pos] = k; ovals[pos] = v;
    }
    __syncthreads();
    {                                              // thread d advances digit d's base and clears the round's counts
      uint32_t t = 0;
#pragma unroll
      for (int w = 0; w < DSORT_TB / 64; w++) { t += wcnt[w][threadIdx.x]; wcnt[w][threadIdx.x] = 0; }
      base_[threadIdx.x] += t;
    }
    __syncthreads();
  }
}
// Stable sort of m pairs by key bits [begin_bit, end_bit), ping-ponging between (k0, v0) — the input — and (k1, v1); both pairs are
// clobbered.  Returns (through *where) 0 or 1: the pair that holds the sorted result.
static hipError_t dev_radix_sort_pairs(hipStream_t st, unsigned long long *k0, int32_t *v0, unsigned long long *k1, int32_t *v1, int64_t m, int begin_bit, int end_bit,
                                       uint32_t *scratch, int *where) {
  *where = 0;
  if (m <= 1 || end_bit <= begin_bit) return hipSuccess;
  const int64_t tiles = (m + DSORT_TILE - 1) / DSORT_TILE;
  unsigned long long *ks[2] = {k0, k1};
  int32_t *vs[2] = {v0, v1};
  int cur = 0;
  for (int shift = begin_bit; shift < end_bit; shift += 8) {
    const int bits = end_bit - shift < 8 ? end_bit - shift : 8;
    const unsigned mask = (1u << bits) - 1u;
    hipError_t e = launch_on(st, dsort_hist_kernel, dim3((unsigned)tiles), dim3(DSORT_TB), 0, ks[cur], m, shift, mask, tiles, scratch);
    if (e == hipSuccess) e = launch_on(st, dsort_digit_scan_kernel, dim3(256), dim3(256), 0, scratch, tiles, scratch + 256 * tiles);
    if (e == hipSuccess)
      e = launch_on(st, dsort_scatter_kernel, dim3((unsigned)tiles), dim3(DSORT_TB), 0, ks[cur], vs[cur], m, shift, mask, tiles, scratch, scratch + 256 * tiles,
                    ks[cur ^ 1], vs[cur ^ 1]);
    if (e != hipSuccess) return e;
    cur ^= 1;
  }
  *where = cur;
  return hipSuccess;
}
