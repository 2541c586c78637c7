// TDMClusterTree on the device: the balanced recursive 2-means tree rebuild (tdm/.../cluster/RecursiveCluster.scala:34-60,141-198,
// ForkJoinProcess.scala).  The reference fits smile's KMeans(k = 2) node by node on a fork-join pool; here a whole LEVEL of the tree
// is one batched problem.
//
//   * The items live in a permutation array whose contiguous segments are the nodes of the current level.  Every split is
//     n/2 | n - n/2 (balanceTree), so the segment offsets of every level follow from n alone (host, cl_level_sizes).
//   * Streaming levels (segments larger than ClCut<EP>::items): one Lloyd iteration of ALL restarts of ALL segments is one pass
//     over the embeddings (cl_lloyd_tile_kernel): a tile of <= 1 024 positions of one segment is scored against that segment's
//     2R centroids with the item's row held in registers, the assignments of all restarts are kept as one bit mask per item, and
//     the per-(restart, cluster) sums are accumulated from the same tile (second read from L2) in fp64.  Per-tile partials are
//     reduced per (segment, restart) in tile order in fp64 (cl_lloyd_reduce_kernel): no floating-point atomics anywhere, the
//     result is a pure function of (embeddings, seed).  Converged restarts are skipped by both kernels.
//   * k-means++ seeding per (node, restart): first seed uniform, second with probability proportional to D^2, drawn from the
//     sampler's counter RNG keyed by (seed, node code, restart).
//   * After the last iteration the best restart (lowest distortion, lowest index on ties) is taken, every item's squared distance
//     to its centroid 0 — the cluster seeded FIRST; smile's own cluster order is as arbitrary — is evaluated in fp64 and rounded
//     to f32, and one stable dev_radix_sort_pairs over (segment << 32 | float bits) orders every segment by distance: positions
//     < n/2 of a segment are the left child.  Equal distances keep the parent's order.
//   * LDS levels (cl_lds_subtree_kernel): once a segment fits the LDS one workgroup loads it and finishes its whole subtree
//     there, one wave per node, down to single items; only codes (and the trace) go back to HBM.
//
// This first version scores with plain fp32 FMAs (register-resident rows against LDS-resident centroids), not with MFMA tiles;
// DESIGN.md says what that costs.
//
// Lloyd's rule (both paths, and tests/cluster_ref.py): iteration t assigns every item to the nearer centroid (ties to centroid 0),
// D_t = sum of the squared distances to the assigned centroid, new centroid = mean of its items; an empty cluster is re-seeded
// at the item farthest from the other centroid (lowest position on ties).  A restart stops after iteration t when the summed
// squared movement of its two centroids is <= tol^2, or t >= 2 and |D_{t-1} - D_t| <= tol, or t = max_iter.  Its distortion is D_t.
//
// Input contract: finite float32 rows.  Every comparison above is false for a NaN distance (no farthest item, no rank), so both
// entry points refuse a NaN or an infinity with DM_ERR_INVALID before the first clustering kernel runs: dm_cluster_tree scans the
// host array, dm_cluster_tree_model checks the gathered rows on the device (cl_nonfinite_kernel).
#define CL_TB 256
#define CL_TILE 1024
#define CL_RMAX 32
#define CL_LDS_BYTES (160 * 1024)          // LDS of one gfx950 CU
#define CL_LDS_RESERVE (24 * 1024)         // everything but the rows (index arrays, distances) and head-room for the compiler's own use

// the LDS cut-off: how many rows of EP floats fit, at most one per thread of the workgroup
template <int EP>
struct ClCut {
  static constexpr int fit = (CL_LDS_BYTES - CL_LDS_RESERVE) / (EP * 4);
  static constexpr int items = fit < CL_TB ? fit : CL_TB;
};

struct ClTrace {                    // device mirrors of dm_cluster_trace (null = not wanted)
  float *c0; int32_t *seeds; int32_t *iters; double *distortion; float *dist; int E;
};

struct ClLevel {
  const float *X;                   // [n][EP]
  int64_t n;
  int level, S, T, R, max_iter;
  double tol;
  unsigned long long seed;
  const int32_t *perm;              // [n] position -> row
  const int32_t *seg_off;           // [S + 1]
  const int32_t *tile_seg, *tile_start, *tile_first;   // [T], [T], [S + 1]
  int32_t *seed_item;               // [S][R][2]
  float *cent;                      // [S][R][2][EP]
  uint8_t *act;                     // [S][R]
  int32_t *iters;                   // [S][R]
  double *dprev, *dfin;             // [S][R]
  float *d2;                        // [R][n] by position (seeding)
  double *part_sum;                 // [T][R][2][EP]
  int32_t *part_cnt1;               // [T][R]
  double *part_dist;                // [T][R]
  float *part_far_d; int32_t *part_far_p;   // [T][R]
  int32_t *any_active;
  int32_t *best;                    // [S]
  float *bestc0;                    // [S][EP]
  unsigned long long *keys; int32_t *vals;
  ClTrace tr;
};

__device__ __forceinline__ double cl_uniform(unsigned long long seed, int64_t node, int restart, unsigned long long ctr) {
  return (double)(dm_sample_draw(seed, node, restart, ctr, 9) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ int cl_first_seed(unsigned long long seed, int64_t node, int restart, int size) {
  const int p = (int)(cl_uniform(seed, node, restart, 0) * (double)size);
  return p < size ? p : size - 1;
}
__device__ __forceinline__ float cl_wave_sum_f(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double cl_wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void cl_iota_kernel(int32_t *p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = (int32_t)i;
}
// rows of a table (row stride `stride`, first `cols` columns) at the given row numbers -> out [n][ocols], zero beyond `cols`
__global__ void cl_gather_rows_kernel(const float *tab, int stride, int cols, const int32_t *rows, int64_t n, int ocols, float *out) {
  const int64_t tot = n * ocols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ocols; const int e = (int)(i % ocols);
    out[i] = e < cols ? tab[(int64_t)rows[r] * stride + e] : 0.f;
  }
}

// lowest row of X [n][cols] that holds a NaN or an infinity -> *first (the caller sets it to INT32_MAX: no such row)
__global__ void cl_nonfinite_kernel(const float *X, int64_t n, int cols, int32_t *first) {
  const int64_t tot = n * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x)
    if ((__float_as_uint(X[i]) & 0x7f800000u) == 0x7f800000u) atomicMin(first, (int32_t)(i / cols));
}

// ---- seeding -----------------------------------------------------------------------------------------------------------------
// first seed of every (segment, restart): uniform position; its row becomes centroid 0.  One 64-lane block per (segment, restart).
template <int EP>
__global__ __launch_bounds__(64) void cl_seed0_kernel(ClLevel L) {
  const int s = blockIdx.x / L.R, r = blockIdx.x % L.R;
  const int base = L.seg_off[s], size = L.seg_off[s + 1] - base;
  const int64_t node = (((int64_t)1 << L.level) - 1) + s;
  const int32_t item = L.perm[base + cl_first_seed(L.seed, node, r, size)];
  float *c = L.cent + ((size_t)blockIdx.x * 2) * EP;
  for (int e = threadIdx.x; e < EP; e += 64) c[e] = L.X[(size_t)item * EP + e];
  if (threadIdx.x == 0) { L.seed_item[(size_t)blockIdx.x * 2] = item; L.act[blockIdx.x] = 1; L.iters[blockIdx.x] = 0; L.dprev[blockIdx.x] = 0.0; L.dfin[blockIdx.x] = 0.0; }
}

template <int EP>
__device__ __forceinline__ void cl_load_row(const float *X, int32_t item, bool valid, float (&x)[EP]) {
  if (valid) {
    const float4 *row = (const float4 *)(X + (size_t)item * EP);
#pragma unroll
    for (int q = 0; q < EP / 4; q++) { const float4 v = row[q]; x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w; }
  } else {
#pragma unroll
    for (int e = 0; e < EP; e++) x[e] = 0.f;
  }
}

// D^2 of every item to the first seed of each restart of its segment: d2[r][position]
template <int EP>
__global__ __launch_bounds__(CL_TB) void cl_seed_dist_kernel(ClLevel L) {
  __shared__ __attribute__((aligned(16))) float cs[CL_RMAX * EP];
  const int tile = blockIdx.x, s = L.tile_seg[tile], start = L.tile_start[tile];
  const int seg_end = L.seg_off[s + 1], end = start + CL_TILE < seg_end ? start + CL_TILE : seg_end;
  const int R = L.R;
  for (int i = threadIdx.x; i < R * EP; i += CL_TB) cs[i] = L.cent[(((size_t)s * R + i / EP) * 2) * EP + i % EP];
  __syncthreads();
  for (int sub = 0; sub < CL_TILE / CL_TB; sub++) {
    const int pos = start + sub * CL_TB + threadIdx.x;
    const bool valid = pos < end;
    float x[EP];
    cl_load_row<EP>(L.X, valid ? L.perm[pos] : 0, valid, x);
    for (int r = 0; r < R; r++) {
      const float *c = cs + r * EP;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < EP; e++) { const float t = x[e] - c[e]; d = fmaf(t, t, d); }
      if (valid) L.d2[(size_t)r * L.n + pos] = d;
    }
  }
}

// second seed of every (segment, restart): position drawn with probability proportional to d2, by a fixed-order fp64 scan
// (256 chunk sums, then a walk inside the chosen chunk).  All-zero distances (every item on the first seed): the next position.
template <int EP>
__global__ __launch_bounds__(CL_TB) void cl_seed_pick_kernel(ClLevel L) {
  __shared__ double csum[CL_TB];
  __shared__ int pick_s;
  const int s = blockIdx.x / L.R, r = blockIdx.x % L.R;
  const int base = L.seg_off[s], size = L.seg_off[s + 1] - base;
  const float *d2 = L.d2 + (size_t)r * L.n + base;
  const int chunk = (size + CL_TB - 1) / CL_TB;
  const int lo = min((int)threadIdx.x * chunk, size), hi = min(lo + chunk, size);
  double sum = 0.0;
  for (int i = lo; i < hi; i++) sum += (double)d2[i];
  csum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t node = (((int64_t)1 << L.level) - 1) + s;
    double total = 0.0;
    for (int c = 0; c < CL_TB; c++) total += csum[c];
    int pick;
    if (!(total > 0.0)) pick = (cl_first_seed(L.seed, node, r, size) + 1) % size;
    else {
      const double target = cl_uniform(L.seed, node, r, 1) * total;
      double cum = 0.0;
      int c = 0, last = 0;
      for (; c < CL_TB; c++) { if (csum[c] > 0.0) last = c; if (cum + csum[c] > target) break; cum += csum[c]; }
      if (c >= CL_TB) { c = last; cum = 0.0; for (int k = 0; k < c; k++) cum += csum[k]; }
      const int clo = min(c * chunk, size), chi = min(clo + chunk, size);
      pick = -1;
      int lastpos = clo;
      for (int i = clo; i < chi; i++) {
        const double d = (double)d2[i];
        if (d > 0.0) lastpos = i;
        cum += d;
        if (cum > target) { pick = i; break; }
      }
      if (pick < 0) pick = lastpos;
    }
    pick_s = pick;
  }
  __syncthreads();
  const int32_t item = L.perm[base + pick_s];
  float *c = L.cent + ((size_t)blockIdx.x * 2 + 1) * EP;
  for (int e = threadIdx.x; e < EP; e += CL_TB) c[e] = L.X[(size_t)item * EP + e];
  if (threadIdx.x == 0) L.seed_item[(size_t)blockIdx.x * 2 + 1] = item;
}

// ---- one Lloyd iteration: tile pass ------------------------------------------------------------------------------------------
template <int EP>
__global__ __launch_bounds__(CL_TB) void cl_lloyd_tile_kernel(ClLevel L) {
  __shared__ __attribute__((aligned(16))) float cs[CL_RMAX * 2 * EP];
  __shared__ uint32_t abits[CL_TILE];
  __shared__ int32_t tperm[CL_TILE];
  __shared__ double wdist[CL_TB / 64][CL_RMAX];
  __shared__ int wcnt[CL_TB / 64][CL_RMAX];
  __shared__ float wfar_d[CL_TB / 64][CL_RMAX];
  __shared__ int wfar_p[CL_TB / 64][CL_RMAX];
  const int tile = blockIdx.x, s = L.tile_seg[tile], start = L.tile_start[tile];
  const int seg_end = L.seg_off[s + 1], end = start + CL_TILE < seg_end ? start + CL_TILE : seg_end;
  const int R = L.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t amask = 0;
  for (int r = 0; r < R; r++) amask |= L.act[(size_t)s * R + r] ? 1u << r : 0u;
  if (amask == 0) return;                                   // every restart of this segment has converged
  for (int i = tid; i < R * 2 * EP; i += CL_TB) cs[i] = L.cent[(size_t)s * R * 2 * EP + i];
  for (int i = tid; i < CL_TILE; i += CL_TB) tperm[i] = start + i < end ? L.perm[start + i] : 0;
  if (tid < (CL_TB / 64) * CL_RMAX) { (&wdist[0][0])[tid] = 0.0; (&wcnt[0][0])[tid] = 0; (&wfar_d[0][0])[tid] = -1.f; (&wfar_p[0][0])[tid] = 0x7fffffff; }
  __syncthreads();
  // phase 1: assignments of every restart, the row in registers
  for (int sub = 0; sub < CL_TILE / CL_TB; sub++) {
    const int pos = start + sub * CL_TB + tid;
    const bool valid = pos < end;
    float x[EP];
    cl_load_row<EP>(L.X, tperm[sub * CL_TB + tid], valid, x);
    uint32_t bits = 0;
    for (int r = 0; r < R; r++) {
      if (!((amask >> r) & 1u)) continue;
      const float *c0 = cs + (size_t)(2 * r) * EP, *c1 = c0 + EP;
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int e = 0; e < EP; e++) {
        const float t0 = x[e] - c0[e], t1 = x[e] - c1[e];
        d0 = fmaf(t0, t0, d0); d1 = fmaf(t1, t1, d1);
      }
      const bool a = d1 < d0;                               // ties to centroid 0
      const float dm = a ? d1 : d0;
      bits |= a ? 1u << r : 0u;
      const double ds = cl_wave_sum_d(valid ? (double)dm : 0.0);
      const int c1n = (int)__popcll(__ballot(valid && a));
      float fd = valid ? dm : -1.f;
      int fp = valid ? pos : 0x7fffffff;
      for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(fd, o); const int op = __shfl_xor(fp, o);
        if (od > fd || (od == fd && op < fp)) { fd = od; fp = op; }
      }
      if (lane == 0) {
        wdist[wave][r] += ds; wcnt[wave][r] += c1n;
        if (fd > wfar_d[wave][r]) { wfar_d[wave][r] = fd; wfar_p[wave][r] = fp; }      // later rounds hold later positions: > keeps the first
      }
    }
    abits[sub * CL_TB + tid] = bits;
  }
  __syncthreads();
  if (tid < R && ((amask >> tid) & 1u)) {
    double pd = 0.0; int pc = 0; float fd = -1.f; int fp = 0x7fffffff;
    for (int w = 0; w < CL_TB / 64; w++) {
      pd += wdist[w][tid]; pc += wcnt[w][tid];
      if (wfar_d[w][tid] > fd || (wfar_d[w][tid] == fd && wfar_p[w][tid] < fp)) { fd = wfar_d[w][tid]; fp = wfar_p[w][tid]; }
    }
    const size_t o = (size_t)tile * R + tid;
    L.part_dist[o] = pd; L.part_cnt1[o] = pc; L.part_far_d[o] = fd; L.part_far_p[o] = fp;
  }
  // phase 2: per-(restart, cluster) sums of the tile, one column per thread, the restarts dealt round-robin to the G thread groups
  constexpr int G = CL_TB / EP, Q = (CL_RMAX + G - 1) / G;
  const int g = tid / EP, e = tid % EP;
  double a0[Q], a1[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) { a0[q] = 0.0; a1[q] = 0.0; }
  const int cnt = end - start;
#pragma unroll 4
  for (int i = 0; i < cnt; i++) {
    const double xv = (double)L.X[(size_t)tperm[i] * EP + e];
    const uint32_t b = abits[i];
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int r = g + q * G;
      if (r < R) {
        const bool k = (b >> r) & 1u;
        a0[q] += k ? 0.0 : xv; a1[q] += k ? xv : 0.0;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int r = g + q * G;
    if (r < R && ((amask >> r) & 1u)) {
      double *o = L.part_sum + (((size_t)tile * R + r) * 2) * EP + e;
      o[0] = a0[q]; o[EP] = a1[q];
    }
  }
}

// ---- one Lloyd iteration: ordered reduce and centroid update, one workgroup per (segment, restart) ------------------------------
template <int EP>
__global__ __launch_bounds__(CL_TB) void cl_lloyd_reduce_kernel(ClLevel L) {
  constexpr int G = CL_TB / EP;
  __shared__ double red[2][G][EP];
  __shared__ double dsh[CL_TB];
  __shared__ int csh[CL_TB];
  __shared__ float fdsh[CL_TB];
  __shared__ int fpsh[CL_TB];
  __shared__ double tot_dist;
  __shared__ int tot_c1, far_pos;
  if (!L.act[blockIdx.x]) return;
  const int s = blockIdx.x / L.R, r = blockIdx.x % L.R, R = L.R, tid = threadIdx.x;
  const int t0 = L.tile_first[s], t1 = L.tile_first[s + 1];
  const int g = tid / EP, e = tid % EP;
  double s0 = 0.0, s1 = 0.0;
  for (int t = t0 + g; t < t1; t += G) {
    const double *p = L.part_sum + (((size_t)t * R + r) * 2) * EP + e;
    s0 += p[0]; s1 += p[EP];
  }
  red[0][g][e] = s0; red[1][g][e] = s1;
  double pd = 0.0; int pc = 0; float fd = -1.f; int fp = 0x7fffffff;
  for (int t = t0 + tid; t < t1; t += CL_TB) {
    const size_t o = (size_t)t * R + r;
    pd += L.part_dist[o]; pc += L.part_cnt1[o];
    const float od = L.part_far_d[o]; const int op = L.part_far_p[o];
    if (od > fd || (od == fd && op < fp)) { fd = od; fp = op; }
  }
  dsh[tid] = pd; csh[tid] = pc; fdsh[tid] = fd; fpsh[tid] = fp;
  __syncthreads();
  if (tid == 0) {
    double D = 0.0; int c1 = 0; float bd = -1.f; int bp = 0x7fffffff;
    for (int i = 0; i < CL_TB; i++) {
      D += dsh[i]; c1 += csh[i];
      if (fdsh[i] > bd || (fdsh[i] == bd && fpsh[i] < bp)) { bd = fdsh[i]; bp = fpsh[i]; }
    }
    // no farthest item was found (no distance compared greater than -1: non-finite rows, which the entry points refuse): the
    // segment's first position, so that the sentinel can never become an address
    const int sb = L.seg_off[s], se = L.seg_off[s + 1];
    tot_dist = D; tot_c1 = c1; far_pos = bp >= sb && bp < se ? bp : sb;
  }
  __syncthreads();
  const int size = L.seg_off[s + 1] - L.seg_off[s];
  const int n1 = tot_c1, n0 = size - n1;
  double mv = 0.0;
  if (tid < EP) {
    double u0 = 0.0, u1 = 0.0;
    for (int k = 0; k < G; k++) { u0 += red[0][k][tid]; u1 += red[1][k][tid]; }
    float *c = L.cent + ((size_t)blockIdx.x * 2) * EP;
    const float far = L.X[(size_t)L.perm[far_pos] * EP + tid];
    const float n0c = n0 > 0 ? (float)(u0 / (double)n0) : far;
    const float n1c = n1 > 0 ? (float)(u1 / (double)n1) : far;
    const double m0 = (double)n0c - (double)c[tid], m1 = (double)n1c - (double)c[EP + tid];
    mv = m0 * m0 + m1 * m1;
    c[tid] = n0c; c[EP + tid] = n1c;
  }
  __syncthreads();
  dsh[tid] = mv;
  __syncthreads();
  if (tid == 0) {
    double moved = 0.0;
    for (int i = 0; i < EP; i++) moved += dsh[i];
    const int it = ++L.iters[blockIdx.x];
    const double D = tot_dist;
    const bool conv = moved <= L.tol * L.tol || (it >= 2 && fabs(L.dprev[blockIdx.x] - D) <= L.tol) || it >= L.max_iter;
    L.dprev[blockIdx.x] = D; L.dfin[blockIdx.x] = D;
    if (conv) L.act[blockIdx.x] = 0; else *L.any_active = 1;
  }
}

// best restart of every segment, its centroid 0, the trace rows of the node
template <int EP>
__global__ void cl_best_kernel(ClLevel L) {
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < L.S; s += gridDim.x * blockDim.x) {
    int b = 0;
    for (int r = 1; r < L.R; r++) if (L.dfin[(size_t)s * L.R + r] < L.dfin[(size_t)s * L.R + b]) b = r;
    L.best[s] = b;
    const float *c = L.cent + (((size_t)s * L.R + b) * 2) * EP;
    for (int e = 0; e < EP; e++) L.bestc0[(size_t)s * EP + e] = c[e];
    const int64_t node = (((int64_t)1 << L.level) - 1) + s;
    if (L.tr.c0) for (int e = 0; e < L.tr.E; e++) L.tr.c0[node * L.tr.E + e] = c[e];
    if (L.tr.seeds) { L.tr.seeds[node * 2] = L.seed_item[((size_t)s * L.R + b) * 2]; L.tr.seeds[node * 2 + 1] = L.seed_item[((size_t)s * L.R + b) * 2 + 1]; }
    if (L.tr.iters) L.tr.iters[node] = L.iters[(size_t)s * L.R + b];
    if (L.tr.distortion) L.tr.distortion[node] = L.dfin[(size_t)s * L.R + b];
  }
}

// squared distance to the best restart's centroid 0 in fp64, rounded to f32 -> the sort key (segment << 32 | float bits)
template <int EP>
__global__ __launch_bounds__(CL_TB) void cl_dist_key_kernel(ClLevel L) {
  __shared__ __attribute__((aligned(16))) float c[EP];
  const int tile = blockIdx.x, s = L.tile_seg[tile], start = L.tile_start[tile];
  const int seg_end = L.seg_off[s + 1], end = start + CL_TILE < seg_end ? start + CL_TILE : seg_end;
  for (int i = threadIdx.x; i < EP; i += CL_TB) c[i] = L.bestc0[(size_t)s * EP + i];
  __syncthreads();
  for (int sub = 0; sub < CL_TILE / CL_TB; sub++) {
    const int pos = start + sub * CL_TB + threadIdx.x;
    if (pos >= end) continue;
    const int32_t item = L.perm[pos];
    float x[EP];
    cl_load_row<EP>(L.X, item, true, x);
    double d = 0.0;
#pragma unroll
    for (int e = 0; e < EP; e++) { const double t = (double)x[e] - (double)c[e]; d = fma(t, t, d); }
    const float df = (float)d;
    L.keys[pos] = ((unsigned long long)(unsigned)s << 32) | (unsigned long long)__float_as_uint(df);
    L.vals[pos] = item;
    if (L.tr.dist) L.tr.dist[(size_t)L.level * L.n + item] = df;
  }
}

// ---- the LDS subtree ---------------------------------------------------------------------------------------------------------
// (start, size) of node k of sub-level d below a segment of m items, and the size of its parent
__device__ __forceinline__ void cl_node_range(int m, int d, int k, int *st, int *sz, int *psz) {
  int s0 = 0, n = m, p = 2;
  for (int b = d - 1; b >= 0; b--) {
    p = n;
    const int l = n >> 1;
    if ((k >> b) & 1) { s0 += l; n -= l; } else n = l;
  }
  *st = s0; *sz = n; *psz = p;
}

struct ClLds {
  const float *X; int64_t n;
  int level, S, R, max_iter;
  double tol;
  unsigned long long seed;
  int32_t *perm;                    // [n]: read, and rewritten with the final order
  const int32_t *seg_off;           // [S + 1]
  int32_t *codes;                   // [n] by row
  ClTrace tr;
};

template <int EP>
__global__ __launch_bounds__(CL_TB) void cl_lds_subtree_kernel(ClLds P) {
  constexpr int CUT = ClCut<EP>::items;
  constexpr int NE = (EP + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char cl_smem[];
  float *xs = (float *)cl_smem;                                   // [CUT][EP]
  int32_t *gitem = (int32_t *)(xs + (size_t)CUT * EP);            // [CUT] row number of local item
  float *dbuf = (float *)(gitem + CUT);                           // [CUT] by position
  int16_t *lp0 = (int16_t *)(dbuf + CUT), *lp1 = lp0 + CUT;       // [CUT] position -> local item, double-buffered
  const int seg = blockIdx.x, base = P.seg_off[seg], m = P.seg_off[seg + 1] - base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (m > CUT) return;                                            // (the host never launches this: a segment must fit)
  for (int i = tid; i < m; i += CL_TB) { gitem[i] = P.perm[base + i]; lp0[i] = (int16_t)i; lp1[i] = (int16_t)i; }
  for (int idx = tid; idx < m * EP; idx += CL_TB) xs[idx] = P.X[(size_t)P.perm[base + idx / EP] * EP + idx % EP];
  __syncthreads();
  int16_t *lp = lp0, *lq = lp1;
  for (int d = 0; d < 31; d++) {
    int maxsz = m;
    for (int b = 0; b < d; b++) maxsz -= maxsz >> 1;
    for (int k = wave; k < (1 << d); k += CL_TB / 64) {
      int st, sz, psz;
      cl_node_range(m, d, k, &st, &sz, &psz);
      if (sz <= 0) continue;
      if (psz <= 1) { if (lane == 0) lq[st] = lp[st]; continue; }   // below a leaf: it keeps the code it has
      const int64_t node = (((int64_t)1 << (P.level + d)) - 1) + ((int64_t)seg << d) + k;
      if (sz == 1) {
        if (lane == 0) { P.codes[gitem[lp[st]]] = (int32_t)node; lq[st] = lp[st]; }
        continue;
      }
      if (sz == 2) {                                               // idx(0) left, idx(1) right
        if (lane < 2) lq[st + lane] = lp[st + lane];
        continue;
      }
      float c0[NE], c1[NE], bc0[NE];
      double bestD = 0.0; int bs0 = -1, bs1 = -1, bit = 0; bool have = false;
      for (int r = 0; r < P.R; r++) {
        const int p0 = cl_first_seed(P.seed, node, r, sz);
        {
          const int li = lp[st + p0];
#pragma unroll
          for (int j = 0; j < NE; j++) { const int e = lane + 64 * j; c0[j] = e < EP ? xs[li * EP + e] : 0.f; }
        }
        double tot = 0.0;
        for (int i = 0; i < sz; i++) {
          const int li = lp[st + i];
          float part = 0.f;
#pragma unroll
          for (int j = 0; j < NE; j++) { const int e = lane + 64 * j; const float t = (e < EP ? xs[li * EP + e] : 0.f) - c0[j]; part = fmaf(t, t, part); }
          const float dd = cl_wave_sum_f(part);
          if (lane == 0) dbuf[st + i] = dd;
          tot += (double)dd;
        }
        __builtin_amdgcn_wave_barrier();
        int p1;
        if (!(tot > 0.0)) p1 = (p0 + 1) % sz;
        else {
          const double target = cl_uniform(P.seed, node, r, 1) * tot;
          double cum = 0.0;
          int lastpos = 0;
          p1 = -1;
          for (int i = 0; i < sz; i++) {
            const double dd = (double)dbuf[st + i];
            if (dd > 0.0) lastpos = i;
            cum += dd;
            if (cum > target) { p1 = i; break; }
          }
          if (p1 < 0) p1 = lastpos;
        }
        __builtin_amdgcn_wave_barrier();
        {
          const int li = lp[st + p1];
#pragma unroll
          for (int j = 0; j < NE; j++) { const int e = lane + 64 * j; c1[j] = e < EP ? xs[li * EP + e] : 0.f; }
        }
        double Dprev = 0.0, D = 0.0;
        int it = 0;
        for (;;) {
          it++;
          double s0[NE], s1[NE];
#pragma unroll
          for (int j = 0; j < NE; j++) { s0[j] = 0.0; s1[j] = 0.0; }
          int n1 = 0, fari = 0;
          float fard = -1.f;
          D = 0.0;
          for (int i = 0; i < sz; i++) {
            const int li = lp[st + i];
            float xr[NE], q0 = 0.f, q1 = 0.f;
#pragma unroll
            for (int j = 0; j < NE; j++) {
              const int e = lane + 64 * j;
              xr[j] = e < EP ? xs[li * EP + e] : 0.f;
              const float t0 = xr[j] - c0[j], t1 = xr[j] - c1[j];
              q0 = fmaf(t0, t0, q0); q1 = fmaf(t1, t1, q1);
            }
            const float d0 = cl_wave_sum_f(q0), d1 = cl_wave_sum_f(q1);
            const bool a = d1 < d0;
            const float dm = a ? d1 : d0;
            D += (double)dm;
            if (dm > fard) { fard = dm; fari = i; }
            if (a) {
              n1++;
#pragma unroll
              for (int j = 0; j < NE; j++) s1[j] += (double)xr[j];
            } else {
#pragma unroll
              for (int j = 0; j < NE; j++) s0[j] += (double)xr[j];
            }
          }
          const int n0 = sz - n1, lf = lp[st + fari];
          double mv = 0.0;
#pragma unroll
          for (int j = 0; j < NE; j++) {
            const int e = lane + 64 * j;
            const float far = e < EP ? xs[lf * EP + e] : 0.f;
            const float n0c = n0 > 0 ? (float)(s0[j] / (double)n0) : far;
            const float n1c = n1 > 0 ? (float)(s1[j] / (double)n1) : far;
            const double m0 = (double)n0c - (double)c0[j], m1 = (double)n1c - (double)c1[j];
            mv += m0 * m0 + m1 * m1;
            c0[j] = n0c; c1[j] = n1c;
          }
          const double moved = cl_wave_sum_d(mv);
          const bool conv = moved <= P.tol * P.tol || (it >= 2 && fabs(Dprev - D) <= P.tol) || it >= P.max_iter;
          Dprev = D;
          if (conv) break;
        }
        if (!have || D < bestD) {
          have = true; bestD = D; bs0 = p0; bs1 = p1; bit = it;
#pragma unroll
          for (int j = 0; j < NE; j++) bc0[j] = c0[j];
        }
      }
      // the split: distance to centroid 0 of the best restart (fp64, rounded to f32), stable rank inside the node
      for (int i = 0; i < sz; i++) {
        const int li = lp[st + i];
        double part = 0.0;
#pragma unroll
        for (int j = 0; j < NE; j++) { const int e = lane + 64 * j; const double t = (double)(e < EP ? xs[li * EP + e] : 0.f) - (double)bc0[j]; part = fma(t, t, part); }
        const float df = (float)cl_wave_sum_d(part);
        if (lane == 0) {
          dbuf[st + i] = df;
          if (P.tr.dist) P.tr.dist[(size_t)(P.level + d) * P.n + gitem[li]] = df;
        }
      }
      if (P.tr.c0) {
#pragma unroll
        for (int j = 0; j < NE; j++) { const int e = lane + 64 * j; if (e < P.tr.E) P.tr.c0[node * P.tr.E + e] = bc0[j]; }
      }
      if (lane == 0) {
        if (P.tr.seeds) { P.tr.seeds[node * 2] = gitem[lp[st + bs0]]; P.tr.seeds[node * 2 + 1] = gitem[lp[st + bs1]]; }
        if (P.tr.iters) P.tr.iters[node] = bit;
        if (P.tr.distortion) P.tr.distortion[node] = bestD;
      }
      __builtin_amdgcn_wave_barrier();
      for (int j = lane; j < sz; j += 64) {
        const float dj = dbuf[st + j];
        int rank = 0;
        for (int i = 0; i < sz; i++) { const float di = dbuf[st + i]; rank += (di < dj || (di == dj && i < j)) ? 1 : 0; }
        lq[st + rank] = lp[st + j];
      }
    }
    __syncthreads();
    { int16_t *t = lp; lp = lq; lq = t; }
    if (maxsz <= 1) break;
  }
  for (int i = tid; i < m; i += CL_TB) P.perm[base + i] = gitem[lp[i]];
}

// ---- host --------------------------------------------------------------------------------------------------------------------
#define CL_GET(ptr, count) do { const int rc_g_ = arena.alloc((ptr), (size_t)(count) * sizeof(*(ptr))); if (rc_g_ != DM_OK) return rc_g_; } while (0)   // device allocations of one call, freed together

static int cl_max_level(int64_t n) { int l = 0; while (((int64_t)1 << l) < n) l++; return l; }
static std::vector<int32_t> cl_level_sizes(int64_t n, int level) {
  std::vector<int32_t> cur{(int32_t)n};
  for (int l = 0; l < level; l++) {
    std::vector<int32_t> nx; nx.reserve(cur.size() * 2);
    for (int32_t s : cur) { nx.push_back(s / 2); nx.push_back(s - s / 2); }
    cur.swap(nx);
  }
  return cur;
}

template <int EP>
static int cluster_run(dm_ctx *h, const float *d_X, int64_t n, int E, int R, int max_iter, double tol, uint64_t seed, int32_t *codes_out,
                       const dm_cluster_trace *trace, dm_cluster_stats *stats) {
  using clk = std::chrono::steady_clock;
  auto secs = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
  dm_cluster_stats st{};
  DevTemps arena(h);
  hipStream_t sm = h->stream;
  const int max_level = cl_max_level(n);
  const int64_t nodes = ((int64_t)1 << max_level) - 1;
  ClTrace tr{};
  tr.E = E;
  if (trace) {
    if ((trace->centroid0 || trace->seeds || trace->iters || trace->distortion) && trace->node_cap < nodes)
      return fail(h, DM_ERR_INVALID, "dm_cluster_tree: trace.node_cap is smaller than 2^max_level - 1");
    if (trace->dist && trace->level_cap < max_level) return fail(h, DM_ERR_INVALID, "dm_cluster_tree: trace.level_cap is smaller than max_level");
    const int64_t nn = nodes > 0 ? nodes : 1;
    if (trace->centroid0) { CL_GET(tr.c0, nn * E); HIPCHK(h, hipMemsetAsync(tr.c0, 0xFF, (size_t)nn * E * 4, sm)); }
    if (trace->seeds) { CL_GET(tr.seeds, nn * 2); HIPCHK(h, hipMemsetAsync(tr.seeds, 0xFF, (size_t)nn * 8, sm)); }
    if (trace->iters) { CL_GET(tr.iters, nn); HIPCHK(h, hipMemsetAsync(tr.iters, 0, (size_t)nn * 4, sm)); }
    if (trace->distortion) { CL_GET(tr.distortion, nn); HIPCHK(h, hipMemsetAsync(tr.distortion, 0xFF, (size_t)nn * 8, sm)); }
    if (trace->dist && max_level > 0) { CL_GET(tr.dist, (int64_t)max_level * n); HIPCHK(h, hipMemsetAsync(tr.dist, 0xFF, (size_t)max_level * n * 4, sm)); }
  }
  int32_t *perm[2] = {nullptr, nullptr}, *d_codes = nullptr;
  unsigned long long *keys[2] = {nullptr, nullptr};
  int rc;
  CL_GET(perm[0], n); CL_GET(perm[1], n); CL_GET(d_codes, n);
  if ((rc = LAUNCH(h, cl_iota_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, perm[0], n)) != DM_OK) return rc;
  HIPCHK(h, hipMemsetAsync(d_codes, 0, (size_t)n * 4, sm));
  int cur = 0, level = 0;
  constexpr int CUT = ClCut<EP>::items;
  const size_t row_bytes = (size_t)n * EP * 4;
  uint32_t *sort_tmp = nullptr;
  for (;; level++) {
    const std::vector<int32_t> sizes = cl_level_sizes(n, level);
    const int S = (int)sizes.size();
    if (*std::max_element(sizes.begin(), sizes.end()) <= CUT) break;
    if (!keys[0]) { CL_GET(keys[0], n); CL_GET(keys[1], n); CL_GET(sort_tmp, dev_sort_scratch_bytes(n) / 4 + 1); }
    const size_t mark = arena.owned.size();
    std::vector<int32_t> seg_off(S + 1, 0), tile_first(S + 1, 0), tile_seg, tile_start;
    for (int s = 0; s < S; s++) {
      seg_off[s + 1] = seg_off[s] + sizes[s];
      tile_first[s] = (int32_t)tile_seg.size();
      for (int32_t p = seg_off[s]; p < seg_off[s + 1]; p += CL_TILE) { tile_seg.push_back(s); tile_start.push_back(p); }
    }
    const int T = (int)tile_seg.size();
    tile_first[S] = T;
    ClLevel L{};
    L.X = d_X; L.n = n; L.level = level; L.S = S; L.T = T; L.R = R; L.max_iter = max_iter; L.tol = tol; L.seed = seed; L.perm = perm[cur]; L.tr = tr;
    int32_t *d_seg_off, *d_tile_seg, *d_tile_start, *d_tile_first;
    CL_GET(d_seg_off, S + 1); CL_GET(d_tile_seg, T); CL_GET(d_tile_start, T); CL_GET(d_tile_first, S + 1);
    HIPCHK(h, hipMemcpyAsync(d_seg_off, seg_off.data(), (size_t)(S + 1) * 4, hipMemcpyHostToDevice, sm));
    HIPCHK(h, hipMemcpyAsync(d_tile_seg, tile_seg.data(), (size_t)T * 4, hipMemcpyHostToDevice, sm));
    HIPCHK(h, hipMemcpyAsync(d_tile_start, tile_start.data(), (size_t)T * 4, hipMemcpyHostToDevice, sm));
    HIPCHK(h, hipMemcpyAsync(d_tile_first, tile_first.data(), (size_t)(S + 1) * 4, hipMemcpyHostToDevice, sm));
    HIPCHK(h, hipStreamSynchronize(sm));                      // (the host vectors are pageable)
    L.seg_off = d_seg_off; L.tile_seg = d_tile_seg; L.tile_start = d_tile_start; L.tile_first = d_tile_first;
    const size_t SR = (size_t)S * R, TR = (size_t)T * R;
    CL_GET(L.seed_item, SR * 2); CL_GET(L.cent, SR * 2 * EP); CL_GET(L.act, SR); CL_GET(L.iters, SR); CL_GET(L.dprev, SR); CL_GET(L.dfin, SR);
    CL_GET(L.d2, (size_t)R * n); CL_GET(L.part_sum, TR * 2 * EP); CL_GET(L.part_cnt1, TR); CL_GET(L.part_dist, TR);
    CL_GET(L.part_far_d, TR); CL_GET(L.part_far_p, TR); CL_GET(L.any_active, 1); CL_GET(L.best, S); CL_GET(L.bestc0, (size_t)S * EP);
    L.keys = keys[0]; L.vals = perm[cur ^ 1];
    // seeding
    auto t0 = clk::now();
    if ((rc = LAUNCH(h, cl_seed0_kernel<EP>, dim3((unsigned)SR), dim3(64), 0, L)) != DM_OK || (rc = LAUNCH(h, cl_seed_dist_kernel<EP>, dim3((unsigned)T), dim3(CL_TB), 0, L)) != DM_OK ||
        (rc = LAUNCH(h, cl_seed_pick_kernel<EP>, dim3((unsigned)SR), dim3(CL_TB), 0, L)) != DM_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(sm));
    st.seeding_s += secs(t0); st.bytes_streamed += (int64_t)row_bytes;
    // Lloyd
    t0 = clk::now();
    for (int it = 0; it < max_iter; it++) {
      HIPCHK(h, hipMemsetAsync(L.any_active, 0, 4, sm));
      if ((rc = LAUNCH(h, cl_lloyd_tile_kernel<EP>, dim3((unsigned)T), dim3(CL_TB), 0, L)) != DM_OK ||
          (rc = LAUNCH(h, cl_lloyd_reduce_kernel<EP>, dim3((unsigned)SR), dim3(CL_TB), 0, L)) != DM_OK) return rc;
      int32_t any = 0;
      HIPCHK(h, hipMemcpyAsync(&any, L.any_active, 4, hipMemcpyDeviceToHost, sm));
      HIPCHK(h, hipStreamSynchronize(sm));
      st.lloyd_passes++; st.bytes_streamed += (int64_t)row_bytes;
      if (!any) break;
    }
    st.lloyd_s += secs(t0);
    // split
    t0 = clk::now();
    if ((rc = LAUNCH(h, cl_best_kernel<EP>, dim3((unsigned)std::min(S / 256 + 1, 1024)), dim3(256), 0, L)) != DM_OK ||
        (rc = LAUNCH(h, cl_dist_key_kernel<EP>, dim3((unsigned)T), dim3(CL_TB), 0, L)) != DM_OK) return rc;
    int sbits = 0;
    while ((1 << sbits) < S) sbits++;
    int where = 0;
    const hipError_t se = dev_radix_sort_pairs(sm, keys[0], perm[cur ^ 1], keys[1], perm[cur], n, 0, 32 + sbits, sort_tmp, &where);
    if (se != hipSuccess) return fail(h, DM_ERR_HIP, std::string("dm_cluster_tree: sort failed: ") + hipGetErrorString(se));
    HIPCHK(h, hipStreamSynchronize(sm));
    // the sorted values are in perm[cur ^ 1] (where == 0) or perm[cur] (where == 1)
    cur = where == 0 ? cur ^ 1 : cur;
    st.split_s += secs(t0); st.bytes_streamed += (int64_t)row_bytes;
    st.levels_streamed++;
    arena.drop_from(mark);
  }
  // the LDS subtree of every segment of this level
  {
    auto t0 = clk::now();
    const std::vector<int32_t> sizes = cl_level_sizes(n, level);
    const int S = (int)sizes.size();
    std::vector<int32_t> seg_off(S + 1, 0);
    for (int s = 0; s < S; s++) seg_off[s + 1] = seg_off[s] + sizes[s];
    int32_t *d_seg_off;
    CL_GET(d_seg_off, S + 1);
    HIPCHK(h, hipMemcpy(d_seg_off, seg_off.data(), (size_t)(S + 1) * 4, hipMemcpyHostToDevice));
    ClLds P{};
    P.X = d_X; P.n = n; P.level = level; P.S = S; P.R = R; P.max_iter = max_iter; P.tol = tol; P.seed = seed; P.perm = perm[cur]; P.seg_off = d_seg_off;
    P.codes = d_codes; P.tr = tr;
    const size_t lds = (size_t)CUT * EP * 4 + (size_t)CUT * (4 + 4 + 2 + 2);
    if ((rc = LAUNCH_LDS(h, cl_lds_subtree_kernel<EP>, dim3((unsigned)S), dim3(CL_TB), lds, P)) != DM_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(sm));
    st.lds_s += secs(t0); st.bytes_streamed += (int64_t)row_bytes;
    st.levels_lds = max_level - level;
  }
  HIPCHK(h, hipMemcpy(codes_out, d_codes, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (trace) {
    if (trace->centroid0) HIPCHK(h, hipMemcpy(trace->centroid0, tr.c0, (size_t)nodes * E * 4, hipMemcpyDeviceToHost));
    if (trace->seeds) HIPCHK(h, hipMemcpy(trace->seeds, tr.seeds, (size_t)nodes * 8, hipMemcpyDeviceToHost));
    if (trace->iters) HIPCHK(h, hipMemcpy(trace->iters, tr.iters, (size_t)nodes * 4, hipMemcpyDeviceToHost));
    if (trace->distortion) HIPCHK(h, hipMemcpy(trace->distortion, tr.distortion, (size_t)nodes * 8, hipMemcpyDeviceToHost));
    if (trace->dist && max_level > 0) HIPCHK(h, hipMemcpy(trace->dist, tr.dist, (size_t)max_level * n * 4, hipMemcpyDeviceToHost));
    if (trace->perm) HIPCHK(h, hipMemcpy(trace->perm, perm[cur], (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  if (stats) *stats = st;
  return DM_OK;
}

static int cluster_dispatch(dm_ctx *h, const float *d_X, int EP, int64_t n, int E, int R, int max_iter, double tol, uint64_t seed, int32_t *codes_out,
                            const dm_cluster_trace *trace, dm_cluster_stats *stats) {
  return dispatch_E(h, EP, "dm_cluster_tree: embed size",
                    [&](auto e) { return cluster_run<decltype(e)::value>(h, d_X, n, E, R, max_iter, tol, seed, codes_out, trace, stats); });
}

static int cluster_check(dm_ctx *h, const char *who, int64_t n, int restarts, int max_iter, double tol, const void *codes_out) {
  if (n < 1 || n > ((int64_t)1 << 30)) return fail(h, DM_ERR_INVALID, std::string(who) + ": n must be 1 .. 2^30 (leaf codes are int32)");
  if (restarts < 1) return fail(h, DM_ERR_INVALID, std::string(who) + ": restarts must be >= 1");
  if (restarts > CL_RMAX) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": at most 32 restarts (one assignment bit per restart and item)");
  if (max_iter < 1 || !(tol >= 0.0)) return fail(h, DM_ERR_INVALID, std::string(who) + ": max_iter must be >= 1 and tol >= 0");
  if (!codes_out) return fail(h, DM_ERR_INVALID, std::string(who) + ": codes_out is null");
  return DM_OK;
}
// n = 1: the reference's degenerate case (code 0), no kernel
static void cluster_single(int32_t *codes_out, const dm_cluster_trace *trace, dm_cluster_stats *stats) {
  codes_out[0] = 0;
  if (trace && trace->perm) trace->perm[0] = 0;
  if (stats) *stats = dm_cluster_stats{};
}

// the finite-input scan of the host array: one pass, branch-free inside a row (an OR of "exponent all ones" over its columns, which
// the compiler vectorises), so it runs at the speed of one core reading memory; -1 = every value finite
static int64_t cluster_first_nonfinite_row(const float *emb, int64_t n, int E) {
  for (int64_t i = 0; i < n; i++) {
    const float *row = emb + i * E;
    uint32_t bad = 0;
    for (int e = 0; e < E; e++) {
      uint32_t u;
      memcpy(&u, row + e, 4);
      bad |= (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    }
    if (bad) return i;
  }
  return -1;
}

int dm_cluster_tree(dm_handle_t h, const float *emb, int64_t n, int E, int restarts, int max_iter, double tol, uint64_t seed, int32_t *codes_out,
                    const dm_cluster_trace *trace, dm_cluster_stats *stats) {
  if (!h) return DM_ERR_INVALID;
  if (!emb) return fail(h, DM_ERR_INVALID, "dm_cluster_tree: emb is null");
  if (E < 1 || E > 128) return fail(h, DM_ERR_UNSUPPORTED, "dm_cluster_tree: embed size must be 1 .. 128");
  const int rc = cluster_check(h, "dm_cluster_tree", n, restarts, max_iter, tol, codes_out);
  if (rc != DM_OK) return rc;
  const int64_t bad_row = cluster_first_nonfinite_row(emb, n, E);
  if (bad_row >= 0) {
    int e = 0;
    while (e < E - 1 && std::isfinite(emb[bad_row * E + e])) e++;
    return fail(h, DM_ERR_INVALID, "dm_cluster_tree: row " + std::to_string(bad_row) + " holds a non-finite value (column " + std::to_string(e) +
                                       "); the embeddings must be finite");
  }
  if (n == 1) { cluster_single(codes_out, trace, stats); return DM_OK; }
  HIPCHK(h, hipSetDevice(h->device));
  const int EP = native_embed(E);
  DevTemps arena(h);
  float *d_X;
  CL_GET(d_X, (size_t)n * EP);
  if (EP != E) HIPCHK(h, hipMemsetAsync(d_X, 0, (size_t)n * EP * 4, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy2D(d_X, (size_t)EP * 4, emb, (size_t)E * 4, (size_t)E * 4, (size_t)n, hipMemcpyHostToDevice));
  return cluster_dispatch(h, d_X, EP, n, E, restarts, max_iter, tol, seed, codes_out, trace, stats);
}

// the loaded table's rows at the items' current leaf codes -> *d_out [n][ocols] on the device
static int cluster_gather_model(dm_ctx *h, const char *who, const int32_t *item_ids, int64_t n, int ocols, DevTemps &arena, float **d_out) {
  if (!h->ids_loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": no tree loaded (item id -> leaf code map)");
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": no weights loaded");
  std::vector<int32_t> codes((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const int32_t id = item_ids[i];
    const int32_t c = id >= 0 && id < h->non_leaf_offset ? h->h_id_to_code[id] : -1;
    if (c < 0) return fail(h, DM_ERR_INVALID, std::string(who) + ": item id " + std::to_string(id) + " is not a leaf of the loaded tree");
    if (c >= h->num_index) return fail(h, DM_ERR_INDEX, std::string(who) + ": leaf code " + std::to_string(c) + " is outside the embedding table");
    codes[i] = c;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (h->dtype == DM_F64) { const int rc = ensure_f32_mirror(h); if (rc != DM_OK) return rc; }
  int32_t *d_rows;
  CL_GET(d_rows, n);
  CL_GET(*d_out, (size_t)n * ocols);
  HIPCHK(h, hipMemcpy(d_rows, codes.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  const int cols = h->embed_log > 0 ? h->embed_log : h->embed;
  const int rc_g = LAUNCH(h, cl_gather_rows_kernel, dim3((unsigned)std::min<int64_t>((n * ocols + 255) / 256, 8192)), dim3(256), 0, h->d_emb32, h->embed, cols, d_rows, n, ocols, *d_out);
  if (rc_g != DM_OK) return rc_g;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_cluster_tree_model(dm_handle_t h, const int32_t *item_ids, int64_t n, int restarts, int max_iter, double tol, uint64_t seed, int32_t *codes_out,
                          const dm_cluster_trace *trace, dm_cluster_stats *stats) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!item_ids) return fail(h, DM_ERR_INVALID, "dm_cluster_tree_model: item_ids is null");
  const int rc = cluster_check(h, "dm_cluster_tree_model", n, restarts, max_iter, tol, codes_out);
  if (rc != DM_OK) return rc;
  DevTemps arena(h);
  float *d_X = nullptr;
  const int rg = cluster_gather_model(h, "dm_cluster_tree_model", item_ids, n, h->embed, arena, &d_X);
  if (rg != DM_OK) return rg;
  {                                                   // the finite-input contract, before any clustering kernel
    int32_t *d_first, first = 0x7fffffff;
    CL_GET(d_first, 1);
    HIPCHK(h, hipMemcpy(d_first, &first, 4, hipMemcpyHostToDevice));
    const int rc_n = LAUNCH(h, cl_nonfinite_kernel, dim3((unsigned)std::min<int64_t>((n * h->embed + 255) / 256, 8192)), dim3(256), 0, d_X, n, h->embed, d_first);
    if (rc_n != DM_OK) return rc_n;
    HIPCHK(h, hipMemcpyAsync(&first, d_first, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (first != 0x7fffffff)
      return fail(h, DM_ERR_INVALID, "dm_cluster_tree_model: row " + std::to_string(first) + " (item id " + std::to_string(item_ids[first]) +
                                         ") holds a non-finite value; the embeddings must be finite");
  }
  if (n == 1) { cluster_single(codes_out, trace, stats); return DM_OK; }
  return cluster_dispatch(h, d_X, h->embed, n, h->embed_log > 0 ? h->embed_log : h->embed, restarts, max_iter, tol, seed, codes_out, trace, stats);
}

int dm_get_leaf_embeddings(dm_handle_t h, const int32_t *item_ids, int64_t n, float *out) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!item_ids || !out || n < 1) return fail(h, DM_ERR_INVALID, "dm_get_leaf_embeddings: bad arguments");
  DevTemps arena(h);
  float *d_X = nullptr;
  const int E = h->embed_log > 0 ? h->embed_log : h->embed;
  const int rg = cluster_gather_model(h, "dm_get_leaf_embeddings", item_ids, n, E, arena, &d_X);
  if (rg != DM_OK) return rg;
  HIPCHK(h, hipMemcpy(out, d_X, (size_t)n * E * 4, hipMemcpyDeviceToHost));
  return DM_OK;
}
