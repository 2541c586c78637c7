// Training step of the DIN scorer (SURVEY.md §8 row A12): one worker's trainBatch
// (tdm/src/main/scala/com/mass/tdm/optim/LocalOptimizer.scala:139-162) = forward, BCEWithLogits
// (scalann/.../nn/BCECriterionWithLogits.scala:28-86), backward of every module, then the dense Adam
// step (scalann/.../optim/Adam.scala:19-73) over the whole compact vector, embedding table included.
//
// Row kernel: same row-fragment layout and transposed products as rows_kernel.hip.inc; the forward is
// recomputed in place, the backward's input-gradient GEMMs use the TRANSPOSED weights as A operand
// (again landing in row-fragment layout), attention backward streams the history rows twice on the
// VALU, embedding gradients are accumulated with float atomics (LookupTable.updateEmbeddings is an
// axpy per index).  Weight gradients (sum over rows of outer products) are formed by a second kernel
// from the per-row vectors this kernel stores (dz, att, dAtt, comb).

// Element-type traits: the kernels below are written once for float (v_mfma_f32_16x16x4_f32) and double
// (v_mfma_f64_16x16x4_f64: the reference trains OTM as DIN[Double], otm/.../model/DIN.scala:12-39, otm/.../optim/
// LocalOptimizer.scala:111-140).  Both MFMAs take A[i][k] / B[k][j] from lane (i or j = l & 15, k = l >> 4); what differs is
// the D layout, i.e. WHICH four features of its row a lane (r, g) holds per 16-feature block:
//   float : D rows 4g + rr      -> features 16 blk + 4 g + t   (contiguous: one 16-byte load / store)
//   double: D rows  g + 4 rr    -> features 16 blk + g + 4 t   (stride 4)
// With the k order of every A fragment following the same map, the output of one product is the operand of the next in both.
template <typename T> struct DmTr;
template <> struct DmTr<float> {
  typedef f32x4 V4;
  static constexpr bool F64 = false;
  static __device__ __forceinline__ int feat(int blk, int g, int t) { return 16 * blk + 4 * g + t; }
  static __device__ __forceinline__ V4 mfma(float a, float b, V4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ V4 load4(const float *row, int blk, int g) { return *(const f32x4 *)(row + 16 * blk + 4 * g); }
  static __device__ __forceinline__ void store4(float *row, int blk, int g, V4 v) { *(f32x4 *)(row + 16 * blk + 4 * g) = v; }
  static __device__ __forceinline__ float xsum(float v) {     // sum over the 4 lanes (g = 0..3) that share a row
    v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (16 << 10)));
    v += __shfl_xor(v, 32);
    return v;
  }
  static __device__ __forceinline__ float sum16(float v) { return dm_sum16(v); }
  static __device__ __forceinline__ float exp_(float x) { return expf(x); }
  static __device__ __forceinline__ float log_(float x) { return logf(x); }
};
template <> struct DmTr<double> {
  typedef f64x4 V4;
  static constexpr bool F64 = true;
  static __device__ __forceinline__ int feat(int blk, int g, int t) { return 16 * blk + g + 4 * t; }
  static __device__ __forceinline__ V4 mfma(double a, double b, V4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ V4 load4(const double *row, int blk, int g) {
    const double *s = row + 16 * blk + g;
    return (V4){s[0], s[4], s[8], s[12]};
  }
  static __device__ __forceinline__ void store4(double *row, int blk, int g, V4 v) {
    double *d = row + 16 * blk + g;
    d[0] = v[0]; d[4] = v[1]; d[8] = v[2]; d[12] = v[3];
  }
  static __device__ __forceinline__ double xsum(double v) { v += dm_xor16_f64(v); v += dm_xor32_f64(v); return v; }
  static __device__ __forceinline__ double sum16(double v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
  }
  static __device__ __forceinline__ double exp_(double x) { return exp(x); }
  static __device__ __forceinline__ double log_(double x) { return log(x); }
};

template <typename T>
struct TrainParamsT {
  typedef typename DmTr<T>::V4 V4;
  const T *emb;
  int64_t num_index;
  const V4 *attA, *w1aA, *w1bA;       // W      rows as A operand  [NT][NJ][64]
  const V4 *attTA, *w1aTA, *w1bTA;    // W^T    rows as A operand  [NT][NJ][64]
  const T *b1, *w2;
  T b2;
  const int32_t *codes, *seqs;
  const unsigned *rowmask;
  const float *labels;         // 0 / 1 (or clipped pseudo targets): float in both arithmetics
  int64_t B;
  int L;
  T inv_B;
  T *grad;                     // compact layout: [emb ; att.W ; l1.W ; l1.b ; l2.W ; l2.b]
  T *DZ, *AT, *DA, *CB;        // [B][E]: dL/dz, attention output, dL/datt, softmax-combined keys
  T *loss_acc;                 // [0] = sum max(x,0)+log(1+exp(-|x|)), [1] = sum x*y
  T *logits;                   // [B]
  T sm_scale;                  // 1 / sqrt(embedSize) of the model (the table may be zero-padded to E)
};
typedef TrainParamsT<float> TrainParams;

// timing experiments (tools/build_probe.sh; wrong results): DM_DBG_TRAIN_NOATOM = no embedding-gradient atomics, DM_DBG_TRAIN_NOSTORE = no
// stores of the four [B][E] intermediates, DM_DBG_TRAIN_NOBWD = no attention backward
#if defined(DM_PROBE_BUILD) && defined(DM_DBG_TRAIN_NOATOM)
#define DM_TR_ATOM(addr, v) do { asm volatile("" :: "v"(v)); } while (0)
#else
#define DM_TR_ATOM(addr, v) atomicAdd(addr, v)
#endif
#if defined(DM_PROBE_BUILD) && defined(DM_DBG_TRAIN_NOSTORE)
#define DM_TR_LIVE(x) false
#else
#define DM_TR_LIVE(x) (x)
#endif
// ML = history positions the loops are unrolled for: 16 (the configs' L = 10), or 32 for histories of 17 .. 32 positions (a second
// instantiation: the two per-position register arrays of the backward pass double)
// FWD = true: the forward half only (logits to p.logits, nothing else written, labels / gradients never touched) — round 6: the fp64 OTM
// pseudo-target forwards (O/tree/OTMTree.scala:131-165) ran on the one-wave-per-row scalar kernel of dm_din_forward, 34 M rows/s.
template <typename T, int E, int ML, bool FWD = false>
__global__ __launch_bounds__(DmTr<T>::F64 ? 256 : DM_BLOCK, DmTr<T>::F64 ? 1 : 2) void dm_train_rows_kernel(TrainParamsT<T> p) {
  typedef DmTr<T> TR;
  typedef typename TR::V4 V4;
  constexpr int NJ = E / 16, NT = E / 16;
  extern __shared__ __attribute__((aligned(16))) char smem_t[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwaves = blockDim.x >> 6;
  // float: att.W and W1b fragments staged in LDS once (2 E^2 floats), the other four matrices read through L2.
  // double: ONE E x E matrix at a time in LDS (128 KB at E = 128), re-staged by the whole workgroup before each of the six products of a
  // tile round (round 4).  Read straight from L2, every wave streamed 768 KB of fragments per tile (157 GB per 3.3 M-row launch) with each
  // group of four MFMAs waiting on its own load: 75 % of a wave's time was SQ_WAIT_ANY at 9 % matrix-pipe utilisation
  // (profiles/r04_otmtrain_summary.json).  The four waves of a workgroup now walk their tiles in lock step.
  const V4 *AttA = p.attA, *W1bA = p.w1bA;
  V4 *Wl = (V4 *)smem_t;
  auto stage = [&](const V4 *src) {
    __syncthreads();                                   // every wave is done with the matrix staged before
    for (int i = tid; i < NT * NJ * 64; i += blockDim.x) Wl[i] = src[i];
    __syncthreads();
  };
  if (!TR::F64) {
    V4 *a_ = (V4 *)smem_t, *b_ = a_ + NT * NJ * 64;
    for (int i = tid; i < NT * NJ * 64; i += blockDim.x) { a_[i] = p.attA[i]; b_[i] = p.w1bA[i]; }
    __syncthreads();
    AttA = a_; W1bA = b_;
  }
  const int r = lane & 15, g = lane >> 4;
  const int L = p.L;
  const T scale = p.sm_scale;
  constexpr bool STAGE_IDX = TR::F64 ? (FWD && ML <= 16) : true;      // (the fp64 training instances are at their register limit: 32 more spilled with it)
  // per-wave staging of a tile's history codes, behind the weight matrices (and the fp64 path's (p, dp) pairs)
  int32_t *IDX = (int32_t *)(smem_t + (TR::F64 ? (size_t)E * E * 8 + (size_t)4 * ML * 16 * 2 * 8 : (size_t)2 * E * E * 4)) + (size_t)wave * ML * 16;
  T *g_emb = p.grad;
  T *g_l1b = p.grad + p.num_index * E + (int64_t)E * E + (int64_t)E * 2 * E;
  T *g_l2w = g_l1b + E, *g_l2b = g_l2w + E;
  const int64_t n_tiles = (p.B + 15) >> 4;
  const V4 vzero = {0, 0, 0, 0};
  for (int64_t tile0 = (int64_t)blockIdx.x * nwaves; tile0 < n_tiles; tile0 += (int64_t)gridDim.x * nwaves) {
    // (the loop is uniform over the workgroup — the fp64 path has workgroup barriers inside; a wave past the last tile runs a dead one)
    const int64_t tile = tile0 + wave;
    int64_t row = tile * 16 + r;
    const bool live = tile < n_tiles && row < p.B;
    if (!live) row = p.B - 1;
    const int32_t code = p.codes[row];
    V4 qa[NJ];
    if (code >= 0) {
      const T *src = p.emb + (int64_t)code * E;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) qa[jc] = TR::load4(src, jc, g);
    } else {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) qa[jc] = vzero;
    }
    const unsigned mask = p.rowmask ? p.rowmask[row] : 0u;
    // The row's history codes are fetched ONCE per tile and parked in LDS ([16 j + r] per wave; round 6).  The three passes over the history
    // (forward, p / dp, ds / dk) used to read every code from global memory right before the gather it addresses: the gather's address
    // hung on a 4-byte load issued behind the previous key's row loads, and vmcnt retires in order — 3 L serial round trips per tile that
    // also drained the row in flight.  (The fp64 TRAINING instances keep the global reads: registers; their 32-position form also has no LDS left.)
    if constexpr (STAGE_IDX) {
#pragma unroll
      for (int k = 0; k < ML / 4; k++) { const int j = g + 4 * k; IDX[j * 16 + r] = (j < L) ? p.seqs[row * L + j] : -1; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    auto hist_code = [&](int j) -> int32_t {
      if constexpr (STAGE_IDX) return IDX[j * 16 + r];
      else return p.seqs[row * L + j];
    };
    auto load_key = [&](V4 (&kv)[NJ], int j) {
      const int32_t c = (j < L) ? hist_code(j) : -1;
      if (c >= 0) {
        const T *ks = p.emb + (int64_t)c * E;
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) kv[jc] = TR::load4(ks, jc, g);
      } else {
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) kv[jc] = vzero;
      }
    };
    auto dot_row = [&](const V4 (&a)[NJ], const V4 (&b)[NJ]) {
      T part = 0;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        part = fma(a[jc][0], b[jc][0], part); part = fma(a[jc][1], b[jc][1], part);
        part = fma(a[jc][2], b[jc][2], part); part = fma(a[jc][3], b[jc][3], part);
      }
      return TR::xsum(part);
    };
    V4 kr[2][NJ];
    // ================= forward (as rows_kernel: online softmax over the history) =================
    T m = -INFINITY, lsum = 0;
    V4 cv[NJ];
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) cv[jc] = vzero;
    load_key(kr[0], 0);
#pragma unroll
    for (int j = 0; j < ML; j++) {
      if (j < L) {
        load_key(kr[(j + 1) & 1], j + 1);
        asm volatile("" ::: "memory");
        T sv = dot_row(qa, kr[j & 1]) * scale;
        if ((mask >> j) & 1u) sv = (T)(-FLT_MAX);
        const T mn = m > sv ? m : sv;
        const T alpha = TR::exp_(m - mn), pj = TR::exp_(sv - mn);
        lsum = fma(lsum, alpha, pj);
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) {
          const V4 kv = kr[j & 1][jc];
          cv[jc][0] = fma(pj, kv[0], cv[jc][0] * alpha); cv[jc][1] = fma(pj, kv[1], cv[jc][1] * alpha);
          cv[jc][2] = fma(pj, kv[2], cv[jc][2] * alpha); cv[jc][3] = fma(pj, kv[3], cv[jc][3] * alpha);
        }
        m = mn;
      }
    }
    const T inv_l = (T)1 / lsum;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) {
      cv[jc][0] *= inv_l; cv[jc][1] *= inv_l; cv[jc][2] *= inv_l; cv[jc][3] *= inv_l;
      if (!FWD && DM_TR_LIVE(live)) TR::store4(p.CB + row * E, jc, g, cv[jc]);
    }
    // (weight-fragment addresses are rebuilt from an opaque per-tile offset: left loop-invariant, hipcc hoists all 384 of them out of the
    //  tile loop and spills them — 500 scratch stores in the prologue, 1 100 reloads per tile, a vmcnt(0) wait behind each)
    int zo = 0;
    asm volatile("" : "+v"(zo));
    const V4 *fAtt = AttA + lane + zo, *fW1a = p.w1aA + lane + zo, *fW1b = W1bA + lane + zo;
    const V4 *fW1bT = p.w1bTA + lane + zo, *fW1aT = p.w1aTA + lane + zo, *fAttT = p.attTA + lane + zo;
    const T *fb1 = p.b1 + zo, *fw2 = p.w2 + zo;      // (the same for the per-lane bias / w2 values and the dense-gradient addresses)
    T *gl1b = g_l1b + zo, *gl2w = g_l2w + zo;
    V4 att[NT];
    V4 zv[NT];
    T part = 0;
    // out[mt] (+)= sum_jc W[mt][jc] x[jc] with the staged matrix (fp64 path)
    auto prod_lds = [&](const V4 (&xin)[NJ], V4 (&out)[NT], const bool accumulate) {
      const V4 *wl = Wl + lane;
#pragma unroll
      for (int mt = 0; mt < NT; mt++) {
        V4 acc = accumulate ? out[mt] : vzero;
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) {
          const V4 wa = wl[(mt * NJ + jc) * 64];
#pragma unroll
          for (int t = 0; t < 4; t++) acc = TR::mfma(wa[t], xin[jc][t], acc);
        }
        out[mt] = acc;
      }
    };
    if constexpr (TR::F64) {
      stage(p.attA);
      prod_lds(cv, att, false);
#pragma unroll
      for (int mt = 0; mt < NT; mt++) if (!FWD && DM_TR_LIVE(live)) TR::store4(p.AT + row * E, mt, g, att[mt]);
      stage(p.w1aA);
      prod_lds(qa, zv, false);
      stage(p.w1bA);
      prod_lds(att, zv, true);
#pragma unroll
      for (int mt = 0; mt < NT; mt++) {
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int f = TR::feat(mt, g, rr);
          zv[mt][rr] += fb1[f];
          part = fma(zv[mt][rr] > 0 ? zv[mt][rr] : (T)0, fw2[f], part);
        }
      }
    } else {
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      V4 acc = vzero;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const V4 wa = fAtt[(mt * NJ + jc) * 64];
#pragma unroll
        for (int t = 0; t < 4; t++) acc = TR::mfma(wa[t], cv[jc][t], acc);
      }
      att[mt] = acc;
      if (!FWD && DM_TR_LIVE(live)) TR::store4(p.AT + row * E, mt, g, acc);
    }
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      V4 acc = vzero;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const V4 wa = fW1a[(mt * NJ + jc) * 64];
        const V4 wb = fW1b[(mt * NJ + jc) * 64];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          acc = TR::mfma(wa[t], qa[jc][t], acc);
          acc = TR::mfma(wb[t], att[jc][t], acc);
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int f = TR::feat(mt, g, rr);
        acc[rr] += fb1[f];
        part = fma(acc[rr] > 0 ? acc[rr] : (T)0, fw2[f], part);
      }
      zv[mt] = acc;
    }
    }
    const T x = TR::xsum(part) + p.b2;
    if constexpr (FWD) {                     // (uniform over the workgroup: the staged-matrix barriers of the next tile still meet)
      if (live && g == 0) p.logits[row] = x;
      continue;
    }
    const T y = (T)p.labels[row];
    // ================= loss + d(loss)/d(logit)  (BCECriterionWithLogits.scala:43-58, 75-84) =================
    const T gl = live ? ((T)1 / ((T)1 + TR::exp_(-x)) - y) * p.inv_B : (T)0;
    if (live && g == 0) {
      p.logits[row] = x;
      atomicAdd(p.loss_acc, (x > 0 ? x : (T)0) + TR::log_((T)1 + TR::exp_(-(x < 0 ? -x : x))));
      atomicAdd(p.loss_acc + 1, x * y);
    }
    {
      T v = (g == 0) ? gl : (T)0;          // one lane per row
      v = TR::sum16(v);
      if (lane == 0) atomicAdd(g_l2b, v);
    }
    // ================= backward through Linear2 / ReLU / Linear1 =================
    V4 dz[NT];
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int f = TR::feat(mt, g, rr);
        const T zz = zv[mt][rr];
        const T hv = zz > 0 ? zz : (T)0;
        const T d = zz > 0 ? gl * fw2[f] : (T)0;
        dz[mt][rr] = d;
        // gradWeight(l2) += gl * h ; gradBias(l1) += dz : reduce over the 16 rows of the tile, one atomic per feature
        const T sw = TR::sum16(gl * hv), sb = TR::sum16(d);
        if (r == 0) { atomicAdd(gl2w + f, sw); atomicAdd(gl1b + f, sb); }
      }
      if (DM_TR_LIVE(live)) TR::store4(p.DZ + row * E, mt, g, dz[mt]);
    }
    // dAtt = W1b^T dz ; dq = W1a^T dz   (Linear gradInput = gradOutput x W, Linear.scala:58-84)
    V4 da[NT], dq[NT];
    V4 dc[NT];
    if constexpr (TR::F64) {
      stage(p.w1bTA);
      prod_lds(dz, da, false);
#pragma unroll
      for (int mt = 0; mt < NT; mt++) if (DM_TR_LIVE(live)) TR::store4(p.DA + row * E, mt, g, da[mt]);
      stage(p.w1aTA);
      prod_lds(dz, dq, false);
      stage(p.attTA);
      prod_lds(da, dc, false);
    } else {
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      V4 acc0 = vzero, acc1 = vzero;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const V4 wa = fW1bT[(mt * NJ + jc) * 64];
        const V4 wb = fW1aT[(mt * NJ + jc) * 64];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          acc0 = TR::mfma(wa[t], dz[jc][t], acc0);
          acc1 = TR::mfma(wb[t], dz[jc][t], acc1);
        }
      }
      da[mt] = acc0; dq[mt] = acc1;
      if (DM_TR_LIVE(live)) TR::store4(p.DA + row * E, mt, g, acc0);
    }
    // dc = att.W^T dAtt
#pragma unroll
    for (int mt = 0; mt < NT; mt++) {
      V4 acc = vzero;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const V4 wa = fAttT[(mt * NJ + jc) * 64];
#pragma unroll
        for (int t = 0; t < 4; t++) acc = TR::mfma(wa[t], da[jc][t], acc);
      }
      dc[mt] = acc;
    }
    }
#if !(defined(DM_PROBE_BUILD) && defined(DM_DBG_TRAIN_NOBWD))
    // ================= attention backward (MatMul, SoftMax, Mask, MatMul(transB)) =================
    // pass C: p_j (recomputed from the running max / sum) and dp_j = dc . k_j
    // (p_j, dp_j) of the 16 rows x L positions: registers in fp32; in fp64 — where they were the kernel's last spilled values — the 32 KB
    // of LDS beside the staged matrix (the four lanes of a row write the same two doubles and each reads back what it wrote: no hand-over)
    T pr[TR::F64 ? 1 : ML], dp[TR::F64 ? 1 : ML];
    T *PD = (T *)(smem_t + (size_t)E * E * sizeof(T)) + ((size_t)wave * ML * 16 + r) * 2;
    T dot = 0;
    load_key(kr[0], 0);
#pragma unroll
    for (int j = 0; j < ML; j++) {
      if constexpr (!TR::F64) { pr[j] = 0; dp[j] = 0; }
      if (j < L) {
        load_key(kr[(j + 1) & 1], j + 1);
        asm volatile("" ::: "memory");
        T sv = dot_row(qa, kr[j & 1]) * scale;
        if ((mask >> j) & 1u) sv = (T)(-FLT_MAX);
        const T prj = TR::exp_(sv - m) * inv_l;
        const T dpj = dot_row(dc, kr[j & 1]);
        if constexpr (TR::F64) { PD[j * 32] = prj; PD[j * 32 + 1] = dpj; } else { pr[j] = prj; dp[j] = dpj; }
        dot = fma(dpj, prj, dot);
      }
    }
    // pass D: ds_j = scale * p_j (dp_j - dot), 0 where masked; dq += ds_j k_j ; dk_j = p_j dc + ds_j q
    load_key(kr[0], 0);
#pragma unroll
    for (int j = 0; j < ML; j++) {
      if (j < L) {
        load_key(kr[(j + 1) & 1], j + 1);
        asm volatile("" ::: "memory");
        T prj, dpj;
        if constexpr (TR::F64) { prj = PD[j * 32]; dpj = PD[j * 32 + 1]; } else { prj = pr[j]; dpj = dp[j]; }
        T ds = (dpj - dot) * prj * scale;
        if ((mask >> j) & 1u) ds = 0;
        const int32_t c = hist_code(j);
        // MiniBatch.transformWithMask replicates one user's history over all of its sampled nodes, so the 16 rows
        // of a tile usually share key j: reduce their contributions over the tile first (one atomic per element
        // instead of 16 on the same address).
        const int32_t c0 = __shfl(c, lane & 48);
        const unsigned long long same = __ballot(c == c0);
        const bool uniform = ((same >> (lane & 48)) & 0xFFFFull) == 0xFFFFull;
        const T pw = live ? prj : (T)0, dw = live ? ds : (T)0;
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) {
          const V4 kv = kr[j & 1][jc];
#pragma unroll
          for (int t = 0; t < 4; t++) {
            dq[jc][t] = fma(ds, kv[t], dq[jc][t]);
            T gk = fma(pw, dc[jc][t], dw * qa[jc][t]);
            if (uniform) {
              gk = TR::sum16(gk);
              if (r == 0 && c0 >= 0) DM_TR_ATOM(g_emb + (int64_t)c0 * E + TR::feat(jc, g, t), gk);
            } else if (live && c >= 0) {
              DM_TR_ATOM(g_emb + (int64_t)c * E + TR::feat(jc, g, t), gk);
            }
          }
        }
      }
    }
    if (live && code >= 0) {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
#pragma unroll
        for (int t = 0; t < 4; t++) DM_TR_ATOM(g_emb + (int64_t)code * E + TR::feat(jc, g, t), dq[jc][t]);
      }
    }
#else
    { T sink = dc[0][0] + dq[0][0]; asm volatile("" :: "v"(sink)); }
#endif
  }
}

// Weight gradients: dW1a = DZ^T Q, dW1b = DZ^T ATT, dAtt.W = DA^T COMB (Linear.accGradParameters,
// S/nn/Linear.scala:86-114: gradWeight.addmm(gradOutput^T, input)).  One wave per (matrix, block of output
// tiles, row chunk); the contraction runs over batch rows on the 16x16x4 MFMA of the model's type; results are added
// atomically into the compact gradient.
template <typename T>
struct WGradParamsT {
  const T *emb;
  const int32_t *codes;
  const T *DZ, *AT, *DA, *CB;
  int64_t B, num_index;
  int64_t chunk;   // rows per block (multiple of 8)
  T *grad;
  int mat_base = 0;   // first matrix of the launch (train_grouped_f64: matrices 1 and 2 over the per-user rows)
};
typedef WGradParamsT<float> WGradParams;

// Round 4: a wave owns a block of RT x RT output tiles (64 x 64 outputs at E >= 64) and a long row range.  With one 16 x 16 tile and 256
// rows per wave every MFMA needed two operand loads of its own (161 GB of L2 reads per 3.3 M-row level, at the gather ceiling) and every
// output address took 12 800 atomic adds; now an operand load feeds RT MFMAs, the next k-step's operands are in flight under the
// current one's MFMAs, and a wave adds its block once.
template <typename T, int E>
__global__ __launch_bounds__(64) void dm_wgrad_kernel(WGradParamsT<T> p) {
  typedef DmTr<T> TR;
  typedef typename TR::V4 V4;
  constexpr int NT = E / 16, RT = NT < 4 ? NT : 4, NB = NT / RT;
  const int lane = threadIdx.x;
  const int blk = blockIdx.x % (NB * NB), mat = blockIdx.x / (NB * NB) + p.mat_base;   // 0: l1a, 1: l1b, 2: att
  const int ot0 = (blk / NB) * RT, kt0 = (blk % NB) * RT;
  const int64_t r0 = (int64_t)blockIdx.y * p.chunk;
  int64_t r1 = r0 + p.chunk;
  if (r1 > p.B) r1 = p.B;
  const int i = lane & 15, kq = lane >> 4;
  const T *G = (mat == 2) ? p.DA : p.DZ;
  const T *X = (mat == 0) ? nullptr : (mat == 1 ? p.AT : p.CB);
  const V4 vzero = {0, 0, 0, 0};
  V4 acc[RT][RT];
#pragma unroll
  for (int x = 0; x < RT; x++)
#pragma unroll
    for (int y = 0; y < RT; y++) acc[x][y] = vzero;
  auto load = [&](int64_t rr, T (&a)[RT], T (&b)[RT]) {
    const int64_t row = rr + kq;
    if (row < r1) {
#pragma unroll
      for (int x = 0; x < RT; x++) a[x] = G[row * E + 16 * (ot0 + x) + i];
      if (mat == 0) {
        const int32_t c = p.codes[row];
#pragma unroll
        for (int y = 0; y < RT; y++) b[y] = c >= 0 ? p.emb[(int64_t)c * E + 16 * (kt0 + y) + i] : (T)0;
      } else {
#pragma unroll
        for (int y = 0; y < RT; y++) b[y] = X[row * E + 16 * (kt0 + y) + i];
      }
    } else {
#pragma unroll
      for (int x = 0; x < RT; x++) { a[x] = 0; b[x] = 0; }
    }
  };
  auto mma = [&](const T (&a)[RT], const T (&b)[RT]) {
#pragma unroll
    for (int x = 0; x < RT; x++)
#pragma unroll
      for (int y = 0; y < RT; y++) acc[x][y] = TR::mfma(a[x], b[y], acc[x][y]);
  };
  T a0[RT], b0[RT], a1[RT], b1[RT];
  load(r0, a0, b0);
  for (int64_t rr = r0; rr < r1; rr += 8) {        // two k-steps of four rows per iteration, operands ping-pong
    load(rr + 4, a1, b1);
    mma(a0, b0);
    load(rr + 8, a0, b0);
    mma(a1, b1);
  }
  // D[o][k = i]: o = 4 kq + rr (float) / kq + 4 rr (double) — the feature map of the D layout
  T *g_att = p.grad + p.num_index * E, *g_l1 = g_att + (int64_t)E * E;
#pragma unroll
  for (int x = 0; x < RT; x++)
#pragma unroll
    for (int y = 0; y < RT; y++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int o = TR::feat(ot0 + x, kq, rr), k = 16 * (kt0 + y) + i;
        T *dst = (mat == 2) ? g_att + (int64_t)o * E + k : g_l1 + (int64_t)o * 2 * E + (mat == 1 ? E : 0) + k;
        atomicAdd(dst, acc[x][y][rr]);
      }
}

// Adam.optimize (scalann/.../optim/Adam.scala:19-73), dense over the whole compact vector; every product and
// sum is rounded separately like the reference's tensor ops (no FMA contraction), epsilon after the sqrt.
// The gradient is scaled by `gscale` first (LocalOptimizer.syncGradients divides the summed worker gradients
// by the number of workers, T/optim/LocalOptimizer.scala:186) and zeroed for the next step.
__device__ __forceinline__ void dm_adam_elem(float *w, float *g, float *s, float *r, int64_t i, float gscale, float b1, float c1,
                                             float b2, float c2, float eps, float neg_step) {
#pragma clang fp contract(off)   // HIP's __fmul_rn/__fadd_rn are plain operators: keep hipcc from fusing them into FMAs
  // plain operators under contract(off): each product and sum is rounded on its own (the __f*_rn helpers are
  // inline functions compiled with contraction allowed, so they would still fuse after inlining)
  const float gi = gscale == 1.0f ? g[i] : g[i] * gscale;
  float si = s[i] * b1;
  const float t1 = c1 * gi;
  si = si + t1;
  const float bu = gi * gi;
  float ri = r[i] * b2;
  const float t2 = c2 * bu;
  ri = ri + t2;
  // sqrt and divide through fp64: (float)op((double)x) is the correctly rounded fp32 result (53 >= 2*24+2)
  float de = (float)sqrt((double)ri);
  de = de + eps;
  de = (float)((double)si / (double)de);
  const float t3 = neg_step * de;
  w[i] = w[i] + t3;
  s[i] = si; r[i] = ri; g[i] = 0.0f;
}
// The same step for a DIN[Double]: Adam.optimize is generic in the tensor's element type, so every operation below is the IEEE
// double operation the JVM performs (plain operators, no FMA contraction; sqrt and divide are correctly rounded in fp64).
__device__ __forceinline__ void dm_adam_elem(double *w, double *g, double *s, double *r, int64_t i, double gscale, double b1, double c1,
                                             double b2, double c2, double eps, double neg_step) {
#pragma clang fp contract(off)
  const double gi = gscale == 1.0 ? g[i] : g[i] * gscale;
  double si = s[i] * b1;
  const double t1 = c1 * gi;
  si = si + t1;
  const double bu = gi * gi;
  double ri = r[i] * b2;
  const double t2 = c2 * bu;
  ri = ri + t2;
  double de = sqrt(ri);
  de = de + eps;
  de = si / de;
  const double t3 = neg_step * de;
  w[i] = w[i] + t3;
  s[i] = si; r[i] = ri; g[i] = 0.0;
}
// The update over a whole vector.  KEEP puts the gradient back after the element update (an accumulating owner: dr_rerank_train.hip.inc).
template <typename T, bool KEEP>
__global__ void dm_adam_kernel(T *w, T *g, T *s, T *r, int64_t n, T gscale, T b1, T c1, T b2, T c2, T eps, T neg_step) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const T gi = g[i];
    dm_adam_elem(w, g, s, r, i, gscale, b1, c1, b2, c2, eps, neg_step);
    if (KEEP) g[i] = gi;
  }
}
// The same update over the ACTIVE embedding rows only (rows[0..n_rows): every row a gradient has ever reached since its TrainVec::init).
// For any other row g = s = r = 0, so the dense step computes s = 0 b1 + c1 0 = 0, r = 0, de = 0 / (sqrt(0) + eps) = 0 (eps > 0),
// t3 = neg_step 0 = -0 and w + (-0) = w bit for bit: leaving those rows alone IS the reference's dense Adam (Adam.scala:19-73),
// without streaming the 8 x 4 bytes per parameter of a table that cannot change.
template <typename T, bool KEEP>
__global__ void dm_adam_rows_kernel(T *w, T *g, T *s, T *r, const int32_t *rows, int64_t n_rows, int E, T gscale, T b1, T c1, T b2, T c2, T eps,
                                    T neg_step) {
  const int64_t n = n_rows * E;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)rows[t / E] * E + (t % E);
    const T gi = g[i];
    dm_adam_elem(w, g, s, r, i, gscale, b1, c1, b2, c2, eps, neg_step);
    if (KEEP) g[i] = gi;
  }
}

// Rebuild every fragment-ordered copy of the three small matrices from the (updated) compact vector.  The fp32 beam kernels'
// B-fragment copies (wfrag / afrag / bfrag) exist for float only.  Each group is skipped when its first pointer is null: wfrag, attA
// (an f64 model without d_tr64), attTA (no training state), att_wT (the f32 mirror of an f64 model has no transposes of its own).
template <typename T, int E>
__global__ void dm_refresh_fragments_kernel(const T *att_w, const T *l1_w, T *wfrag, T *afrag, T *bfrag,
                                            T *attA, T *w1aA, T *w1bA, T *attTA, T *w1aTA, T *w1bTA,
                                            T *att_wT, T *l1T) {
  typedef DmTr<T> TR;
  constexpr int NJ = E / 16, NT = E / 16;
  const int n = NJ * NT * 64 * 4;
  // plain transposes read by the general forward (din_forward_t): att_wT [k][o], l1T [2E k][o]
  if (att_wT)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 3 * E * E; i += gridDim.x * blockDim.x) {
    if (i < E * E) { const int k = i / E, o = i % E; att_wT[i] = att_w[o * E + k]; }
    else { const int j = i - E * E, k = j / E, o = j % E; l1T[j] = l1_w[o * 2 * E + k]; }
  }
  for (int fi = blockIdx.x * blockDim.x + threadIdx.x; fi < n; fi += gridDim.x * blockDim.x) {
    const int t = fi & 3, ln = (fi >> 2) & 63, blk = fi >> 8;
    const int hi = blk / NT, lo = blk % NT;       // NJ == NT
    const int col = ln & 15;
    if (wfrag) {   // B-fragment order [jc = hi][nt = lo] of the fp32 beam kernels (k = 16 jc + 4 (ln >> 4) + t)
      const int k = 16 * hi + 4 * (ln >> 4) + t, o = 16 * lo + col;
      wfrag[fi] = l1_w[o * 2 * E + k]; afrag[fi] = att_w[o * E + k]; bfrag[fi] = l1_w[o * 2 * E + E + k];
    }
    if (attA) {   // A-fragment order [mt = hi][jc = lo], k in the element type's feature map
      const int o = 16 * hi + col, k = TR::feat(lo, ln >> 4, t);
      attA[fi] = att_w[o * E + k]; w1aA[fi] = l1_w[o * 2 * E + k]; w1bA[fi] = l1_w[o * 2 * E + E + k];
      if (attTA) { attTA[fi] = att_w[k * E + o]; w1aTA[fi] = l1_w[k * 2 * E + o]; w1bTA[fi] = l1_w[k * 2 * E + E + o]; }
    }
  }
}
