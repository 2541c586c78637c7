// Persistent beam-search kernel, one wave per SIMD with W1a resident in the AccVGPRs ("W kernel"): the split-fp16 scorer of
// beam_kernel.hip.inc (same arithmetic, same results bit for bit) re-laid for the measured limiter of that kernel — the 64 KB
// of W1a fragment reads every 16-row tile makes from LDS (DESIGN.md §3: the LDS-fed stream tops out at 0.48 of the fp16 pipe).
//
//   * 256-thread workgroups, ONE wave per SIMD with the full 512-register budget: the 256 AccVGPRs hold the E*E fp16 hi and lo
//     planes of W1a (64 A fragments of v_mfma_f32_16x16x32_f16 at E = 128) for the whole life of the wave, loaded once from L2;
//     every MFMA of the W1a chain takes its A operand straight from an AGPR (vdst / srcB / srcC in ArchVGPRs), so the chain
//     makes NO LDS reads at all (tools/agpr_mfma_microbench.hip: 0.85-0.87 of the fp16 dense peak from one wave per SIMD).
//   * a wave is a TEAM of its own: it pops a user, walks it through every level with the frontier in its LDS slot and never
//     meets another wave (no team barriers, no polling); the 512-slot prune is a register bitonic sort with 8 keys per lane.
//   * with a single wave per SIMD nothing hides a wave's non-MFMA work, so the tile is software-pipelined BY HAND: the VALU
//     work of three tiles — epilogue of tile t-1, softmax of tile t, operand split of tile t+1 — is cut into small pieces that
//     sit between the 4-MFMA batches of tile t's W1a chain (the matrix pipe takes one MFMA per ~16 cycles and the SIMD issues
//     2-3 other instructions in its shadow), gathers run one tile ahead in registers and an L2 touch runs three tiles ahead.
//   * every MFMA here is inline assembly (an AGPR A operand with ArchVGPR accumulators has no builtin; and with the AGPR file
//     full the compiler must not pick AGPR-form accumulators for any other MFMA).  Wait states the assembler text hides from
//     the compiler are explicit: an MFMA result is read by VALU code at least four MFMAs later (or after an s_nop that names
//     it), a VALU-written operand is consumed at least two issue slots later, accumulate chains need none.
//
// Reference: the same level fold as beam_kernel.hip.inc — Recommender._recommend (tdm/src/main/scala/com/mass/tdm/model/
// Recommender.scala:40-107), CandidateSearcher.beamSearch (otm/src/main/scala/com/mass/otm/model/CandidateSearcher.scala:58-80),
// the DIN forward (tdm/.../model/DIN.scala:18-42) in the per-user restructured form.

#define DMW_BLOCK 256
#define DMW_NWAVES 4

__device__ __forceinline__ void dmw_mfma_av(f32x4 &acc, const dm_h8 &a, const dm_h8 &b) {
  asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(a), "v"(b));
}
// srcC = 0: starts a chain.  The accumulator is declared read-write although its old value is not used: the loop-carried
// variable then keeps ONE register set (a fresh output would make the compiler copy 32 registers at every loop back-edge)
__device__ __forceinline__ void dmw_mfma_av0(f32x4 &acc, const dm_h8 &a, const dm_h8 &b) {
  asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "+v"(acc) : "a"(a), "v"(b));
}
__device__ __forceinline__ void dmw_mfma_vv(f32x4 &acc, const dm_h8 &a, const dm_h8 &b) {
  asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void dmw_mfma_vv0(f32x4 &acc, const dm_h8 &a, const dm_h8 &b) {
  asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void dmw_mfma_f32(f32x4 &acc, float a, float b) {
  asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
#define DMW_PIN() __builtin_amdgcn_sched_barrier(0)
// LDS traffic of ONE wave executes in order; this only stops the compiler from moving accesses across it
__device__ __forceinline__ void dmw_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// A tile's operand gathers are issued from assembly, so that the COMPILER does not count them: vector-memory loads return in
// order, and its s_waitcnt placement at the loop header (the merge of the pre-header's and the back edge's pending loads) made
// the score MFMAs of a tile wait for the gathers issued a few hundred cycles earlier for the tile AFTER it.  The kernel places
// the waits itself (dmw_vmwait): the gathers of one operand set are followed by exactly those of the other set.
template <int OFF>
__device__ __forceinline__ void dmw_gather16(dm_h8 &dst, const dm_h8 *src) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(src), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void dmw_vmwait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N)); }

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>).  The tile below is several hundred call
// sites that must ALL be resolved at compile time (register arrays indexed by constants, `if constexpr` work placement); a
// `#pragma unroll` loop of that size runs into the unroller's size threshold and silently stays a loop (arrays -> scratch).
template <typename F, int... I>
__device__ __forceinline__ void dm_static_for_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void dm_static_for(F &&f) { dm_static_for_impl(f, std::make_integer_sequence<int, N>{}); }
#define DMW_FOR(N, v) dm_static_for<N>([&](auto v##_c) { constexpr int v = decltype(v##_c)::value;
#define DMW_END });

// the operand split of dm_split8 in four 4-instruction pieces (so that they can sit between MFMAs): x = hi + lo,
// hi = f16(x * s), lo = f16(x * s - hi); a piece never reads a register the previous instruction wrote half of
__device__ __forceinline__ void dmw_split_a(const f32x4 &u, const f32x4 &v, float s, unsigned (&h)[4]) {
  asm volatile("v_fma_mixlo_f16 %0, %4, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "v_fma_mixlo_f16 %1, %5, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "v_fma_mixlo_f16 %2, %6, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "v_fma_mixlo_f16 %3, %7, %8, 0 op_sel_hi:[0,0,0]"
               : "=&v"(h[0]), "=&v"(h[1]), "=&v"(h[2]), "=&v"(h[3]) : "v"(u[0]), "v"(u[2]), "v"(v[0]), "v"(v[2]), "v"(s));
}
__device__ __forceinline__ void dmw_split_b(const f32x4 &u, const f32x4 &v, float s, unsigned (&h)[4]) {
  asm volatile("v_fma_mixhi_f16 %0, %4, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "v_fma_mixhi_f16 %1, %5, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "v_fma_mixhi_f16 %2, %6, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "v_fma_mixhi_f16 %3, %7, %8, 0 op_sel_hi:[0,0,0]\n\t"
               "s_nop 0"
               : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]) : "v"(u[1]), "v"(u[3]), "v"(v[1]), "v"(v[3]), "v"(s));
}
__device__ __forceinline__ void dmw_split_c(const f32x4 &u, const f32x4 &v, float s, const unsigned (&h)[4], unsigned (&l)[4]) {
  asm volatile("v_fma_mixlo_f16 %0, %4, %8, -%9 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
               "v_fma_mixlo_f16 %1, %5, %8, -%10 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
               "v_fma_mixlo_f16 %2, %6, %8, -%11 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
               "v_fma_mixlo_f16 %3, %7, %8, -%12 op_sel:[0,0,0] op_sel_hi:[0,0,1]"
               : "=&v"(l[0]), "=&v"(l[1]), "=&v"(l[2]), "=&v"(l[3])
               : "v"(u[0]), "v"(u[2]), "v"(v[0]), "v"(v[2]), "v"(s), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]));
}
__device__ __forceinline__ void dmw_split_d(const f32x4 &u, const f32x4 &v, float s, const unsigned (&h)[4], unsigned (&l)[4]) {
  asm volatile("v_fma_mixhi_f16 %0, %4, %8, -%9 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
               "v_fma_mixhi_f16 %1, %5, %8, -%10 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
               "v_fma_mixhi_f16 %2, %6, %8, -%11 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
               "v_fma_mixhi_f16 %3, %7, %8, -%12 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
               "s_nop 0"
               : "+v"(l[0]), "+v"(l[1]), "+v"(l[2]), "+v"(l[3])
               : "v"(u[1]), "v"(u[3]), "v"(v[1]), "v"(v[3]), "v"(s), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]));
}
// the same four pieces, ONE instruction at a time (element i = 0..3 of the piece), so that each can sit behind its own MFMA.
// x = the fp32 source of the half being written: piece a/c take u[0], u[2], v[0], v[2]; piece b/d take u[1], u[3], v[1], v[3].
__device__ __forceinline__ float dmw_split_src(const f32x4 &u, const f32x4 &v, int piece, int i) {
  const int odd = piece & 1;
  return i == 0 ? u[odd] : i == 1 ? u[2 + odd] : i == 2 ? v[odd] : v[2 + odd];
}
__device__ __forceinline__ void dmw_split_1(const f32x4 &u, const f32x4 &v, float s, unsigned (&h)[4], unsigned (&l)[4], int piece, int i) {
  const float x = dmw_split_src(u, v, piece, i);
  if (piece == 0) asm volatile("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "=v"(h[i]) : "v"(x), "v"(s));
  else if (piece == 1) asm volatile("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(h[i]) : "v"(x), "v"(s));
  else if (piece == 2) asm volatile("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=&v"(l[i]) : "v"(x), "v"(s), "v"(h[i]));
  else asm volatile("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l[i]) : "v"(x), "v"(s), "v"(h[i]));
}
__device__ __forceinline__ dm_h8 dmw_pack(const unsigned (&x)[4]) {
  typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
  const u32x4_ v = {x[0], x[1], x[2], x[3]};
  return __builtin_bit_cast(dm_h8, v);
}

// Register bitonic sort of 512 keys, 8 consecutive per lane (element 8 * lane + e), in the direction-free form of the network:
// the merge of phase k opens with a FLIP (element i against i ^ (k - 1)) and continues with the half-cleaners i ^ j, j = k/4 .. 1;
// every compare-exchange then keeps the smaller key at the lower index — no per-lane direction bit, no xor with the compare
// mask.  Element strides below 8 are in-lane; across lanes a flip pairs lane l with l ^ (k/8 - 1) (a mirror inside a group of
// k/8 lanes: DPP quad_perm / row_half_mirror / row_mirror, ds_swizzle for 32, one bpermute for 64) and element e with 7 - e.
template <int MASK>
__device__ __forceinline__ uint32_t dmw_lane_xor(uint32_t v, int lane) {
  if constexpr (MASK == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
  else if constexpr (MASK == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
  else if constexpr (MASK == 3) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x1B, 0xF, 0xF, true);   // quad_perm [3,2,1,0]
  else if constexpr (MASK == 7) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  else if constexpr (MASK == 15) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true); // row_mirror
  else if constexpr (MASK == 4 || MASK == 8 || MASK == 16 || MASK == 31)
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (MASK << 10));                                    // bit mode: lane ^ MASK
  else return (uint32_t)__shfl((int)v, lane ^ MASK);                                                             // 32, 63: one bpermute
}
// Keys are built as (descending-order key of the score << 30) | position: the two top bits are clear, so the 64 bits read as a
// double are a non-negative finite number (exponent field <= 0x3ff) and the order of the doubles is the order of the integers.  A
// compare-exchange is then v_min_f64 + v_max_f64 — two instructions instead of v_cmp_lt_u64 + four v_cndmask (fp64 denormals are
// never flushed: the kernel keeps the default denormal mode, and min / max return one operand's bits unchanged).
#define DMW_KEY_SHIFT 30
#define DMW_KEY_POS(k) ((uint32_t)(k) & 0x3FFFFFFFu)
#define DMW_KEY_PAD 0x7FEFFFFFFFFFFFFFull          // the largest finite double: sorts behind every real key
__device__ __forceinline__ unsigned long long dmw_make_key(float score, unsigned pos) {
  return ((unsigned long long)dm_desc_key(score) << DMW_KEY_SHIFT) | pos;
}
__device__ __forceinline__ void dmw_cx(unsigned long long &a, unsigned long long &b) {      // a <- min, b <- max
  unsigned long long lo, hi;
  asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
  asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
  a = lo; b = hi;
}
// in-lane stage: partner element e ^ X (X = K - 1 for a flip, X = j for a half-cleaner)
template <int X>
__device__ __forceinline__ void dmw_sort_inlane(unsigned long long (&key)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e++) if ((e ^ X) > e) dmw_cx(key[e], key[e ^ X]);
}
// Cross-lane stages keep a lane's keys NEGATED (sign bit set) while the lane is the upper one of its pair: the lower lane
// holds k_a and receives -k_b, the upper holds -k_b and receives k_a, and BOTH execute  mine = min(mine, -received)  —
// min(k_a, k_b) below, -max(k_a, k_b) above: one v_min_f64 with a source modifier, no per-lane direction.  `neg` is the
// lane's current state (0 or 0x80000000); moving to the state the next stage needs is one v_xor per key.
__device__ __forceinline__ void dmw_sort_role(unsigned long long (&key)[8], unsigned &neg, unsigned want) {
  const unsigned m = neg ^ want;
#pragma unroll
  for (int e = 0; e < 8; e++) key[e] ^= (unsigned long long)m << 32;
  neg = want;
}
// cross-lane stage: partner lane l ^ LM; FLIP pairs element e with 7 - e
template <int LM, bool FLIP>
__device__ __forceinline__ void dmw_sort_xlane(unsigned long long (&key)[8], int lane, unsigned &neg) {
  constexpr int TOP = LM >= 32 ? 32 : LM >= 16 ? 16 : LM >= 8 ? 8 : LM >= 4 ? 4 : LM >= 2 ? 2 : 1;      // the bit that orders the pair
  dmw_sort_role(key, neg, (lane & TOP) ? 0x80000000u : 0u);
  unsigned long long o[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const uint32_t olo = dmw_lane_xor<LM>((uint32_t)key[e], lane), ohi = dmw_lane_xor<LM>((uint32_t)(key[e] >> 32), lane);
    o[FLIP ? 7 - e : e] = ((unsigned long long)ohi << 32) | olo;
  }
#pragma unroll
  for (int e = 0; e < 8; e++) asm("v_min_f64 %0, %0, -%1" : "+v"(key[e]) : "v"(o[e]));
}
template <int K>
__device__ __forceinline__ void dmw_sort_phase(unsigned long long (&key)[8], int lane, unsigned &neg) {
  if constexpr (K <= 8) dmw_sort_inlane<K - 1>(key);
  else dmw_sort_xlane<K / 8 - 1, true>(key, lane, neg);
  if constexpr (K >= 512) dmw_sort_xlane<16, false>(key, lane, neg);
  if constexpr (K >= 256) dmw_sort_xlane<8, false>(key, lane, neg);
  if constexpr (K >= 128) dmw_sort_xlane<4, false>(key, lane, neg);
  if constexpr (K >= 64) dmw_sort_xlane<2, false>(key, lane, neg);
  if constexpr (K >= 32) dmw_sort_xlane<1, false>(key, lane, neg);
  if constexpr (K >= 16) dmw_sort_role(key, neg, 0u);          // the in-lane stages work on plain keys
  if constexpr (K >= 16) dmw_sort_inlane<4>(key);
  if constexpr (K >= 8) dmw_sort_inlane<2>(key);
  if constexpr (K >= 4) dmw_sort_inlane<1>(key);
}

// ---- the per-row setup product  G_j = W1b (att.W k_j)  in two stages on the fp32 matrix pipe:  T1 = K att_w^T,  G = T1 W1b^T.
// Row j of G depends on history row k_j and the dense weights alone — not on the user, nor on which rows share the 16-row tile —
// so the same code serves the W kernel's per-user setup and the builder of the per-row table (BeamParams::g_table), whose rows
// are therefore the setup's values bit for bit.
//
// One stage: 16 x E times E x E, one 16-column tile at a time; the B fragments (L2-resident, shared by every user) are fetched
// TWO tiles ahead of the tile being multiplied — one wave has nothing else to hide their latency with.  Lane (r, g) holds row r
// of the left operand, columns 16 jc + 4 g .. + 3 in a[jc]; emit(nt, acc) receives rows 4 g .. 4 g + 3 of column 16 nt + r.
template <int E, typename Emit>
__device__ __forceinline__ void dmw_gemm16(const f32x4 *frag, const f32x4 (&a)[E / 16], int lane, Emit &&emit) {
  constexpr int NJ = E / 16, NT = E / 16;
  f32x4 bq[3][NJ];
  // uniform base + one 32-bit lane offset (opaque: else the NJ * NT lane addresses are loop-invariant over the users, get
  // hoisted and spilled, and every load then waits for the scratch reload of its own address)
  unsigned lo16 = 16u * (unsigned)lane;
  asm volatile("" : "+v"(lo16));
  const char *fb = (const char *)frag;
  auto fetch = [&](auto nt_c) {
    constexpr int nt = decltype(nt_c)::value;
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) bq[nt % 3][jc] = *(const f32x4 *)(fb + (size_t)((jc * NT + nt) * 1024) + lo16);
  };
  fetch(std::integral_constant<int, 0>{});
  if constexpr (NT > 1) fetch(std::integral_constant<int, 1>{});
  DMW_FOR(NT, nt)
    if constexpr (nt + 2 < NT) fetch(std::integral_constant<int, nt + 2>{});
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    asm volatile("s_nop 1" : "+v"(acc));
#pragma unroll
    for (int jc = 0; jc < NJ; jc++)
#pragma unroll
      for (int t = 0; t < 4; t++) dmw_mfma_f32(acc, a[jc][t], bq[nt % 3][jc][t]);
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(acc));
    emit(nt, acc);
  DMW_END
}
// the transpose between the stages, through T1s[16][E + 4] in LDS: the first stage's output (rows 4 g .. 4 g + 3 of a column per
// lane) becomes the second stage's left operand (row r, four consecutive columns per lane)
template <int E>
__device__ __forceinline__ void dmw_t1_put(float *T1s, int r, int g, int nt, const f32x4 &acc) {
#pragma unroll
  for (int rr = 0; rr < 4; rr++) T1s[(4 * g + rr) * (E + 4) + 16 * nt + r] = acc[rr];
}
template <int E>
__device__ __forceinline__ void dmw_t1_get(const float *T1s, int r, int g, f32x4 (&ta)[E / 16]) {
#pragma unroll
  for (int jc = 0; jc < E / 16; jc++) ta[jc] = *(const f32x4 *)(T1s + r * (E + 4) + 16 * jc + 4 * g);
}

// The table of setup rows: out[c][0 .. E) = W1b (att.W emb[c]) without b1, for every row c of the fp32 table.  One wave per 16
// table rows, grid-stride; each wave runs the setup's two stages on its rows as the W kernel does on a user's history rows.
template <int E>
__global__ __launch_bounds__(DMW_BLOCK) void dm_build_g_table_kernel(const float *emb, const f32x4 *afrag, const f32x4 *bfrag, int64_t n_rows, float *out) {
  constexpr int NJ = E / 16;
  __shared__ __attribute__((aligned(16))) float T1all[DMW_NWAVES][16 * (E + 4)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  float *T1s = T1all[wave];
  const int64_t n_tiles = (n_rows + 15) / 16;
  for (int64_t t = (int64_t)blockIdx.x * DMW_NWAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * DMW_NWAVES) {
    const int64_t row = 16 * t + r;
    f32x4 ka[NJ];
    if (row < n_rows) {
      const f32x4 *src = (const f32x4 *)(emb + row * E) + g;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) ka[jc] = src[4 * jc];
    } else {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) ka[jc] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    dmw_gemm16<E>(afrag, ka, lane, [&](int nt, const f32x4 &acc) { dmw_t1_put<E>(T1s, r, g, nt, acc); });
    dmw_wave_sync();
    f32x4 ta[NJ];
    dmw_t1_get<E>(T1s, r, g, ta);
    dmw_wave_sync();          // T1 is in registers: the next tile of rows may overwrite it
    dmw_gemm16<E>(bfrag, ta, lane, [&](int nt, const f32x4 &acc) {
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int64_t orow = 16 * t + 4 * g + rr;
        if (orow < n_rows) out[orow * E + 16 * nt + r] = acc[rr];
      }
    });
  }
}

struct BeamWLds { int b1, w2, lb, slot0, slot_stride, x_kfrag, x_gfrag, y_keys, y_acode0, y_acode1, y_aval, misc, total; };
__host__ __device__ inline BeamWLds dm_beamw_lds(int E, int cap, int pcap, int kq) {
  const int kcols = kq >= 4 ? 16 : 12;
  BeamWLds l;
  int o = 0;
  l.b1 = o; o += E * 4;
  l.w2 = o; o += E * 4;
  l.lb = o; o += DM_N_LEVEL_BOUNDS * 4;          // the tree's per-level existence bounds (BeamParams::level_last)
  l.slot0 = o;
  int s = 0;
  l.x_kfrag = s; s += (E / 16) * 4 * kcols * 16;          // K as fp16 hi / lo planes, A-fragment order of the 16x16x32 shape
  l.x_gfrag = s; s += kq * (E / 16) * 64 * 4 > (E / 16) * 64 * 16 ? kq * (E / 16) * 64 * 4 : (E / 16) * 64 * 16;   // (G + b1): fp32 planes, then [hi | lo] fp16
  const int ybase = s;
  l.y_keys = s; s += pcap * 8;
  l.y_acode0 = s; s += cap * 4;
  l.y_acode1 = s; s += cap * 4;
  l.y_aval = s; s += cap * 4;
  if (s - ybase < 16 * (E + 4) * 4) s = ybase + 16 * (E + 4) * 4;   // T1 scratch during setup
  s = (s + 15) & ~15;
  l.misc = s; s += 64 * 4;
  l.slot_stride = s;
  o += s * DMW_NWAVES;
  l.total = (o + 15) & ~15;
  return l;
}

// work item -> gap of the W1a chain (NSLOT gaps, one per batch).  Softmax of the tile early; the next tile's k-step s is split
// IN PLACE once this tile's k-step s has been multiplied (one batch of slack); smaller E squeeze everything evenly.
// softmax item k -> MFMA position of the chain (npos positions): one item per position from the fourth gap on, four positions
// of slack after each cross-lane exchange (items 4, 5, 10, 11 issue one); short chains squeeze the items evenly
constexpr int dmw_sm_pos(int npos, int k) {
  const int skips = (k > 4 ? 4 : 0) + (k > 5 ? 4 : 0) + (k > 10 ? 4 : 0) + (k > 11 ? 4 : 0);
  return npos >= 64 ? 12 + k + skips : (k * npos) / 18;
}
constexpr int dmw_sp_slot(int nslot, int gps, int s, int piece) { const int b = 3 * gps * (s + 1) + piece; return b < nslot ? b : nslot - 1; }
constexpr int dmw_ep_slot(int nb, int j) { const int last = 3 * (j / nb) - 1, first = 3 * (j / nb - 1); return first + ((j % nb) * (last - first + 1)) / nb; }

// ---- the FOLDED attention-combine (L <= 10): H^T += (G + b1)^T P^T in ONE v_mfma_f32_16x16x32_f16 per feature tile.
// The product has three terms per history position — p_hi G_hi, p_hi G_lo, p_lo G_hi — so 3 L <= 30 of the 32 contraction
// slots of one MFMA.  Lane group g of the tile holds p of positions g, g + 4, g + 8 (i = 0, 1, 2) and owns k-slots 8 g .. 8 g + 7;
// positions 8 and 9 (groups 0, 1) would need nine slots, so their p_lo G_hi term lives in slot 2 of group g + 2, whose own third
// position (10, 11) does not exist.  This function is THE slot map: the per-user setup writes the (G + b1) fragment through its
// inverse, the tile code packs the P operand by it (dmw_fold_p_item states what the packing puts into every slot).
enum { DMW_HH = 0, DMW_HL = 1, DMW_LH = 2 };          // p_hi G_hi, p_hi G_lo, p_lo G_hi
#define DMW_FOLD_MAXL 10
struct DmwSlot { int grp, k; };
constexpr DmwSlot dmw_fold_slot(int pos, int term) {
  const int g = pos & 3, i = pos >> 2;
  if (term == DMW_HH) return DmwSlot{g, i};
  if (term == DMW_HL) return DmwSlot{g, 4 + i};
  return i == 0 ? DmwSlot{g, 3} : i == 1 ? DmwSlot{g, 7} : DmwSlot{g + 2, 2};
}
// inverse: the (position, term) of slot (grp, k) as 4 * pos + term, -1 for a slot no term owns
constexpr int dmw_fold_src(int grp, int k) {
  for (int pos = 0; pos < DMW_FOLD_MAXL; pos++)
    for (int term = 0; term < 3; term++) {
      const DmwSlot s = dmw_fold_slot(pos, term);
      if (s.grp == grp && s.k == k) return 4 * pos + term;
    }
  return -1;
}
// the G part of k-slot k — hi, or lo for a p_hi G_lo term — is the same in every lane group that uses the slot (the G writer
// converts by slot, not by lane)
constexpr bool dmw_fold_g_lo(int k) { return k >= 4 && k < 7; }
// what the tile code packs into slot (grp, k) of the P operand: item j (0, 1) as 2 * pos + (1 = the lo part), -1 for none.
// Slots 0-2 / 4-6 carry p_hi of the lane's own positions, 3 / 7 p_lo of its first two, and slot 2 is OR-ed with p_lo of the
// third position of the lane 32 further (group grp ^ 2): of the two halves OR-ed there one is always +0
constexpr int dmw_fold_p_item(int grp, int k, int j) {
  if (j == 0) return k == 3 ? 2 * grp + 1 : k == 7 ? 2 * (grp + 4) + 1 : 2 * (grp + 4 * (k & 3));
  return k == 2 ? 2 * ((grp ^ 2) + 8) + 1 : -1;
}
// for every L <= 10: every (position < L, term) owns exactly one slot, no slot has two owners, and what the P operand holds in
// a slot is the owner's p part or — a position >= L has p = +0 in both parts — zero: every unused slot multiplies a zero
constexpr bool dmw_fold_map_ok() {
  for (int L = 1; L <= DMW_FOLD_MAXL; L++) {
    int owners[4][8] = {};
    for (int pos = 0; pos < L; pos++)
      for (int term = 0; term < 3; term++) {
        const DmwSlot s = dmw_fold_slot(pos, term);
        if (s.grp < 0 || s.grp > 3 || s.k < 0 || s.k > 7) return false;
        if (++owners[s.grp][s.k] > 1) return false;
        if (dmw_fold_src(s.grp, s.k) != 4 * pos + term || dmw_fold_g_lo(s.k) != (term == DMW_HL)) return false;
      }
    for (int grp = 0; grp < 4; grp++)
      for (int k = 0; k < 8; k++) {
        const int src = dmw_fold_src(grp, k);
        const int want = src >= 0 && (src >> 2) < L ? 2 * (src >> 2) + ((src & 3) == DMW_LH ? 1 : 0) : -1;
        for (int j = 0; j < 2; j++) {
          const int it = dmw_fold_p_item(grp, k, j);
          if (it >= 0 && (it >> 1) < L && it != want) return false;          // a live p part in a slot that is not its own
        }
        if (want >= 0 && dmw_fold_p_item(grp, k, 0) != want && dmw_fold_p_item(grp, k, 1) != want) return false;
      }
  }
  return true;
}
static_assert(dmw_fold_map_ok(), "folded attention-combine: the slot map and the P packing disagree");
// position whose (G + b1) value slot k of lane group grp holds, per k as one nibble per group (15 = none: the half is zero)
constexpr unsigned dmw_fold_pos_nibbles(int k) {
  unsigned w = 0;
  for (int grp = 0; grp < 4; grp++) { const int s = dmw_fold_src(grp, k); w |= (unsigned)(s < 0 ? 15 : s >> 2) << (4 * grp); }
  return w;
}

template <int E, int KQ, bool FOLD>
__global__ __launch_bounds__(DMW_BLOCK, 1) void dm_beam_w_kernel(BeamParams p) {
  static_assert(!FOLD || KQ <= 3, "the folded attention-combine holds 10 history positions");
  constexpr int NJ = E / 16, NT = E / 16, NS = E / 32;
  constexpr int KCOLS = KQ >= 4 ? 16 : 12;
  constexpr int NB = NT < 4 ? NT : 4;          // MFMAs per batch (independent accumulators issued back to back)
  constexpr int NGRP = NS * (NT / NB);         // batches-of-three in the W1a chain: 8 at E = 128
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const BeamWLds lo = dm_beamw_lds(E, p.cap, p.pcap, KQ);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CAP = p.cap, L = p.L;
  float *B1 = (float *)(smem + lo.b1), *W2 = (float *)(smem + lo.w2);
  int *LB = (int *)(smem + lo.lb);
  char *slotp = smem + lo.slot0 + wave * lo.slot_stride;
  unsigned long long *keys = (unsigned long long *)(slotp + lo.y_keys);
  float *A_val = (float *)(slotp + lo.y_aval);
  int *misc = (int *)(slotp + lo.misc);
  const dm_h8 *Kh = (const dm_h8 *)(slotp + lo.x_kfrag);
  const float *Gf = (const float *)(slotp + lo.x_gfrag);

  // ---- once per wave: W1a hi / lo planes into the AccVGPRs ([plane][s][nt] fragments, lane-major in global memory) ----
  dm_h8 wreg[2 * NS * NT];
#pragma unroll
  for (int i = 0; i < 2 * NS * NT; i++) {
    const dm_h8 t = p.wsplit[i * 64 + lane];
    asm volatile("" : "=a"(wreg[i]) : "0"(t));
  }
  for (int i = tid; i < E; i += DMW_BLOCK) { B1[i] = p.b1[i]; W2[i] = p.w2[i] * p.out_unscale; }
  // the existence bounds of the tree's levels, staged once (a by-value array indexed by a level would live in scratch); without
  // them — OTM, DM_LEVEL_BOUNDS=0 — every level reads "use the bits"
  if (tid < DM_N_LEVEL_BOUNDS) LB[tid] = (p.mode == 0 && p.level_last) ? p.level_last[tid] : DM_LEVEL_USE_BITS;
  __syncthreads();                 // b1 / w2: the only workgroup-wide barrier
  const float scale2 = (float)(1.4426950408889634 * (double)p.sm_scale) * p.score_unscale;
  unsigned long long my_rows = 0;
#ifdef DM_PHASE_TIMERS
  unsigned long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tlast = clock64();
#define WMARK(k) do { unsigned long long tn_ = clock64(); tph[k] += tn_ - tlast; tlast = tn_; } while (0)
#else
#define WMARK(k) do {} while (0)
#endif
#ifdef DM_SETUP_TIMERS      // finer split of the per-user setup, reported through the tile-timer slots
  unsigned long long tsu[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long ts_last = 0;
#define SMARK(k) do { unsigned long long tn_ = clock64(); if (k >= 0) tsu[k < 0 ? 0 : k] += tn_ - ts_last; ts_last = tn_; } while (0)
#else
#define SMARK(k) do {} while (0)
#endif
#ifdef DM_TILE_TIMERS
  unsigned long long ttile[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tt_last = 0;
#define TMARK(k) do { unsigned long long tn_ = clock64(); ttile[k] += tn_ - tt_last; tt_last = tn_; } while (0)
#else
#define TMARK(k) do {} while (0)
#endif

  // LDS traffic of ONE wave executes in order; this only stops the compiler from moving accesses across it
  auto wsync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // ordered scan over elements laid out lane-major, 4 per lane
  auto scan4 = [&](unsigned bits4, int &total) -> int {
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int before = 0, wtot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const unsigned long long m = __ballot((bits4 >> j) & 1u);
      before += __popcll(m & below);
      wtot += __popcll(m);
    }
    total = wtot;
    return before;
  };
  auto scan8 = [&](unsigned bits8, int &total) -> int {       // the same, 8 per lane
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int before = 0, wtot = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const unsigned long long m = __ballot((bits8 >> j) & 1u);
      before += __popcll(m & below);
      wtot += __popcll(m);
    }
    total = wtot;
    return before;
  };
  // register bitonic sort of 512 keys, 8 consecutive per lane; ascending; keys unique => the stable order
  auto reg_sort8 = [&](unsigned long long (&key)[8], int Pn) {
    // the lane id is made opaque: computed from the real one the lane masks are loop-invariant over the whole kernel, get hoisted
    // and — with every register taken by the tile loop — spilled
    int ln = lane;
    asm volatile("" : "+v"(ln));
    unsigned neg = 0u;
    dmw_sort_phase<2>(key, ln, neg);
    dmw_sort_phase<4>(key, ln, neg);
    dmw_sort_phase<8>(key, ln, neg);
    if (Pn >= 16) dmw_sort_phase<16>(key, ln, neg);
    if (Pn >= 32) dmw_sort_phase<32>(key, ln, neg);
    if (Pn >= 64) dmw_sort_phase<64>(key, ln, neg);
    if (Pn >= 128) dmw_sort_phase<128>(key, ln, neg);
    if (Pn >= 256) dmw_sort_phase<256>(key, ln, neg);
    if (Pn >= 512) dmw_sort_phase<512>(key, ln, neg);
  };
  // LDS bitonic sort for frontiers beyond 512 slots (beam > 256)
  auto lds_sort = [&](int P) {
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        wsync();
        for (int c = lane; c < (P >> 1); c += 64) {
          const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1)), l2 = i + j;
          const unsigned long long a = keys[i], b = keys[l2];
          const bool asc = (i & k) == 0;
          const unsigned long long mn = a < b ? a : b, mx = a < b ? b : a;
          keys[i] = asc ? mn : mx; keys[l2] = asc ? mx : mn;
        }
      }
    wsync();
  };
  auto store_keys8 = [&](const unsigned long long (&key)[8], int ln) {
    const int i0 = 8 * ln;
    if (i0 < p.pcap) {
      *(ulonglong2 *)(keys + i0) = make_ulonglong2(key[0], key[1]);
      *(ulonglong2 *)(keys + i0 + 2) = make_ulonglong2(key[2], key[3]);
      *(ulonglong2 *)(keys + i0 + 4) = make_ulonglong2(key[4], key[5]);
      *(ulonglong2 *)(keys + i0 + 6) = make_ulonglong2(key[6], key[7]);
    }
  };

  const int64_t wsb = ((int64_t)blockIdx.x * DMW_NWAVES + wave) * p.ws_cap;

  for (;;) {
    // ================= next user from the global queue =================
    long long user;
    {
      unsigned long long u = 0;
      if (lane == 0) u = atomicAdd(p.next_user, 1ull);
      u = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)u);
      user = u < (unsigned long long)p.U ? (long long)u : -1;
    }
    if (user < 0) break;
    WMARK(6);

    // ================= per-user setup =================
    SMARK(-1);
    if (lane == 0) {
      int beam = p.beam;
      if (p.widen && p.consumed_off) {   // Recommender.recommendItems, Recommender.scala:28-33
        const int nc = (int)(p.consumed_off[user + 1] - p.consumed_off[user]);
        const int w = (nc + p.topk) / 2;
        beam = w > beam ? w : beam;
        if (2 * beam > CAP) beam = CAP / 2;
      }
      const int level = 31 - __clz(beam);        // getLevelStart, :210-216
      const int start = (1 << level) - 1;
      int n_iter = p.mode == 0 ? p.max_level - level + 1 : p.otm_leaf_level - level;
      if (n_iter < 0) n_iter = 0;
      if (n_iter > 34) n_iter = 34;
      misc[M_BEAM] = beam; misc[M_START] = start; misc[M_NITER] = n_iter; misc[M_LVOFF] = 0; misc[M_KEPT] = 0;
      misc[M_GMAX] = 0; misc[M_GSP] = DM_G32;
    }
    {
      // one history position per lane: the id -> code lookups are dependent global loads, L of them in flight at once
      int32_t code = -1;
      if (lane < L) {
        const int32_t id = p.seq[user * L + lane];
        if (p.mode == 1) code = id;             // OTM: node ids, -1 = pad
        else if (id == 0) code = -1;            // TDMTree.idToCode, TDMTree.scala:35-56
        else if (id < p.non_leaf_offset && id >= 0 && p.id_to_code[id] >= 0) code = p.id_to_code[id];
        else {
          const int32_t t = (int32_t)((uint32_t)id - (uint32_t)p.non_leaf_offset);
          code = (t > p.max_code) ? -1 : t;
        }
        if (code < -1 || code >= p.num_index) code = -1;
      }
      if (lane < 16) misc[M_SEQ + lane] = code;          // positions L .. 15 read as pads
      const unsigned pm = (unsigned)__ballot(lane < L && code == -1);
      if (lane == 0) misc[M_PADMASK] = p.use_mask ? pm : 0u;
    }
    wsync();
    SMARK(0);
    // history rows -> K planes;  T1 = K att_w^T;  G = T1 W1b^T + b1   (fp32 MFMA, once per user)
    {
      const int r = lane & 15, g = lane >> 4;
      const int32_t kcode = (r < L) ? misc[M_SEQ + r] : -1;
      f32x4 ka[NJ];
      if (kcode >= 0) {
        const f32x4 *src = (const f32x4 *)(p.emb + (int64_t)kcode * E) + g;    // LookupTable.scala:35-40
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) ka[jc] = src[4 * jc];
      } else {
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) ka[jc] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      float *Gfw = (float *)(slotp + lo.x_gfrag);
      float gm = 0.0f;
      // (G + b1) of rows 4 g .. 4 g + 3, column 16 nt + r, into the fp32 planes; positions past the history are zero
      auto put_g = [&](int r_, int g_, int nt, const f32x4 &acc) {
        if (g_ < KQ) {
          const float bb = B1[16 * nt + r_];
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const float gv = (4 * g_ + rr < L) ? acc[rr] + bb : 0.0f;
            Gfw[(g_ * NT + nt) * 64 + rr * 16 + r_] = gv;
            gm = __builtin_fmaxf(gm, __builtin_fabsf(gv));
          }
        }
      };
      // with the per-row table (BeamParams::g_table) G is one more gather per history position, issued behind the key row's: lane
      // (r, g) takes, for the positions 4 g .. 4 g + 3, the words 16 nt + r of their table rows — what the second product below
      // would leave in its accumulators.  A pad's key row is zero, and so is its product.
      const bool g_tab = p.g_table != nullptr;
      // (an opaque copy of the lane id: the addresses computed from the real one are invariant over the users, get hoisted out
      // of the user loop and spilled)
      int lt = lane;
      asm volatile("" : "+v"(lt));
      const int rt = lt & 15, gt = lt >> 4;
      if (g_tab) {
        float gr[4][NT];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int32_t gcode = misc[M_SEQ + 4 * gt + rr];
          if (gcode >= 0) {
            const float *src = p.g_table + (int64_t)gcode * E + rt;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) gr[rr][nt] = src[16 * nt];
          } else {
#pragma unroll
            for (int nt = 0; nt < NT; nt++) gr[rr][nt] = 0.0f;
          }
        }
        DMW_FOR(NT, nt)
          put_g(rt, gt, nt, (f32x4){gr[0][nt], gr[1][nt], gr[2][nt], gr[3][nt]});
        DMW_END
      }
      if (rt < KCOLS) {
        dm_h8 *Khw = (dm_h8 *)(slotp + lo.x_kfrag);
#pragma unroll
        for (int s = 0; s < NS; s++) {
          dm_h8 hi, lw;
          dm_split8(ka[2 * s], ka[2 * s + 1], p.emb_scale, hi, lw);
          Khw[(s * 4 + gt) * KCOLS + rt] = hi;
          Khw[((NS + s) * 4 + gt) * KCOLS + rt] = lw;
        }
      }
      SMARK(1);
      if (!g_tab) {
        // T1 = K att_w^T;  G = T1 W1b^T  (dmw_gemm16), once per user
        float *T1s = (float *)(slotp + lo.y_keys);          // [16][E + 4]
        dmw_gemm16<E>(p.afrag, ka, lane, [&](int nt, const f32x4 &acc) { dmw_t1_put<E>(T1s, r, g, nt, acc); });
        wsync();
        SMARK(2);
        f32x4 ta[NJ];
        dmw_t1_get<E>(T1s, r, g, ta);
        dmw_gemm16<E>(p.bfrag, ta, lane, [&](int nt, const f32x4 &acc) { put_g(r, g, nt, acc); });
        SMARK(3);
      }
      unsigned gbits = __float_as_uint(gm);
      gbits = gbits < 0x7f800000u ? gbits : 0x7f800000u;     // NaN counts as "out of range"
      for (int o = 32; o > 0; o >>= 1) { const unsigned t_ = (unsigned)__shfl_xor((int)gbits, o); gbits = t_ > gbits ? t_ : gbits; }
      wsync();
      // (G + b1) * 2^sg as fp16 [hi | lo] against p * 2^sp, sg + sp = the accumulator scale; outside the fp16 range the user
      // keeps the fp32-input product (same rule as beam_kernel.hip.inc)
      const int S = (int)((__float_as_uint(p.acc_scale) >> 23) & 0xff) - 127;
      int sp = DM_G32;
      if (gbits < 0x7f800000u) {
        const int e = gbits ? (int)(gbits >> 23) - 126 : -126;
        sp = S - (14 - e);
        if (sp < -10) sp = -10;
        if (sp > 15) sp = DM_G32;
      }
      constexpr int NENT = NT * 64;           // one dm_h8 per (feature tile, lane)
      constexpr int NQ = (NENT + 63) / 64;
      if constexpr (FOLD) {
        // the folded layout: half k of lane group g_ is the G part of the (position, term) that owns slot (g_, k) — dmw_fold_slot
        if (sp != DM_G32) {
          const float gs = __uint_as_float((unsigned)(S - sp + 127) << 23);
          float gv[NQ][8];
#pragma unroll
          for (int q = 0; q < NQ; q++) {
            const int idx = lt + 64 * q;
            const int nt_ = (idx >> 6) % NT, m_ = idx & 15, g_ = (idx >> 4) & 3;
            DMW_FOR(8, k)
              const int pos = (int)((dmw_fold_pos_nibbles(k) >> (4 * g_)) & 15u);
              const int posc = pos < 4 * KQ ? pos : 0;
              const float v = Gfw[((posc >> 2) * NT + nt_) * 64 + (posc & 3) * 16 + m_] * gs;
              gv[q][k] = pos < 4 * KQ ? v : 0.0f;
            DMW_END
          }
          wsync();   // every fp32 value has been read: the planes overwrite the region
          typedef float f32x2_ __attribute__((ext_vector_type(2)));
#pragma unroll
          for (int q = 0; q < NQ; q++) {
            float x[8];
            DMW_FOR(8, k)     // a G_lo slot holds what the fp16 hi part leaves of the value
              x[k] = dmw_fold_g_lo(k) ? gv[q][k] - (float)(_Float16)gv[q][k] : gv[q][k];
            DMW_END
            const dm_h2 h01 = __builtin_convertvector((f32x2_){x[0], x[1]}, dm_h2), h23 = __builtin_convertvector((f32x2_){x[2], x[3]}, dm_h2);
            const dm_h2 h45 = __builtin_convertvector((f32x2_){x[4], x[5]}, dm_h2), h67 = __builtin_convertvector((f32x2_){x[6], x[7]}, dm_h2);
            dm_h8 o;
            o[0] = h01[0]; o[1] = h01[1]; o[2] = h23[0]; o[3] = h23[1]; o[4] = h45[0]; o[5] = h45[1]; o[6] = h67[0]; o[7] = h67[1];
            ((dm_h8 *)Gfw)[lt + 64 * q] = o;
          }
        } else {
          for (int i = lane; i < KQ * NT * 64; i += 64) Gfw[i] *= p.acc_scale;
        }
      } else if (sp != DM_G32) {
        const float gs = __uint_as_float((unsigned)(S - sp + 127) << 23);
        float gv[NQ][4];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
          const int idx = lane + 64 * q;
          const int nt_ = (idx >> 6) % NT, m_ = idx & 15, g_ = (idx >> 4) & 3;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int pos = g_ + 4 * i;
            gv[q][i] = ((pos >> 2) < KQ) ? Gfw[((pos >> 2) * NT + nt_) * 64 + (pos & 3) * 16 + m_] * gs : 0.0f;
          }
        }
        wsync();   // every fp32 value has been read: the planes overwrite the region
        typedef float f32x2_ __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int q = 0; q < NQ; q++) {
          const int idx = lane + 64 * q;
          const dm_h2 h01 = __builtin_convertvector((f32x2_){gv[q][0], gv[q][1]}, dm_h2);
          const dm_h2 h23 = __builtin_convertvector((f32x2_){gv[q][2], gv[q][3]}, dm_h2);
          const dm_h2 l01 = __builtin_convertvector((f32x2_){gv[q][0] - (float)h01[0], gv[q][1] - (float)h01[1]}, dm_h2);
          const dm_h2 l23 = __builtin_convertvector((f32x2_){gv[q][2] - (float)h23[0], gv[q][3] - (float)h23[1]}, dm_h2);
          dm_h8 o;
          o[0] = h01[0]; o[1] = h01[1]; o[2] = h23[0]; o[3] = h23[1]; o[4] = l01[0]; o[5] = l01[1]; o[6] = l23[0]; o[7] = l23[1];
          ((dm_h8 *)Gfw)[idx] = o;
        }
      } else {
        for (int i = lane; i < KQ * NT * 64; i += 64) Gfw[i] *= p.acc_scale;
      }
      if (lane == 0) misc[M_GSP] = sp;
    }
    wsync();
    SMARK(4);
    // Users whose (G + b1) does not fit the fp16 range against p (DESIGN.md §3 "Scaling") keep the fp32-input product for the
    // attention-combine term.  Rare (never with the reference's zero-initialised biases): they are handed to the LDS-fed kernel,
    // which carries that path, through a list in global memory — so that this kernel's tile loop has ONE path and no branch.
    if (__builtin_amdgcn_readfirstlane(misc[M_GSP]) == DM_G32) {
      if (lane == 0) { const unsigned long long q = atomicAdd(p.defer_count, 1ull); p.defer_users[q] = (int32_t)user; }
      continue;
    }
    // initial frontier: codes [start, 2*start+1) that exist, pred 0 (Recommender.scala:53-56)
    int n_cand;
    int lv0;          // the level of the initial frontier
    {
      const int start = misc[M_START];
      const int n_iter0 = misc[M_NITER];
      int32_t *A0 = (int32_t *)(slotp + lo.y_acode0);
      int base = 0;
      // the start level's bound (the user's own level: widened beams start at different ones): its existing codes are the run
      // start .. last, so the frontier is start .. min(2 start, last) — no bit loads, no scan
      lv0 = 31 - __clz(__builtin_amdgcn_readfirstlane(start) + 1);
      const int last0 = __builtin_amdgcn_readfirstlane(LB[lv0]);
      if (last0 != DM_LEVEL_USE_BITS) {
        const int hi0 = 2 * start < last0 ? 2 * start : last0;
        base = (n_iter0 > 0 && hi0 >= start) ? hi0 - start + 1 : 0;
#pragma unroll 1
        for (int i = lane; i < base; i += 64) { A0[i] = start + i; A_val[i] = 0.0f; }
      } else
      for (int r0 = 0; r0 < CAP / 2; r0 += 256) {
        unsigned bits = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int i = r0 + 4 * lane + j;
          const int64_t code = (int64_t)start + i;
          bool ok = n_iter0 > 0 && i <= start;
          if (ok && p.mode == 0) ok = code < p.n_slots && dm_bit(p.exists_bits, code);
          bits |= ok ? (1u << j) : 0u;
        }
        int total;
        const int before = scan4(bits, total);
#pragma unroll
        for (int j = 0; j < 4; j++)
          if ((bits >> j) & 1u) {
            const int q = base + before + __popc(bits & ((1u << j) - 1));
            A0[q] = start + r0 + 4 * lane + j; A_val[q] = 0.0f;
          }
        base += total;
      }
      n_cand = base;
    }
    wsync();

    const int n_iter = misc[M_NITER];
    const int beam = misc[M_BEAM];
    const unsigned padmask = (unsigned)misc[M_PADMASK];
    const int gsp = __builtin_amdgcn_readfirstlane(misc[M_GSP]);
    const float pscale = gsp != DM_G32 ? __uint_as_float((unsigned)(gsp + 127) << 23) : 1.0f;
    int cur = 0;
    int leaf_tot = 0;
    SMARK(5);
    WMARK(0);

    // ================= level loop =================
    for (int it = 0; it < n_iter; it++) {
      int32_t *Acur = (int32_t *)(slotp + (cur ? lo.y_acode1 : lo.y_acode0));
      int32_t *Anext = (int32_t *)(slotp + (cur ? lo.y_acode0 : lo.y_acode1));
      const int n = n_cand;
      const bool first = (it == 0);
      int m_nl = n;
      int leaf_base = leaf_tot;
      int nchild = 0;
      // per-lane addresses of the bookkeeping phases are derived from an OPAQUE copy of the lane id: computed from the real one
      // they are loop-invariant, get hoisted out of the user loop, kept alive through the tile loop and spilled (each use then
      // opens with a scratch reload)
      int ln = lane;
      asm volatile("" : "+v"(ln));
      // the existence bound of the children's level (wave-uniform; DM_LEVEL_USE_BITS: the level has none, or OTM)
      const int clv = lv0 + it + 1;
      const int lastc = __builtin_amdgcn_readfirstlane(LB[clv < DM_N_LEVEL_BOUNDS ? clv : DM_N_LEVEL_BOUNDS - 1]);
      // ---- P1: split leaves / non-leaves, in order (Recommender.scala:62-70) ----
      if (p.mode == 0) {
        if (p.leaf_fast) {
          if (it == n_iter - 1) {
            for (int i = ln; i < n; i += 64) {
              const int q = leaf_base + i;
              if (q < p.ws_cap) { p.ws_code[wsb + q] = Acur[i]; p.ws_score[wsb + q] = A_val[i]; }
            }
            leaf_base += n; m_nl = 0;
          }
        } else {
          int nl = 0;
          for (int r0 = 0; r0 < n; r0 += 256) {
            unsigned lbits = 0, nbits = 0;
            int32_t cc[4]; float vv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const int i = r0 + 4 * ln + j;
              const bool valid = i < n;
              cc[j] = valid ? Acur[i] : 0; vv[j] = valid ? A_val[i] : 0.0f;
              const bool isleaf = valid && dm_bit(p.leaf_bits, cc[j]);
              lbits |= isleaf ? (1u << j) : 0u;
              nbits |= (valid && !isleaf) ? (1u << j) : 0u;
            }
            int tl, tn;
            const int bl = scan4(lbits, tl);
            const int bn = scan4(nbits, tn);
            wsync();                       // every read of this round is done before the compaction writes
#pragma unroll
            for (int j = 0; j < 4; j++) {
              if ((nbits >> j) & 1u) { const int q = nl + bn + __popc(nbits & ((1u << j) - 1)); Acur[q] = cc[j]; A_val[q] = vv[j]; }
              if ((lbits >> j) & 1u) {
                const int q = leaf_base + bl + __popc(lbits & ((1u << j) - 1));
                if (q < p.ws_cap) { p.ws_code[wsb + q] = cc[j]; p.ws_score[wsb + q] = vv[j]; }
              }
            }
            nl += tn; leaf_base += tl;
            wsync();
          }
          m_nl = nl;
        }
        leaf_tot = leaf_base;
        if (lane == 0) misc[M_LVOFF + it + 1] = leaf_base;
      }
      // ---- P2: stable top-beam (Recommender.scala:74-87 / CandidateSearcher.scala:117-120) ----
      const bool do_sort = (p.mode == 0) ? (m_nl > beam) : !first;
      const int nb = do_sort ? (m_nl < beam ? m_nl : beam) : m_nl;
      if (do_sort) {
        int P = 2;
        while (P < m_nl) P <<= 1;
        if (P <= 512) {
          // 8 consecutive scores per lane in two 16-byte LDS reads (slots past m_nl hold stale values: masked to the padding key)
          unsigned long long key[8];
          const int rd = 8 * ln + 8 <= CAP ? 8 * ln : 0;
          const f32x4 v0 = *(const f32x4 *)(A_val + rd), v1 = *(const f32x4 *)(A_val + rd + 4);
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const int i = 8 * ln + e;
            const float sc = e < 4 ? v0[e & 3] : v1[e & 3];
            key[e] = (i < m_nl) ? dmw_make_key(sc, (unsigned)i) : DMW_KEY_PAD;
          }
          reg_sort8(key, P);
          store_keys8(key, ln);
        } else {
          for (int i = ln; i < P; i += 64)
            keys[i] = (i < m_nl) ? dmw_make_key(A_val[i], (unsigned)i) : DMW_KEY_PAD;
          lds_sort(P);
        }
        wsync();
      }
      WMARK(1);
      // ---- P3: children 2c+1, 2c+2 of the beam, in beam order, existence-filtered (:88-92) ----
      // eight children (four parents) per lane and round: the existence bits of a whole 512-slot frontier are one round of loads
      for (int r0 = 0; r0 < 2 * nb; r0 += 512) {
        unsigned bits = 0, vbits = 0;
        int64_t ch[8];
        bool ok[8];
        // the four parents' LDS reads as TWO rounds, not eight: every key position is read without a condition (an unsorted
        // level selects the slot's own index instead; the key area is the wave's own LDS either way) — under `do_sort ? :` each
        // key read sat in a branch of its own with a wait behind it, one dependent round trip after the other
        // (the scheduling barriers keep the rounds apart: left alone the scheduler waits for one read before it issues the next)
        int ppic[4];
        uint32_t pkey[4];
        int32_t ppc[4];
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) {
          const int pi = (r0 >> 1) + 4 * ln + j2;
          ppic[j2] = pi < nb ? pi : 0;
        }
        DMW_PIN();
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) pkey[j2] = ((const uint32_t *)keys)[2 * ppic[j2]];
        DMW_PIN();
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) ppic[j2] = do_sort ? (int)DMW_KEY_POS(pkey[j2]) : ppic[j2];
        DMW_PIN();
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) ppc[j2] = Acur[ppic[j2]];
        DMW_PIN();
#pragma unroll
        for (int j2 = 0; j2 < 4; j2++) {
          const int pi = (r0 >> 1) + 4 * ln + j2;
          const bool valid = pi < nb;
          vbits |= valid ? (3u << (2 * j2)) : 0u;
          const int32_t pc = ppc[j2];
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const int64_t c = (int64_t)pc * 2 + 1 + h;
            ch[2 * j2 + h] = c;
            ok[2 * j2 + h] = valid && c < p.num_index && (p.mode != 0 || c < p.n_slots);
          }
        }
        const bool bounded = lastc != DM_LEVEL_USE_BITS;          // (never in mode 1: its LB reads "use the bits")
        if (bounded) {
          // the level's existing codes are the run first .. lastc: no load, the answer is a compare
#pragma unroll
          for (int j = 0; j < 8; j++) ok[j] = ok[j] && ch[j] <= (int64_t)lastc;
        } else if (p.mode == 0) {
          uint32_t w[8];
#pragma unroll
          for (int j = 0; j < 8; j++) w[j] = ok[j] ? p.exists_bits[ch[j] >> 5] : 0u;
#pragma unroll
          for (int j = 0; j < 8; j++) ok[j] = ok[j] && ((w[j] >> (ch[j] & 31)) & 1u);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) bits |= ok[j] ? (1u << j) : 0u;
        if (bounded && __ballot(bits != vbits) == 0ull) {
          // every child of this round's parents exists: the ordered compaction is the identity (lane ln's eight children are
          // elements 8 ln .. 8 ln + 7 of the round, and the parents of a round are a prefix of its slots)
          const int rem = 2 * nb - r0;
#pragma unroll
          for (int j = 0; j < 8; j++)
            if ((bits >> j) & 1u) Anext[nchild + 8 * ln + j] = (int32_t)ch[j];
          nchild += rem < 512 ? rem : 512;
        } else {
          int total;
          const int before = scan8(bits, total);
#pragma unroll
          for (int j = 0; j < 8; j++)
            if ((bits >> j) & 1u) Anext[nchild + before + __popc(bits & ((1u << j) - 1))] = (int32_t)ch[j];
          nchild += total;
        }
      }
      n_cand = nchild;
      cur ^= 1;
      wsync();
      WMARK(2);

      // ---- P4: score the children, 16-row tiles, software-pipelined over three tiles ----
      {
        const int32_t *codes = Anext;
        const int ncs = __builtin_amdgcn_readfirstlane(nchild);      // wave-uniform: loop control on the SALU
        const int tot = (ncs + 15) >> 4;
        const int r = lane & 15, g = lane >> 4;
        // a tile's fp16 operands come straight from the pre-split table (dm_build_emb_split_kernel): per row and k-step s the
        // lane group g finds [hi 8 halfs | lo 8 halfs] = the B operands of v_mfma_f32_16x16x32_f16, 32 contiguous bytes
        auto row_ptr = [&](int tile) -> const dm_h8 * {
          const int row = tile * 16 + r;
          const int32_t code = codes[row < ncs ? row : ncs - 1];
          return p.emb_split + (int64_t)code * (E / 4) + 2 * g;       // E / 4 dm_h8 entries per row
        };
        const int kpos = (r >> 2) + 4 * (r & 3);
        const int kfi = g * KCOLS + (kpos < KCOLS - 1 ? kpos : KCOLS - 1);
        float smul[4], sadd[4];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const bool ispad = (padmask >> (g + 4 * rr)) & 1u, inval = g + 4 * rr >= L;
          smul[rr] = (ispad || inval) ? 0.0f : scale2;
          sadd[rr] = inval ? -INFINITY : (ispad ? -FLT_MAX : 0.0f);
        }
        const dm_h8 *Gh = (const dm_h8 *)Gf;

        // ---- register-resident state of the pipeline
        dm_h8 ah[NS], al[NS], zh[NS], zl[NS];    // operand sets of even / odd tiles (hi, lo per k-step): three tiles are in flight —
                                                // a set's k-step is re-loaded with the tile after next as soon as it has been multiplied
        f32x4 acc[NT];                // H^T accumulators; the finished tile's are read by its epilogue under the next tile's first MFMAs
        // from here to the end of the tile loop the outstanding loads are the gathers below, in order.  The builtin (not the
        // assembly wait), and on EVERY path into the loop: the compiler has to know that none of its own loads or stores is
        // pending, or it waits for them (that is: for the newest gathers) inside the loop
        __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0), expcnt / lgkmcnt untouched
        if (tot > 0) {
          const dm_h8 *s0p = row_ptr(0), *s1p = row_ptr(tot > 1 ? 1 : 0);
          DMW_FOR(NS, s) dmw_gather16<128 * s>(ah[s], s0p); dmw_gather16<128 * s + 16>(al[s], s0p); DMW_END
          DMW_FOR(NS, s) dmw_gather16<128 * s>(zh[s], s1p); dmw_gather16<128 * s + 16>(zl[s], s1p); DMW_END
        }
        // relu as ONE integer max (sign bit set <=> negative as an int; the accumulators come out of assembly, so a float
        // max would first be canonicalised); two partial sums halve the dependent-FMA chain; the w2 vector of a feature tile is
        // fetched from LDS one whole piece ahead.  Element rr of piece nt is one (max, fma) pair: it rides behind one MFMA.
        f32x4 wwc = *(const f32x4 *)(W2 + 4 * g), wwn = wwc;
        float epart0 = 0.f, epart1 = 0.f;
        auto epi_elem = [&](int nt, int rr) {
          if (rr == 0) { wwc = wwn; wwn = *(const f32x4 *)(W2 + 16 * ((nt + 1) % NT) + 4 * g); }
          const int hb = __float_as_int(acc[nt][rr]);
          const float hv = __int_as_float(hb > 0 ? hb : 0);
          if (rr & 1) epart1 = fmaf(hv, wwc[rr], epart1); else epart0 = fmaf(hv, wwc[rr], epart0);
        };
        float exl = 0.f, epart = 0.f;           // the epilogue's cross-lane exchange in flight
        auto epi_finish = [&](int tile, int step) {      // tile == -1 (nothing finished yet): only the reset
          if (step == 0) { epart = epart0 + epart1; exl = dm_xor16(epart); }
          else if (step == 1) { epart += exl; exl = dm_xor32(epart); }
          else {
            const int orow = tile * 16 + r;
            if (g == 0 && tile >= 0 && orow < ncs) A_val[orow] = (epart + exl) + p.b2;
            epart0 = 0.f; epart1 = 0.f;
          }
        };
        constexpr int GPS = NT / NB;               // W1a-chain groups (of three batches) per k-step
        constexpr int EPG = GPS >= 2 ? NB / 2 : 0; // epilogue pieces that ride behind the LAST group of the attention-combine product
        constexpr int NSLOT = 3 * NGRP;            // gaps between the batches of the W1a chain: 24 at E = 128
        // the user's key fragments for this lane: fetched from LDS at the END of a tile for the next one, so that the score
        // MFMAs that open a tile never wait for LDS (and nothing keeps 32 registers busy through the W1a chain)
        dm_h8 kf0[NS], kf1[NS];
        auto load_keys = [&]() {
#pragma unroll
          for (int s = 0; s < NS; s++) { kf0[s] = Kh[s * 4 * KCOLS + kfi]; kf1[s] = Kh[(NS + s) * 4 * KCOLS + kfi]; }
        };
        load_keys();
        WMARK(3);

#ifdef DM_TILE_TIMERS
        tt_last = clock64();
#endif
        auto do_tile = [&](int tile, dm_h8 (&bh)[NS], dm_h8 (&bl)[NS]) {
          const dm_h8 *nsrc = row_ptr(tile + 2 < tot ? tile + 2 : tot - 1);      // the tile that takes over this set (clamped: a re-read, never used)
          DMW_PIN();
          // ---- scores S^T = K Q^T: hi*hi, hi*lo, lo*hi on three accumulation chains.  Behind each MFMA rides its share of the
          //      first NB epilogue pieces of the previous tile (those accumulators are the first the W1a chain rewrites; at
          //      tile 0 they run on stale accumulators and the result is dropped: no branch inside the MFMA stream)
          f32x4 s0, s1, s2;
          DMW_FOR(NS, s)
            // k-step s of this set: behind its lo half were issued the later k-steps of the set and the other set's whole tile
            dmw_vmwait<2 * (NS - 1 - s) + 2 * NS>();
            DMW_FOR(3, m)
              if constexpr (m == 0) { if constexpr (s == 0) dmw_mfma_vv0(s0, kf0[s], bh[s]); else dmw_mfma_vv(s0, kf0[s], bh[s]); }
              else if constexpr (m == 1) { if constexpr (s == 0) dmw_mfma_vv0(s1, kf0[s], bl[s]); else dmw_mfma_vv(s1, kf0[s], bl[s]); }
              else { if constexpr (s == 0) dmw_mfma_vv0(s2, kf1[s], bh[s]); else dmw_mfma_vv(s2, kf1[s], bh[s]); }
              DMW_PIN();
              // (when the attention-combine product has a second group, the first EPG pieces already ran behind it).  The pieces
              // go one after the other — each fetches the NEXT piece's w2 vector — spread over the 3 NS gaps of this region
              DMW_FOR(4 * (NB - EPG), el)
                if constexpr ((el * 3 * NS) / (4 * (NB - EPG)) == 3 * s + m) epi_elem(EPG + el / 4, el % 4);
              DMW_END
              DMW_PIN();
            DMW_END
          DMW_END
          TMARK(0);
          // ---- W1a chain, A operands from the AccVGPRs, with the remaining VALU work of three tiles in its shadow
          float x[4], e[4], mx = 0.f, sum = 0.f;
          f32x4 pr = {0.f, 0.f, 0.f, 0.f};
          dm_h8 pb0, pb1;
          dm_h8 gvv[NT];                    // (G + b1) fragments, fetched from LDS in the last gaps of the W1a chain
          float xl = 0.f;        // a cross-lane exchange in flight: issued behind one MFMA, consumed >= 4 MFMAs later (LDS crossbar latency)
          typedef float f32x2_ __attribute__((ext_vector_type(2)));
          dm_h2 p01, p23, q01, q23;
          typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
          unsigned xq = 0u;      // folded product: the p_lo half received from the lane 32 further
          // Mask.scala:17-35, SoftMax.scala:28-42 in the base-2 domain (4 positions in the lane, 12 in lanes r+16, r+32, r+48),
          // cut into 18 items of 1-4 VALU instructions; item k rides behind the MFMA at position dmw_sm_pos(k) of the chain
          auto softmax_item = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if constexpr (k < 4) {
              if constexpr (k == 0 && NSLOT < 10) asm volatile("s_nop 7" : "+v"(s0), "+v"(s1), "+v"(s2));
              x[k] = fmaf((s0[k] + s1[k]) + s2[k], smul[k], sadd[k]);
            } else if constexpr (k == 4) { mx = __builtin_fmaxf(__builtin_fmaxf(x[0], x[1]), __builtin_fmaxf(x[2], x[3])); xl = dm_xor16(mx); }
            else if constexpr (k == 5) { mx = __builtin_fmaxf(mx, xl); xl = dm_xor32(mx); }
            else if constexpr (k == 6) { mx = __builtin_fmaxf(mx, xl); e[0] = __builtin_amdgcn_exp2f(x[0] - mx); }
            else if constexpr (k < 10) { e[k - 6] = __builtin_amdgcn_exp2f(x[k - 6] - mx); }
            else if constexpr (k == 10) { sum = (e[0] + e[1]) + (e[2] + e[3]); xl = dm_xor16(sum); }
            else if constexpr (k == 11) { sum += xl; xl = dm_xor32(sum); }
            else if constexpr (k == 12) { sum += xl; sum = __builtin_amdgcn_rcpf(sum) * pscale; }
            else if constexpr (k == 13) { pr[0] = e[0] * sum; pr[1] = e[1] * sum; }
            else if constexpr (k == 14) { pr[2] = e[2] * sum; pr[3] = e[3] * sum; }
            else if constexpr (k == 15) { p01 = __builtin_convertvector((f32x2_){pr[0], pr[1]}, dm_h2); p23 = __builtin_convertvector((f32x2_){pr[2], pr[3]}, dm_h2); }
            else if constexpr (k == 16) {
              q01 = __builtin_convertvector((f32x2_){pr[0] - (float)p01[0], pr[1] - (float)p01[1]}, dm_h2);
              q23 = __builtin_convertvector((f32x2_){pr[2] - (float)p23[0], pr[3] - (float)p23[1]}, dm_h2);
              // folded product: p_lo of positions 8, 9 goes to the lane 32 further (slot 2 of group g + 2, dmw_fold_slot)
              if constexpr (FOLD && KQ >= 3) xq = (unsigned)__shfl_xor((int)__builtin_bit_cast(unsigned, q23), 32);
            } else if constexpr (FOLD) {
              // [ph0 ph1 ph2|X pl0 | ph0 ph1 ph2 pl1]: of ph2 and the received X = pl2 one is +0 in every lane (dmw_fold_p_item)
              const unsigned u01 = __builtin_bit_cast(unsigned, p01), u23 = __builtin_bit_cast(unsigned, p23), v01 = __builtin_bit_cast(unsigned, q01);
              const unsigned lo2 = u23 & 0xffffu;
              const u32x4_ pu = {u01, (lo2 | (xq & 0xffffu)) | (v01 << 16), u01, lo2 | (v01 & 0xffff0000u)};
              pb0 = __builtin_bit_cast(dm_h8, pu);
            } else {
              pb0 = (dm_h8){p01[0], p01[1], p23[0], p23[1], p01[0], p01[1], p23[0], p23[1]};
              pb1 = (dm_h8){q01[0], q01[1], q23[0], q23[1], 0, 0, 0, 0};
            }
          };
          // the work of gap `slot`, cut once more: `sub` = which MFMA of the batch it rides behind (0 .. NB-1)
          // The W1a chain runs accumulator group by accumulator group (all k-steps of accumulators 0..NB-1, then of NB..2NB-1):
          // the second group's accumulators keep the previous tile's values for half the chain, so their epilogue spreads
          // over NPOS/2 positions instead of three gaps.  Position = index of the MFMA a piece of work rides behind.
          constexpr int NPOS = NSLOT * NB;           // 96 at E = 128
          constexpr int HALF = NPOS / GPS;           // positions per accumulator group
          auto filler = [&](auto pos_c) {
            constexpr int pos = decltype(pos_c)::value;
            // softmax: 18 items, evenly spread (a cross-lane result is consumed >= 5 MFMAs after its issue)
#ifdef DMW_DBG_SM_UPTO
            DMW_FOR(DMW_DBG_SM_UPTO, k) if constexpr ((NPOS >= 96 ? 2 + 5 * k : (k * NPOS) / 18) == pos) softmax_item(k_c); DMW_END
#else
            DMW_FOR(18, k) if constexpr ((NPOS >= 96 ? 2 + 5 * k : (k * NPOS) / 18) == pos) softmax_item(k_c); DMW_END
#endif
            // epilogue of the previous tile's accumulators NB .. NT-1: before the second group starts
            if constexpr (GPS >= 2) {
              DMW_FOR(4 * (NT - NB), el) if constexpr ((el * HALF) / (4 * (NT - NB)) == pos) epi_elem(NB + el / 4, el % 4); DMW_END
            }
            DMW_FOR(3, st)
              constexpr int fp = (GPS >= 2 ? HALF : 0) + 6 * st + 1;
              if constexpr (pos == (fp < NPOS ? fp : NPOS - 1)) epi_finish(tile - 1, st);
            DMW_END
            // (G + b1) fragments for the attention-combine product, in the last positions
#ifndef DMW_DBG_NO_GVV
            DMW_FOR(NT, f) if constexpr (pos == (NPOS - 3 * NT + 2 * f > 0 ? NPOS - 3 * NT + 2 * f : 0)) gvv[f] = Gh[f * 64 + lane]; DMW_END
#endif
            // k-step s of this operand set was last multiplied at the end of the LAST group's k-step s: one batch of slack
            // later its registers take the tile after next
            DMW_FOR(NS - 1, s)
              constexpr int free_pos = ((GPS - 1) * NS + s + 1) * 3 * NB + NB;
#ifndef DMW_DBG_NO_GATHER
              if constexpr (pos == (free_pos < NPOS ? free_pos : NPOS - 1)) { dmw_gather16<128 * s>(bh[s], nsrc); dmw_gather16<128 * s + 16>(bl[s], nsrc); }
#endif
            DMW_END
          };
          DMW_FOR(GPS, gg)
            DMW_FOR(NS, s)
              constexpr int nb0 = gg * NB, base = (gg * NS + s) * 3 * NB;
              // a batch = NB MFMAs on NB different accumulators; behind EACH MFMA rides the work placed at its position
              DMW_FOR(NB, i)
                if constexpr (s == 0) dmw_mfma_av0(acc[nb0 + i], wreg[(NS + s) * NT + nb0 + i], bh[s]);
                else dmw_mfma_av(acc[nb0 + i], wreg[(NS + s) * NT + nb0 + i], bh[s]);
                DMW_PIN(); filler(std::integral_constant<int, base + i>{}); DMW_PIN();
              DMW_END
              DMW_FOR(NB, i)
                dmw_mfma_av(acc[nb0 + i], wreg[s * NT + nb0 + i], bl[s]);
                DMW_PIN(); filler(std::integral_constant<int, base + NB + i>{}); DMW_PIN();
              DMW_END
              DMW_FOR(NB, i)
                dmw_mfma_av(acc[nb0 + i], wreg[s * NT + nb0 + i], bh[s]);
                DMW_PIN(); filler(std::integral_constant<int, base + 2 * NB + i>{}); DMW_PIN();
              DMW_END
            DMW_END
            TMARK(1 + gg);
          DMW_END
          // ---- H^T += (G + b1)^T P^T.  Behind its MFMAs: the split of the last k-step of the next tile, and — behind the LAST
          //      group — the epilogue elements of this tile's first EPG accumulators (final since the group before)
          if constexpr (FOLD) {
            // one MFMA per feature tile: the three terms of every position share its 32 contraction slots (dmw_fold_slot)
            asm volatile("s_nop 1" : "+v"(pb0));
            load_keys();                 // the next tile's score MFMAs open with these: a whole product of slack
            DMW_FOR(GPS, gg)
              constexpr int nb0 = gg * NB;
              DMW_FOR(NB, ii)
                dmw_mfma_vv(acc[nb0 + ii], gvv[nb0 + ii], pb0);
                DMW_PIN();
#ifndef DMW_DBG_NO_GATHER
                if constexpr (gg == 0 && ii == 1 % NB) dmw_gather16<128 * (NS - 1)>(bh[NS - 1], nsrc);
                if constexpr (gg == 0 && ii == 2 % NB) dmw_gather16<128 * (NS - 1) + 16>(bl[NS - 1], nsrc);
#endif
                if constexpr (EPG > 0 && gg == GPS - 1) {
                  DMW_FOR(4 * EPG, el) if constexpr ((el * NB) / (4 * EPG) == ii) epi_elem(el / 4, el % 4); DMW_END
                }
                DMW_PIN();
              DMW_END
            DMW_END
          } else {
            asm volatile("s_nop 1" : "+v"(pb0), "+v"(pb1));
            load_keys();                 // the next tile's score MFMAs open with these: a whole product of slack
            constexpr int NGAP = 2 * GPS;
            DMW_FOR(GPS, gg)
              constexpr int nb0 = gg * NB;
              DMW_FOR(2 * NB, ii)
                constexpr int i = ii % NB, half = ii / NB;
                if constexpr (half == 0) dmw_mfma_vv(acc[nb0 + i], gvv[nb0 + i], pb1); else dmw_mfma_vv(acc[nb0 + i], gvv[nb0 + i], pb0);
                DMW_PIN();
#ifndef DMW_DBG_NO_GATHER
                if constexpr (gg == 0 && ii == 1) dmw_gather16<128 * (NS - 1)>(bh[NS - 1], nsrc);
                if constexpr (gg == 0 && ii == 2 % (2 * NB)) dmw_gather16<128 * (NS - 1) + 16>(bl[NS - 1], nsrc);
#endif
                if constexpr (EPG > 0 && gg == GPS - 1) {
                  DMW_FOR(4 * EPG, el) if constexpr ((el * 2 * NB) / (4 * EPG) == ii) epi_elem(el / 4, el % 4); DMW_END
                }
                DMW_PIN();
              DMW_END
            DMW_END
          }
          TMARK(1 + GPS);
          TMARK(2 + GPS);
        };
        // ---- E = 128: the same tile, its VALU work placed by hand at TWO instructions per gap at most.  Measured with one
        //      wave per SIMD (tools/gap_filler_microbench.hip): behind a v_mfma_f32_16x16x32_f16 two VALU instructions, an LDS or
        //      global load, a DPP move or a swizzle are free (16.3 -> 16.4 cycles per MFMA); a third VALU instruction costs 4
        //      cycles, a packed-fp32 one (v_pk_fma / v_pk_add / v_pk_mul_f32) 17 — it holds the matrix pipe — and a load whose
        //      result is read in the same gap its whole latency.  So: scalar fp32 only (the library is built with
        //      -fno-slp-vectorize: the vectoriser packs adjacent scalar adds and fmas), one epilogue element (relu + fma) or two
        //      softmax instructions per gap, every cross-lane or LDS result read six gaps later.
        //      Gaps of a tile: 0..11 behind the score MFMAs, 12..107 behind the W1a chain, 108..123 behind the
        //      attention-combine product.  The 32 epilogue elements of tile t: pieces 0..3 (accumulators final half way through
        //      t's last product) behind t's last ten MFMAs and the next tile's score MFMAs; pieces 4..7 behind every third
        //      MFMA of the next tile's first accumulator group.
        //      FOLD: the attention-combine product is 8 MFMAs (gaps 108..115, 116 gaps per tile) and pieces 0..3 are final after
        //      its first four.  Their elements keep the distance (in gaps) they had behind the MFMA that finalises their
        //      accumulator: five behind this tile's last MFMAs, nine behind the next tile's score MFMAs, the last two in the
        //      free gaps 1 and 2 of its W1a chain (accumulator 3 is rewritten at chain position 3); pieces 4..7 follow at chain
        //      positions 3, 6, .. 45 and 46 (the elements run in order: each piece fetches the next one's w2 vector).
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
        u32x4_ pbu0 = {0u, 0u, 0u, 0u}, pbu1 = {0u, 0u, 0u, 0u};       // the P operands; pbu1 lanes 2, 3 stay zero (FOLD: pbu0 alone)
        constexpr int FG_S = 3 * NS, FG_W = 3 * NS + 3 * NGRP * NB;          // 12, 108
        constexpr int FG_N = FG_W + (FOLD ? 1 : 2) * GPS * NB;               // gaps per tile: 124, FOLD 116
        constexpr auto el_gap = [](int el) constexpr -> int {
          if constexpr (FOLD) {
            // accumulator n is final four MFMAs earlier than unfolded, so its elements sit four gaps earlier, counted on from the
            // product's first MFMA: 2 3 4 6 | 7 8 10 11 | 13 14 15 17 | 18 19 21 22 for pieces 0 | 1 | 2 | 3
            if (el >= 16) return el < 31 ? FG_S + 3 + 3 * (el - 16) : FG_S + 46;
            const int pos = 2 + (el * 22) / 16;
            return pos < FG_N - FG_W ? FG_W + pos : pos - (FG_N - FG_W);
          }
          if (el >= 16) return FG_S + 3 * (el - 16);
          const int slot = (el * 22) / 16;
          return slot < 10 ? FG_W + 6 + slot : slot - 10;
        };
        auto do_tile_f = [&](int tile, dm_h8 (&bh)[NS], dm_h8 (&bl)[NS]) {
          const int ntile = tile + 2 < tot ? tile + 2 : tot - 1;      // the tile that takes over this set (clamped: a re-read, never used)
          int nrow = 0;
          int32_t ncode = 0;
          int64_t noff = 0;
          const dm_h8 *nsrc = nullptr;
          f32x4 s0, s1, s2;
          float t[4], x[4], e[4], pr[4];
          float ma = 0.f, mb = 0.f, mx = 0.f, sum = 0.f, sb = 0.f, xl = 0.f;
          dm_h8 gvv[NT];
          unsigned pu01 = 0u, pu23 = 0u;
          unsigned xt = 0u, xq = 0u;        // FOLD: p_lo of the lane's third position, sent to / received from the lane 32 further
          typedef float f32x2_ __attribute__((ext_vector_type(2)));
          auto gap = [&](auto g_c) {
            constexpr int G = decltype(g_c)::value;
            constexpr int w = G - FG_S;                   // position in the W1a chain
            // ---- epilogue elements (of the previous tile below FG_W + 6 — FOLD: FG_W + 2 —, of this one from there)
#ifndef DMW_DBG_F_NOEPI
            DMW_FOR(4 * NT, el) if constexpr (el_gap(el) == G) epi_elem(el / 4, el % 4); DMW_END
#endif
            if constexpr (w == 48) epi_finish(tile - 1, 0);
            if constexpr (w == 54) epi_finish(tile - 1, 1);
            if constexpr (w == 60) epi_finish(tile - 1, 2);
#ifndef DMW_DBG_F_NOSM
            // ---- softmax of this tile (Mask.scala:17-35, SoftMax.scala:28-42 in the base-2 domain)
            if constexpr (w == 4) { t[0] = s0[0] + s1[0]; t[1] = s0[1] + s1[1]; }
            if constexpr (w == 5) { t[2] = s0[2] + s1[2]; t[3] = s0[3] + s1[3]; }
            if constexpr (w == 7) { t[0] += s2[0]; t[1] += s2[1]; }
            if constexpr (w == 8) { t[2] += s2[2]; t[3] += s2[3]; }
            if constexpr (w == 10) { x[0] = fmaf(t[0], smul[0], sadd[0]); x[1] = fmaf(t[1], smul[1], sadd[1]); }
            if constexpr (w == 11) { x[2] = fmaf(t[2], smul[2], sadd[2]); x[3] = fmaf(t[3], smul[3], sadd[3]); }
            if constexpr (w == 13) { ma = __builtin_fmaxf(x[0], x[1]); mb = __builtin_fmaxf(x[2], x[3]); }
            if constexpr (w == 14) { mx = __builtin_fmaxf(ma, mb); xl = dm_xor16(mx); }
            if constexpr (w == 20) { mx = __builtin_fmaxf(mx, xl); xl = dm_xor32(mx); }
            if constexpr (w == 26) { mx = __builtin_fmaxf(mx, xl); x[0] -= mx; }
            if constexpr (w == 28) { x[1] -= mx; x[2] -= mx; }
            if constexpr (w == 29) { x[3] -= mx; e[0] = __builtin_amdgcn_exp2f(x[0]); }
            if constexpr (w == 31) { e[1] = __builtin_amdgcn_exp2f(x[1]); e[2] = __builtin_amdgcn_exp2f(x[2]); }
            if constexpr (w == 32) e[3] = __builtin_amdgcn_exp2f(x[3]);
            if constexpr (w == 34) { sum = e[0] + e[1]; sb = e[2] + e[3]; }
            if constexpr (w == 35) { sum += sb; xl = dm_xor16(sum); }
            if constexpr (w == 41) { sum += xl; xl = dm_xor32(sum); }
            if constexpr (w == 47) sum += xl;
            if constexpr (w == 49) sum = __builtin_amdgcn_rcpf(sum);
            if constexpr (w == 50) sum *= pscale;
            if constexpr (w == 52) { pr[0] = e[0] * sum; pr[1] = e[1] * sum; }
            if constexpr (w == 53) { pr[2] = e[2] * sum; pr[3] = e[3] * sum; }
            if constexpr (w == 55) {
              pu01 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_){pr[0], pr[1]}, dm_h2));
              pu23 = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_){pr[2], pr[3]}, dm_h2));
            }
            if constexpr (FOLD) {
              // the single operand [ph0 ph1 | ph2+X pl0 | ph0 ph1 | ph2 pl1] (dmw_fold_slot; ph3 = 0 rides in the upper halves of
              // dwords 1 and 3 until the low parts overwrite it).  X = pl2 of the lane 32 further: one exchange of a dword, issued
              // behind its own MFMA and OR-ed in eight gaps later — of ph2 and X one is +0 in every lane
              constexpr int K0 = dmw_fold_slot(0, DMW_LH).k, K1 = dmw_fold_slot(4, DMW_LH).k, K2 = dmw_fold_slot(8, DMW_LH).k;
              static_assert(K0 == 3 && K1 == 7 && K2 == 2 && dmw_fold_slot(8, DMW_LH).grp == 2, "the packing below places p_lo by hand");
              if constexpr (w == 56) { pbu0[0] = pu01; pbu0[2] = pu01; }
              if constexpr (w == 58) { pbu0[K0 >> 1] = pu23; pbu0[K1 >> 1] = pu23; }
              if constexpr (w == 59) {
                asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "+v"(pbu0[K0 >> 1]) : "v"(pu01), "v"(pr[0]));
                asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(pbu0[K1 >> 1]) : "v"(pu01), "v"(pr[1]));
              }
              if constexpr (KQ >= 3) {
                if constexpr (w == 61) asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(xt) : "v"(pu23), "v"(pr[2]));
                if constexpr (w == 62) xq = (unsigned)__shfl_xor((int)xt, 32);
                if constexpr (w == 70) pbu0[K2 >> 1] |= xq & 0xffffu;
              }
            }
            if constexpr (!FOLD && w == 56) { pbu0[0] = pu01; pbu0[1] = pu23; }
            if constexpr (!FOLD && w == 58) { pbu0[2] = pu01; pbu0[3] = pu23; }
            // the low parts p - fp16(p): one mixed-precision fma per element, rounded once like the subtraction it replaces
            if constexpr (!FOLD && w == 59) {
              asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(pbu1[0]) : "v"(pu01), "v"(pr[0]));
              asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(pbu1[1]) : "v"(pu23), "v"(pr[2]));
            }
            if constexpr (!FOLD && w == 61) {
              asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(pbu1[0]) : "v"(pu01), "v"(pr[1]));
              asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(pbu1[1]) : "v"(pu23), "v"(pr[3]));
            }
#endif
            // ---- the row that takes over this operand set, its gathers, the (G + b1) and key fragments
            if constexpr (w == 16) { nrow = ntile * 16 + r; nrow = nrow < ncs ? nrow : ncs - 1; }
            if constexpr (w == 17) ncode = codes[nrow];
#ifdef DMW_DBG_HOTROWS          // timing only: every gather hits a 8 MB window of the table (L2 / Infinity-Cache resident)
            if constexpr (w == 37) noff = (int64_t)(ncode & 16383) * (E / 4);
#else
            if constexpr (w == 37) noff = (int64_t)ncode * (E / 4);
#endif
            if constexpr (w == 38) nsrc = p.emb_split + noff + 2 * g;
#ifndef DMW_DBG_NO_GATHER
            DMW_FOR(NS - 1, s)
              if constexpr (w == (NS + s + 1) * 3 * NB + NB) { dmw_gather16<128 * s>(bh[s], nsrc); dmw_gather16<128 * s + 16>(bl[s], nsrc); }
            DMW_END
            if constexpr (G == FG_W + 1) dmw_gather16<128 * (NS - 1)>(bh[NS - 1], nsrc);
            if constexpr (G == FG_W + 2) dmw_gather16<128 * (NS - 1) + 16>(bl[NS - 1], nsrc);
#endif
#ifndef DMW_DBG_F_NOLD
            DMW_FOR(NT, f) if constexpr (w == 72 + 2 * f) gvv[f] = Gh[f * 64 + lane]; DMW_END
            DMW_FOR(NS, s)
              if constexpr (G == FG_W + 2 * s) kf0[s] = Kh[s * 4 * KCOLS + kfi];
              if constexpr (G == FG_W + 2 * s + 1) kf1[s] = Kh[(NS + s) * 4 * KCOLS + kfi];
            DMW_END
#endif
          };
          DMW_PIN();
          // ---- scores S^T = K Q^T: hi*hi, hi*lo, lo*hi on three accumulation chains
          DMW_FOR(NS, s)
#if !defined(DMW_DBG_NO_GATHER) && !defined(DMW_DBG_NOWAIT)
            dmw_vmwait<2 * (NS - 1 - s) + 2 * NS>();      // k-step s of this set: behind it, the set's later k-steps and the other set's tile
#endif
            DMW_FOR(3, m)
              if constexpr (m == 0) { if constexpr (s == 0) dmw_mfma_vv0(s0, kf0[s], bh[s]); else dmw_mfma_vv(s0, kf0[s], bh[s]); }
              else if constexpr (m == 1) { if constexpr (s == 0) dmw_mfma_vv0(s1, kf0[s], bl[s]); else dmw_mfma_vv(s1, kf0[s], bl[s]); }
              else { if constexpr (s == 0) dmw_mfma_vv0(s2, kf1[s], bh[s]); else dmw_mfma_vv(s2, kf1[s], bh[s]); }
              DMW_PIN(); gap(std::integral_constant<int, 3 * s + m>{}); DMW_PIN();
            DMW_END
          DMW_END
          TMARK(0);
          // ---- W1a chain, accumulator group by accumulator group, A operands from the AccVGPRs
          DMW_FOR(GPS, gg)
            DMW_FOR(NS, s)
              constexpr int nb0 = gg * NB, base = FG_S + (gg * NS + s) * 3 * NB;
              DMW_FOR(NB, i)
                if constexpr (s == 0) dmw_mfma_av0(acc[nb0 + i], wreg[(NS + s) * NT + nb0 + i], bh[s]);
                else dmw_mfma_av(acc[nb0 + i], wreg[(NS + s) * NT + nb0 + i], bh[s]);
                DMW_PIN(); gap(std::integral_constant<int, base + i>{}); DMW_PIN();
              DMW_END
              DMW_FOR(NB, i)
                dmw_mfma_av(acc[nb0 + i], wreg[s * NT + nb0 + i], bl[s]);
                DMW_PIN(); gap(std::integral_constant<int, base + NB + i>{}); DMW_PIN();
              DMW_END
              DMW_FOR(NB, i)
                dmw_mfma_av(acc[nb0 + i], wreg[s * NT + nb0 + i], bh[s]);
                DMW_PIN(); gap(std::integral_constant<int, base + 2 * NB + i>{}); DMW_PIN();
              DMW_END
            DMW_END
            TMARK(1 + gg);
          DMW_END
          // ---- H^T += (G + b1)^T P^T
          if constexpr (FOLD) {
            const dm_h8 pbf = __builtin_bit_cast(dm_h8, pbu0);
            DMW_FOR(GPS, gg)
              DMW_FOR(NB, i)
                dmw_mfma_vv(acc[gg * NB + i], gvv[gg * NB + i], pbf);
                DMW_PIN(); gap(std::integral_constant<int, FG_W + gg * NB + i>{}); DMW_PIN();
              DMW_END
            DMW_END
          } else {
            const dm_h8 pb0 = __builtin_bit_cast(dm_h8, pbu0), pb1 = __builtin_bit_cast(dm_h8, pbu1);
            DMW_FOR(GPS, gg)
              constexpr int nb0 = gg * NB;
              DMW_FOR(2 * NB, ii)
                constexpr int i = ii % NB, half = ii / NB;
                if constexpr (half == 0) dmw_mfma_vv(acc[nb0 + i], gvv[nb0 + i], pb1); else dmw_mfma_vv(acc[nb0 + i], gvv[nb0 + i], pb0);
                DMW_PIN(); gap(std::integral_constant<int, FG_W + gg * 2 * NB + ii>{}); DMW_PIN();
              DMW_END
            DMW_END
          }
          TMARK(1 + GPS);
          TMARK(2 + GPS);
        };
        // pairs of tiles, then the odd one: with the second tile of a pair under a condition the compiler's own load tracking
        // sees a path on which the other set's gathers were never issued, and waits for this set's newest ones instead
        int tile = 0;
        if constexpr (E == 128) {
          for (; tile + 1 < tot; tile += 2) {
            do_tile_f(tile, ah, al);
            do_tile_f(tile + 1, zh, zl);
          }
          if (tile < tot) do_tile_f(tile, ah, al);
        } else {
          for (; tile + 1 < tot; tile += 2) {
            do_tile(tile, ah, al);
            do_tile(tile + 1, zh, zl);
          }
          if (tile < tot) do_tile(tile, ah, al);
        }
        dmw_vmwait<0>();             // the clamped re-reads of the last two tiles: nothing of the loop stays in flight
        my_rows += (unsigned long long)ncs;
        WMARK(4);
        if (tot > 0) {
          // the last tile's epilogue has no next tile to hide under
          DMW_PIN();
          asm volatile("s_nop 7\n\ts_nop 7");          // MFMA results -> VALU readers
          DMW_PIN();
          // (the elements the tile ran behind its own last MFMAs are done: whole pieces, or — hand-placed FOLD tile — the first five)
          constexpr int EL_IN = (E == 128 && FOLD) ? 5 : 4 * EPG;
          static_assert(E != 128 || (el_gap(EL_IN - 1) >= FG_W && el_gap(EL_IN) < FG_W), "elements placed behind the tile's own product");
          DMW_FOR(4 * NT - EL_IN, j) epi_elem((EL_IN + j) / 4, (EL_IN + j) % 4); DMW_END
          epi_finish(tot - 1, 0); epi_finish(tot - 1, 1); epi_finish(tot - 1, 2);
        }
      }
      wsync();
      WMARK(5);
      if (p.trace_counts && it < p.trace_levels) {
        const int64_t tb = (user * p.trace_levels + it);
        if (lane == 0) p.trace_counts[tb] = nchild;
        for (int i = lane; i < nchild; i += 64) { p.trace_codes[tb * CAP + i] = Anext[i]; p.trace_scores[tb * CAP + i] = A_val[i]; }
      }
    }  // levels

    // ================= final selection =================
    if (p.mode == 1) {
      const int32_t *Acur = (const int32_t *)(slotp + (cur ? lo.y_acode1 : lo.y_acode0));
      const int nn = n_cand;
      if (lane == 0) p.out_counts[user] = nn;
      for (int i = lane; i < nn && i < p.out_stride; i += 64) {
        p.out_ids[user * p.out_stride + i] = Acur[i];
        p.out_scores[user * p.out_stride + i] = A_val[i];
      }
      wsync();
      continue;
    }
    // TDM: leaves are in ws in level-block order; the reference's list has the LATEST block first
    // (leafNodes ++: levelInfo.leafNodes, Recommender.scala:65-70), then drops consumed ids (:103-106),
    // then TDM.recommend does a stable sortBy(-pred).take(topk) (TDM.scala:21).
    {
      wsync();
      const int total = leaf_tot < p.ws_cap ? leaf_tot : p.ws_cap;
      const int nblk = n_iter;
      const int64_t c0 = p.consumed_off ? p.consumed_off[user] : 0;
      const int64_t c1 = p.consumed_off ? p.consumed_off[user + 1] : 0;
      int P = 2;
      while (P < total) P <<= 1;
      if (P <= 512 && total <= CAP && P <= p.pcap) {
        // the whole leaf list fits one register sort: ids and scores are staged in LDS by list position (the frontier arrays
        // are free now), so that the output is read back without a second chain of global loads
        int32_t *Sid = (int32_t *)(slotp + lo.y_acode0);
        float *Ssc = A_val;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        int32_t lcode[8], lid[8];
        float lsc[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int i = 8 * ln + e;
          lcode[e] = i < total ? p.ws_code[wsb + i] : 0;
          lsc[e] = i < total ? p.ws_score[wsb + i] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; e++) lid[e] = p.node_id[lcode[e]];
        unsigned long long rkey[8];
        int kept_local = 0;
        int b = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int i = 8 * ln + e;
          unsigned long long key = DMW_KEY_PAD;
          if (i < total) {
            bool drop = false;
            for (int64_t q = c0; q < c1; q++) drop |= (p.consumed_ids[q] == lid[e]);
            while (b + 1 < nblk && i >= misc[M_LVOFF + b + 1]) b++;          // blocks are in list order: b only grows with e
            const int pos = (total - misc[M_LVOFF + b + 1]) + (i - misc[M_LVOFF + b]);
            Sid[pos] = lid[e]; Ssc[pos] = lsc[e];
            if (!drop) { key = dmw_make_key(lsc[e], (unsigned)pos); kept_local++; }
          }
          rkey[e] = key;
        }
        int kept = kept_local;
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
        reg_sort8(rkey, P);
        store_keys8(rkey, ln);
        wsync();
        const int nout = kept < p.topk ? kept : p.topk;
        for (int rk = ln; rk < nout; rk += 64) {
          const int pos = (int)DMW_KEY_POS(keys[rk]);
          p.out_ids[user * p.out_stride + rk] = Sid[pos];
          p.out_scores[user * p.out_stride + rk] = Ssc[pos];
        }
        if (lane == 0) p.out_counts[user] = nout;
      } else if (P <= p.pcap) {
        int kept_local = 0;
        for (int i = lane; i < P; i += 64) {
          unsigned long long key = DMW_KEY_PAD;
          if (i < total) {
            const int32_t code = p.ws_code[wsb + i];
            const float sc = p.ws_score[wsb + i];
            const int32_t id = p.node_id[code];
            bool drop = false;
            for (int64_t q = c0; q < c1; q++) drop |= (p.consumed_ids[q] == id);
            int b = 0;
            while (b + 1 < nblk && i >= misc[M_LVOFF + b + 1]) b++;
            const int pos = (total - misc[M_LVOFF + b + 1]) + (i - misc[M_LVOFF + b]);
            if (!drop) { key = dmw_make_key(sc, (unsigned)pos); kept_local++; }
          }
          keys[i] = key;
        }
        int kept = kept_local;
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
        lds_sort(P);
        wsync();
        const int nout = kept < p.topk ? kept : p.topk;
        for (int rk = lane; rk < nout; rk += 64) {
          const int pos = (int)DMW_KEY_POS(keys[rk]);
          int b = 0;
          while (b + 1 < nblk && pos < total - misc[M_LVOFF + b + 1]) b++;
          const int i = misc[M_LVOFF + b] + (pos - (total - misc[M_LVOFF + b + 1]));
          p.out_ids[user * p.out_stride + rk] = p.node_id[p.ws_code[wsb + i]];
          p.out_scores[user * p.out_stride + rk] = p.ws_score[wsb + i];
        }
        if (lane == 0) p.out_counts[user] = nout;
      } else {
        // leaf list outgrew the LDS key area (trees with leaves on many levels): exact O(n^2) ranking
        uint32_t *khi = p.ws_khi + wsb, *klo = p.ws_klo + wsb;
        int kept_local = 0;
        for (int i = lane; i < total; i += 64) {
          const int32_t code = p.ws_code[wsb + i];
          const int32_t id = p.node_id[code];
          bool drop = false;
          for (int64_t q = c0; q < c1; q++) drop |= (p.consumed_ids[q] == id);
          int b = 0;
          while (b + 1 < nblk && i >= misc[M_LVOFF + b + 1]) b++;
          const int pos = (total - misc[M_LVOFF + b + 1]) + (i - misc[M_LVOFF + b]);
          khi[i] = dm_desc_key(p.ws_score[wsb + i]);
          klo[i] = drop ? 0xFFFFFFFFu : (uint32_t)pos;
          kept_local += drop ? 0 : 1;
        }
        int kept = kept_local;
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int i = lane; i < total; i += 64) {
          const uint32_t hi = khi[i], lp = klo[i];
          if (lp == 0xFFFFFFFFu) continue;
          int rank = 0;
          for (int j = 0; j < total; j++) {
            const uint32_t hj = khi[j], lj = klo[j];
            rank += (lj != 0xFFFFFFFFu) && ((hj < hi) || (hj == hi && lj < lp));
          }
          if (rank < p.topk) {
            p.out_ids[user * p.out_stride + rank] = p.node_id[p.ws_code[wsb + i]];
            p.out_scores[user * p.out_stride + rank] = p.ws_score[wsb + i];
          }
        }
        if (lane == 0) p.out_counts[user] = kept < p.topk ? kept : p.topk;
      }
    }
    wsync();
  }  // users
  if (lane == 0 && my_rows) atomicAdd(p.scored_rows, my_rows);
#ifdef DM_PHASE_TIMERS
  WMARK(6);
  if (lane == 0 && p.phase_cycles) for (int k = 0; k < 8; k++) atomicAdd(p.phase_cycles + k, tph[k]);
#endif
#ifdef DM_TILE_TIMERS
  if (lane == 0 && p.phase_cycles) for (int k = 0; k < 8; k++) atomicAdd(p.phase_cycles + 8 + k, ttile[k]);
#endif
#ifdef DM_SETUP_TIMERS
  if (lane == 0 && p.phase_cycles) for (int k = 0; k < 8; k++) atomicAdd(p.phase_cycles + 8 + k, tsu[k]);
#endif
}
