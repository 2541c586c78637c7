// Persistent beam-search kernel (TDM and OTM variants) for gfx950.
//
// Replaces the level fold of Recommender._recommend (tdm/src/main/scala/com/mass/tdm/
// model/Recommender.scala:40-107) and CandidateSearcher.beamSearch (otm/src/main/scala/
// com/mass/otm/model/CandidateSearcher.scala:58-80) together with the DIN forward they
// call once per level (tdm/.../model/DIN.scala:18-42).
//
// Design (DESIGN.md §3):
//   * one 512-thread workgroup (8 waves, 2 per SIMD) per CU, split into independent TEAMS of
//     TW waves (normally 4 teams x 2 waves).  A team pulls one user at a time from a global
//     queue and walks it through all tree levels with the frontier in its LDS slot.  Teams
//     never meet at a workgroup barrier, so the prune/expand phases of one team run under
//     the MFMA phases of the others (two waves of different teams share every SIMD).
//   * the scorer is restructured around the fact that the history is per USER, not per
//     candidate row (the reference replicates it 2*beam times):
//        logit = w2 . relu( W1a q + sum_j p_j G_j + b1 ) + b2,
//        p     = softmax_j( q.k_j / sqrt(E), pads -> -FLT_MAX ),
//        G_j   = W1b (W_att k_j)           -- once per user, L rows
//     which is algebraically the reference's  W1 [q ; W_att sum_j p_j k_j] + b1.
//   * per 16-row tile one wave runs the three products TRANSPOSED (weights / keys / G as the MFMA A operand, the
//     gathered rows / softmax weights as B):  S^T = K Q^T,  the softmax in the C layout (4 positions per lane + two
//     LDS-crossbar exchanges),  H^T = W1a Q^T + (G + b1)^T P^T  into E/16 accumulators, and the ReLU / w2 epilogue.
//     SPLIT = false: v_mfma_f32_16x16x4_f32 throughout.  SPLIT = true (default for E >= 32): every fp32 operand as
//     fp16 hi + lo, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation (DESIGN.md §3).
//   * gathered embedding rows go HBM -> VGPR directly in fragment layout, one tile ahead (each row is consumed by
//     exactly one wave); W1a, the user's keys and G are read from LDS in fragment order (conflict-free ds_read_b128).
//   * prune = exact stable top-b: bitonic sort of 64-bit keys (descending Float.compareTo key,
//     input position) in LDS == a stable TimSort with comparator y.pred.compareTo(x.pred)
//     (Recommender.scala:77-84), because the keys are unique.

// Timing knock-outs (DM_DBG_* / DMW_DBG_*: builds that drop a stage and produce WRONG results, used to attribute kernel time)
// and the in-kernel cycle counters (DM_*_TIMERS) exist only in probe builds: tools/ compiles its own copy of the library with
// -DDM_PROBE_BUILD plus the switch it needs.  The product build (dismember_amd/_native.py) never defines DM_PROBE_BUILD, and
// any of these switches without it is a build error — a knock-out cannot reach a shipped library by accident.
#if !defined(DM_PROBE_BUILD) &&                                                                                            \
    (defined(DM_DBG_NO_S) || defined(DM_DBG_NO_GATHER) || defined(DM_DBG_NO_EPI) || defined(DM_DBG_NO_XLANE) ||             \
     defined(DM_SPLIT_NO_MIX) || defined(DMW_DBG_F_NOEPI) || defined(DMW_DBG_F_NOLD) || defined(DMW_DBG_F_NOSM) ||          \
     defined(DMW_DBG_HOTROWS) || defined(DMW_DBG_NOWAIT) || defined(DMW_DBG_NO_GATHER) || defined(DMW_DBG_NO_GVV) ||        \
     defined(DMW_DBG_SM_UPTO) || defined(DM_PHASE_TIMERS) || defined(DM_TILE_TIMERS) || defined(DM_SETUP_TIMERS))
#error "timing knock-outs and in-kernel timers need -DDM_PROBE_BUILD (probe builds only: they change results)"
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 dm_h8 __attribute__((ext_vector_type(8)));   // A / B operand of v_mfma_f32_16x16x32_f16
typedef _Float16 dm_h2 __attribute__((ext_vector_type(2)));

#define DM_BLOCK 512
#define DM_NWAVES 8
#define DM_MAXL 16
#define DM_PIPE_MAXL 32        // history positions of the per-level pipelines (otm64.hip.inc, tdm_pipeline.hip.inc): 17 .. 32 take those
// Per-level existence bounds of a loaded tree (dm_level_bounds_bits): entry l is the largest existing code of level l when the
// level's existing codes are exactly [2^l - 1, last] ("exists" is then code <= last), 2^l - 2 for an empty level, and
// DM_LEVEL_USE_BITS for a level with a gap — only the bitmap answers there
#define DM_N_LEVEL_BOUNDS 32
#define DM_LEVEL_USE_BITS (-2)

struct BeamParams {
  // weights
  const float *emb;          // [num_index][E]
  const f32x4 *wfrag;        // W1a^T in B-fragment order [NJ][NT][64] float4
  const f32x4 *afrag;        // att_w   as B fragments [NJ][NT][64] float4 (T1 = K att_w^T)
  const f32x4 *bfrag;        // W1b     as B fragments [NJ][NT][64] float4 (G = T1 W1b^T)
  const float *b1, *w2;      // [E]
  float b2;
  // split scorer (DESIGN.md "split-fp16 scorer"): W1a * 2^sh_w as two fp16 planes (hi, lo) in the A-fragment order of
  // v_mfma_f32_16x16x32_f16, [plane][E/32 k-steps][NT][64 lanes] x 8 halfs; rows are scaled by emb_scale = 2^sh_e
  const dm_h8 *wsplit;
  const dm_h8 *emb_split;    // the table pre-split for the one-wave-per-SIMD kernel: [row][E/32 k-steps][4 g][hi 8 | lo 8] halfs, row stride E*4 bytes
  float emb_scale, score_unscale, acc_scale, out_unscale;   // 2^sh_e, 2^(-2 sh_e), 2^(sh_e+sh_w), 2^-(sh_e+sh_w)
  const float *g_table;      // [num_index][E]: row c = W1b (att.W emb[c]), what the W kernel's per-user setup computes for a history position
                             //    holding code c (dm_build_g_table_kernel); null: the setup runs the two products itself
  int64_t num_index;
  // tree
  const uint32_t *exists_bits, *leaf_bits;
  const int32_t *node_id, *id_to_code;
  const int32_t *level_last; // [DM_N_LEVEL_BOUNDS] per-level existence bounds (dm_level_bounds_bits), read by the one-wave-per-SIMD kernel;
                             //    null (DM_LEVEL_BOUNDS=0, or no tree): every existence test reads exists_bits
  int64_t n_slots;
  int32_t non_leaf_offset, max_code, max_level;
  int leaf_fast;             // 1: every leaf sits at max_level and nothing else does (TreeBuilder.flattenLeaves)
  // request
  const int32_t *seq;        // [U][L] item ids (TDM) or node codes (OTM)
  int64_t U;
  int L, use_mask, beam, topk, widen;
  const int64_t *consumed_off;
  const int32_t *consumed_ids;
  int mode;                  // 0 TDM, 1 OTM (complete tree, always sort, no leaf handling),
                             // 2 brute force: score every leaf of a slice, keep the best topk (build-defined
                             //   recall oracle, SURVEY.md §8d; order = score desc, then leaf code asc)
  const int32_t *bf_leaf_codes;   // all leaf codes, ascending
  int64_t bf_n_leaf;
  int bf_slices, bf_chunk;        // work item = (user, slice); rows scored per iteration
  int64_t bf_per_slice;
  unsigned long long *bf_out_keys;   // [U * slices][topk] sorted keys (desc score key << 32 | code)
  int otm_leaf_level;
  int nteams, cap, pcap;     // teams per workgroup, candidate capacity (multiple of 16), pow2 >= cap
  // outputs
  int32_t *out_ids;
  float *out_scores;
  int32_t *out_counts;
  int out_stride;            // topk (TDM) or 2*beam (OTM)
  // workspace: per (block, team) leaf list
  int32_t *ws_code;
  float *ws_score;
  uint32_t *ws_khi, *ws_klo;  // key scratch for leaf lists that outgrow LDS
  int ws_cap;
  unsigned long long *next_user;   // work queue head (zeroed before every launch)
  // trace (optional)
  int32_t *trace_codes;
  float *trace_scores;
  int32_t *trace_counts;
  int trace_levels;
  unsigned long long *scored_rows;
  unsigned long long *phase_cycles;   // [8] debug accumulators (DM_PHASE_TIMERS builds)
  // hand-over from the one-wave-per-SIMD kernel (beam_kernel_w.hip.inc): users it defers are appended to defer_users; the
  // LDS-fed kernel, launched right after it, then works through user_list[0 .. *user_count) instead of 0 .. U
  unsigned long long *defer_count;
  int32_t *defer_users;
  const unsigned long long *user_count;
  const int32_t *user_list;
  float sm_scale;            // 1 / sqrt(embedSize) of the MODEL (Mask.scala:10): smaller than 1 / sqrt(E) when the table is zero-padded to E
  int static_users;          // 1: team t of block b takes user b * nteams + t and exits (no work queue; U <= grid * nteams)
  int host_direct;           // 1: seq / out_* are host-mapped pinned memory of a single-request call: the kernel fills every
                             //    output slot, fences at system scope and stores out_counts[user] LAST — the flag the host polls
};

__device__ __forceinline__ uint32_t dm_desc_key(float s) {
  uint32_t b = __float_as_uint(s);
  if (s != s) b = 0x7fc00000u;                         // floatToIntBits: one canonical NaN, greatest
  uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // -0.0 < +0.0
  return ~asc;                                          // ascending key order == descending score
}

template <int CTRL>
__device__ __forceinline__ float dm_dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
// all-reduce over the 16 lanes of a DPP row; every lane ends with the bitwise-same value
// cross-row exchanges on the LDS crossbar (ds_swizzle / ds_bpermute): they do not take VALU issue slots
#ifdef DM_DBG_NO_XLANE   // timing experiments only (wrong results)
__device__ __forceinline__ float dm_xor16(float x) { return x; }
__device__ __forceinline__ float dm_xor32(float x) { return x; }
#else
__device__ __forceinline__ float dm_xor16(float x) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x1F | (16 << 10)));
}
__device__ __forceinline__ float dm_xor32(float x) { return __shfl_xor(x, 32); }
#endif
__device__ __forceinline__ float dm_sum16(float x) {
  x += dm_dpp<0xB1>(x);   // quad_perm [1,0,3,2]
  x += dm_dpp<0x4E>(x);   // quad_perm [2,3,0,1]
  x += dm_dpp<0x141>(x);  // row_half_mirror
  x += dm_dpp<0x140>(x);  // row_mirror
  return x;
}
__device__ __forceinline__ float dm_max16(float x) {
  x = fmaxf(x, dm_dpp<0xB1>(x));
  x = fmaxf(x, dm_dpp<0x4E>(x));
  x = fmaxf(x, dm_dpp<0x141>(x));
  x = fmaxf(x, dm_dpp<0x140>(x));
  return x;
}

__device__ __forceinline__ bool dm_bit(const uint32_t *bits, int64_t i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// value held by lane ^ m (m a power of two <= 32): DPP for 1/2, ds_swizzle bit-mode for 4/8/16, bpermute for 32
__device__ __forceinline__ uint32_t dm_xor_lane(uint32_t v, int m) {
  switch (m) {
    case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
    case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
    case 4: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (4 << 10));
    case 8: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (8 << 10));
    case 16: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (16 << 10));
    default: return (uint32_t)__shfl_xor((int)v, 32);
  }
}

// the same exchange entirely on the VALU (no LDS-crossbar round trip of ~100 cycles on a latency chain): DPP row rotations for 4 and
// 8, gfx950's v_permlane16_swap / v_permlane32_swap for 16 and 32 (checked lane by lane on MI355X: tools/lane_xor_probe.hip)
__device__ __forceinline__ uint32_t dm_xor_lane_valu(uint32_t v, int m, int lane) {
  switch (m) {
    case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
    case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
    case 4: {
      const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, true);   // row_ror:4  -> lane - 4 (mod 16)
      const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x12C, 0xF, 0xF, true);   // row_ror:12 -> lane + 4 (mod 16)
      return (lane & 4) ? a : b;
    }
    case 8: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true);          // row_ror:8
    case 16: { const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); return (lane & 16) ? r[0] : r[1]; }
    default: { const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); return (lane & 32) ? r[0] : r[1]; }
  }
}

// One bitonic compare-exchange stage on 4 consecutive keys per lane (element index base+e), stride J
// known at compile time so the partner exchange is straight-line code; k (the phase) only feeds the
// sort direction.  J = 1, 2: in-lane; J = 4..128: partner lane = lane ^ (J/4).
template <int J>
__device__ __forceinline__ void dm_sort_stage(unsigned long long (&key)[4], int lane, int base, int k) {
  if (J == 1) {
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const bool asc = ((base + e) & k) == 0;
      const unsigned long long a = key[e], b = key[e + 1];
      const bool sw = (a < b) != asc;
      key[e] = sw ? b : a; key[e + 1] = sw ? a : b;
    }
  } else if (J == 2) {
    const bool asc = (base & k) == 0;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const unsigned long long a = key[e], b = key[e + 2];
      const bool sw = (a < b) != asc;
      key[e] = sw ? b : a; key[e + 2] = sw ? a : b;
    }
  } else {
    constexpr int M = J / 4;
    const bool keepmin = ((lane & M) == 0) == ((base & k) == 0);
    uint32_t olo[4], ohi[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      olo[e] = dm_xor_lane((uint32_t)key[e], M);
      ohi[e] = dm_xor_lane((uint32_t)(key[e] >> 32), M);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const unsigned long long o = ((unsigned long long)ohi[e] << 32) | olo[e];
      key[e] = ((key[e] < o) == keepmin) ? key[e] : o;
    }
  }
}

// LDS carve-up (bytes), shared by host (size) and device (offsets)
struct BeamLds {
  int wfrag, b1, w2, slot0, slot_stride;
  int x_kfrag, x_gfrag;            // region X: K^T / G fragments of the current user
  int y_keys, y_acode0, y_acode1, y_aval;   // region Y: T1 scratch during setup, then the frontier
  int misc, sync, total;
};
// kt = 2: histories of 17 .. 32 positions — two 16-position key tiles (K^T fragments, G planes and the misc words twice)
__host__ __device__ inline BeamLds dm_beam_lds(int E, int nteams, int cap, int pcap, int kq, bool split = false, int kt = 1) {
  const int kcols = (kq >= 4 || kt > 1) ? 16 : 12;   // history columns kept in the K^T fragments (per key tile)
  BeamLds l;
  int o = 0;
  l.wfrag = o; o += E * E * 4;
  l.b1 = o; o += E * 4;
  l.w2 = o; o += E * 4;
  l.slot0 = o;
  int s = 0;
  // X: K^T fragments [NJ][4 g][kcols n] float4 + G planes [kq][NT][64] float
  l.x_kfrag = s; s += kt * (E / 16) * 4 * kcols * 16;
  // (G + b1)^T A fragments, one fp32 plane per k-step (4 positions each); split scorer: fp16 hi / lo, 16 B per lane and tile
  l.x_gfrag = s; s += (split || kt > 1) ? kt * (E / 16) * 64 * 16 : kq * (E / 16) * 64 * 4;
  const int ybase = s;
  l.y_keys = s; s += pcap * 8;
  l.y_acode0 = s; s += cap * 4;
  l.y_acode1 = s; s += cap * 4;
  l.y_aval = s; s += cap * 4;
  if (s - ybase < 16 * (E + 4) * 4) s = ybase + 16 * (E + 4) * 4;   // T1 scratch during setup
  s = (s + 15) & ~15;
  l.misc = s; s += (kt > 1 ? 96 : 64) * 4;
  l.slot_stride = s;
  o += s * nteams;
  o = (o + 15) & ~15;
  l.sync = o; o += 64 * 4;
  l.total = (o + 15) & ~15;
  return l;
}

// misc[] slots
enum { M_NCAND = 0, M_USER = 1, M_LEAFTOT = 2, M_PADMASK = 3, M_BEAM = 4, M_START = 5, M_NITER = 6, M_KEPT = 7,
       M_SEQ = 8 /* +DM_MAXL */, M_LVOFF = 24 /* +36 */, M_NPOOL = 60, M_WORK = 61,
       M_GMAX = 62 /* split scorer: bits of max |G + b1| of the user */, M_GSP = 63 /* exponent of the scale on p, DM_G32 = fp32 P x G */,
       M_SEQ_HI = 64 /* +16: history positions 16 .. 31 (two-key-tile instances only) */, M_PADMASK_HI = 80 };
#define DM_G32 1000

// x (already scaled into the fp16 range) = hi + lo + O(2^-22 |x|): hi = RNE16(x), lo = RNE16(x - hi) (the residual is exact
// in fp32).  8 values -> two MFMA operands.
__device__ __forceinline__ void dm_split8(const f32x4 &u, const f32x4 &v, float s, dm_h8 &hi, dm_h8 &lo) {
#ifndef DM_SPLIT_NO_MIX
  // two mixed-precision FMAs per value: hi = f16(x * s), lo = f16(x * s - hi) (v_fma_mix{lo,hi}_f16 take fp32 and fp16
  // sources side by side and write one half of the destination; the fp32 intermediate x * s - hi is exact)
  typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
  unsigned h0, h1, h2, h3, l0, l1, l2, l3;
  // ONE asm block: the assembler text is opaque to the compiler's hazard recogniser, and on gfx950 an instruction that writes
  // half a register (dst_sel) must not be followed at once by a reader of that register.  Inside the block every dependent
  // pair is four instructions apart; the trailing s_nop (4 wait states) covers the first consumer after it.
  asm("v_fma_mixlo_f16 %0, %8, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixlo_f16 %1, %10, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixlo_f16 %2, %12, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixlo_f16 %3, %14, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %9, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixhi_f16 %1, %11, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixhi_f16 %2, %13, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixhi_f16 %3, %15, %16, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixlo_f16 %4, %8, %16, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixlo_f16 %5, %10, %16, -%1 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixlo_f16 %6, %12, %16, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixlo_f16 %7, %14, %16, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %4, %9, %16, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %5, %11, %16, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %6, %13, %16, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %7, %15, %16, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
      "s_nop 3"
      : "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
      : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]), "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(s));
  const u32x4_ h = {h0, h1, h2, h3}, l = {l0, l1, l2, l3};
  hi = __builtin_bit_cast(dm_h8, h); lo = __builtin_bit_cast(dm_h8, l);
#else
  typedef float f32x2_ __attribute__((ext_vector_type(2)));
  const float x[8] = {u[0] * s, u[1] * s, u[2] * s, u[3] * s, v[0] * s, v[1] * s, v[2] * s, v[3] * s};
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const dm_h2 a = __builtin_convertvector((f32x2_){x[i], x[i + 1]}, dm_h2);        // v_cvt_pk_f16_f32 (RNE)
    hi[i] = a[0]; hi[i + 1] = a[1];
    const dm_h2 b = __builtin_convertvector((f32x2_){x[i] - (float)a[0], x[i + 1] - (float)a[1]}, dm_h2);
    lo[i] = b[0]; lo[i + 1] = b[1];
  }
#endif
}

// KQ = ceil(L / 4): k-steps of the P x G product.  SPLIT: the three products of the tile (scores, the W1a half and the
// attention half of linear1) run on the fp16 matrix pipe with every fp32 operand split into hi + lo halves (3 MFMAs per
// product: hi*hi + hi*lo + lo*hi, fp32 accumulation) instead of the fp32-input MFMA, which on gfx950 runs at the vector rate.
// KT = 2 (with KQ = 4): histories of 17 .. 32 positions.  The reference's Attention takes any sequence length
// (scalann/src/main/scala/com/mass/scalann/nn/Attention.scala:34-53); here a second 16-position key tile rides through the same tile
// code: twice the score MFMAs, a softmax over 8 positions per lane, twice the attention-combine MFMAs — the W1a chain (three
// quarters of the tile) is unchanged.
template <int E, int KQ, bool SPLIT, int KT = 1>
__global__ __launch_bounds__(DM_BLOCK, 2) void dm_beam_kernel(BeamParams p) {
  static_assert(KT == 1 || (KT == 2 && KQ == 4), "two key tiles come with full k-step counts");
  constexpr int NJ = E / 16, NT = E / 16;
  constexpr int NS = SPLIT ? E / 32 : 1;   // k-steps of the fp16 products
  static_assert(!SPLIT || E % 32 == 0, "the split scorer needs an embedding size that is a multiple of 32");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const BeamLds lo = dm_beam_lds(E, p.nteams, p.cap, p.pcap, KQ, SPLIT, KT);
  constexpr int KCOLS = KQ >= 4 ? 16 : 12;
  constexpr int KBLK = NJ * 4 * KCOLS;       // 16-byte entries of one key tile's K^T fragments
  constexpr int KQT = KT * KQ;               // k-steps (of 4 positions) of the fp32 P x G product
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CAP = p.cap, L = p.L;
  const int TW = DM_NWAVES / p.nteams;   // waves per team
  const int TT = TW * 64;                // threads per team
  const int team = wave / TW, tw = wave % TW;
  const int tt = tid - team * TT;

  f32x4 *Wfrag = (f32x4 *)(smem + lo.wfrag);
  float *B1 = (float *)(smem + lo.b1), *W2 = (float *)(smem + lo.w2);
  char *slotp = smem + lo.slot0 + team * lo.slot_stride;
  int *syncw = (int *)(smem + lo.sync);          // [0..7] team barrier counters, [8..] scan scratch
  unsigned long long *keys = (unsigned long long *)(slotp + lo.y_keys);
  float *A_val = (float *)(slotp + lo.y_aval);
  int *misc = (int *)(slotp + lo.misc);
  const f32x4 *Kf = (const f32x4 *)(slotp + lo.x_kfrag);
  const float *Gf = (const float *)(slotp + lo.x_gfrag);

  // ---- once per workgroup: stage W1a^T fragments, b1, w2 ----
  // (split mode: the same E*E*4 bytes hold the two fp16 planes, and w2 carries the inverse of the accumulator scale)
  if (SPLIT) { for (int i = tid; i < NJ * NT * 64; i += DM_BLOCK) Wfrag[i] = ((const f32x4 *)p.wsplit)[i]; }
  else { for (int i = tid; i < NJ * NT * 64; i += DM_BLOCK) Wfrag[i] = p.wfrag[i]; }
  for (int i = tid; i < E; i += DM_BLOCK) { B1[i] = p.b1[i]; W2[i] = SPLIT ? p.w2[i] * p.out_unscale : p.w2[i]; }
  const dm_h8 *Wh = (const dm_h8 *)(smem + lo.wfrag);
  const dm_h8 *Kh = (const dm_h8 *)(slotp + lo.x_kfrag);
  (void)Wh; (void)Kh;
  if (tid < 64) syncw[tid] = 0;
  __syncthreads();   // the only workgroup-wide barrier in the kernel
  const float scale = p.sm_scale;   // Mask.scala:10
  const float scale2 = (float)(1.4426950408889634 * (double)p.sm_scale) * (SPLIT ? p.score_unscale : 1.0f);   // the same in the base-2 domain of v_exp_f32
  (void)scale;
  unsigned long long my_rows = 0;
#ifdef DM_TILE_TIMERS
  unsigned long long ttile[5] = {0, 0, 0, 0, 0};
#endif
#ifdef DM_PHASE_TIMERS
  unsigned long long tph[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tlast = clock64();
#define PHASE_MARK(k) do { unsigned long long tn_ = clock64(); tph[k] += tn_ - tlast; tlast = tn_; } while (0)
#else
#define PHASE_MARK(k) do {} while (0)
#endif

  // ---- team barrier: monotonic LDS counter, one arrival per wave ----
  int bar_target = 0;
  int *bar_cnt = syncw + team;
  auto team_barrier = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (TW > 1) {
      bar_target += TW;
      if (lane == 0) {
        __hip_atomic_fetch_add(bar_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(bar_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - bar_target < 0)
          __builtin_amdgcn_s_sleep(1);
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  // order LDS traffic inside ONE wave (DS ops of a wave execute in order; this only stops the compiler)
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };

  // ---- ordered team-wide scan over elements laid out thread-major, 4 per thread ----
  // bits4: flags of elements 4*tt+j.  Returns #set flags before this thread's first element; total via ref.
  int scan_phase = 0;
  auto team_scan4 = [&](unsigned bits4, int &total) -> int {
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int before = 0, wtot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      unsigned long long m = __ballot((bits4 >> j) & 1u);
      before += __popcll(m & below);
      wtot += __popcll(m);
    }
    if (TW == 1) { total = wtot; return before; }
    int *w = syncw + 8 + scan_phase * DM_NWAVES;
    if (lane == 0) w[wave] = wtot;
    team_barrier();
    int off = 0; total = 0;
    for (int k = 0; k < TW; k++) {
      int c = w[team * TW + k];
      if (k < tw) off += c;
      total += c;
    }
    scan_phase ^= 1;
    return off + before;
  };

  // ---- bitonic sort of keys[0..P) ascending, P a power of two >= 2*TW ----
  auto bitonic_sort = [&](int P) {
    const int chunk = P / TW;                      // elements owned by one wave
    const int per_wave = (P >> 1) / TW;            // compare-exchanges per wave and stage
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        const bool cross = (2 * j > chunk);
        if (cross) team_barrier(); else wave_sync();
        for (int c = tw * per_wave + lane; c < (tw + 1) * per_wave; c += 64) {
          const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
          const int l2 = i + j;
          const unsigned long long a = keys[i], b = keys[l2];
          const bool asc = (i & k) == 0;
          const unsigned long long mn = a < b ? a : b, mx = a < b ? b : a;
          keys[i] = asc ? mn : mx;
          keys[l2] = asc ? mx : mn;
        }
        if (cross) team_barrier();
      }
    }
    wave_sync();
  };

  // ---- in-register bitonic sort: every wave keeps 256 keys, 4 CONSECUTIVE per lane (element
  //      x = 4*lane + e of its chunk [256*tw, 256*tw+256)): strides 1,2 are in-lane, 4..128 are lane
  //      xors (DPP / ds_swizzle / one bpermute), >= 256 go through LDS once.  Sorts indices [0, Pn)
  //      ascending, Pn a power of two <= 256*TW.  Keys are unique, so the result is the stable order.
  auto reg_sort = [&](unsigned long long (&key)[4], int Pn) {
    const int base = tw * 256 + 4 * lane;
    for (int k = 2; k <= Pn; k <<= 1) {
      // strides >= 256 cross waves: one LDS exchange each (only phases k >= 512)
      for (int j = k >> 1; j >= 256; j >>= 1) {
        // waves whose chunk lies beyond Pn hold padding only: they keep the barriers but stay out of the exchange
        // (the key region has room for the sorted range, not for 256 * TW slots)
        const bool in = base < Pn;
        if (in) {
          *(ulonglong2 *)(keys + base) = make_ulonglong2(key[0], key[1]);
          *(ulonglong2 *)(keys + base + 2) = make_ulonglong2(key[2], key[3]);
        }
        team_barrier();
        if (in) {
          const ulonglong2 o01 = *(const ulonglong2 *)(keys + (base ^ j));
          const ulonglong2 o23 = *(const ulonglong2 *)(keys + (base ^ j) + 2);
          const unsigned long long o[4] = {o01.x, o01.y, o23.x, o23.y};
          const bool keepmin = ((base & j) == 0) == ((base & k) == 0);
#pragma unroll
          for (int e = 0; e < 4; e++) key[e] = ((key[e] < o[e]) == keepmin) ? key[e] : o[e];
        }
        team_barrier();
      }
      if (k >= 256) dm_sort_stage<128>(key, lane, base, k);
      if (k >= 128) dm_sort_stage<64>(key, lane, base, k);
      if (k >= 64) dm_sort_stage<32>(key, lane, base, k);
      if (k >= 32) dm_sort_stage<16>(key, lane, base, k);
      if (k >= 16) dm_sort_stage<8>(key, lane, base, k);
      if (k >= 8) dm_sort_stage<4>(key, lane, base, k);
      if (k >= 4) dm_sort_stage<2>(key, lane, base, k);
      dm_sort_stage<1>(key, lane, base, k);
    }
  };

  // one-wave teams, at most 64 keys (the reference's serving default: candidateNum 20 -> 40 candidates per level): ONE key per
  // lane, 21 compare-exchange stages of a lane-xor each — a few hundred cycles where the 256-key register sort takes 4 000
  auto sort64 = [&](unsigned long long key) -> unsigned long long {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const unsigned long long o = ((unsigned long long)dm_xor_lane_valu((uint32_t)(key >> 32), j, lane) << 32) | dm_xor_lane_valu((uint32_t)key, j, lane);
        const bool keepmin = ((lane & j) == 0) == ((lane & k) == 0);
        key = ((key < o) == keepmin) ? key : o;
      }
    }
    return key;
  };

  const int64_t wsb = ((int64_t)blockIdx.x * p.nteams + team) * p.ws_cap;
  bool static_done = false;       // static_users: one user per team, no queue (requests smaller than the grid: the single-request path)

  __builtin_amdgcn_s_setprio(3);
  for (;;) {
    // ================= next user from the global queue =================
    PHASE_MARK(4);
    if (p.static_users) {
      if (static_done) break;
      static_done = true;
    }
    if (tt == 0) {
      unsigned long long u = p.static_users ? (unsigned long long)blockIdx.x * p.nteams + team : atomicAdd(p.next_user, 1ull);
      const unsigned long long n_work = (p.mode == 2) ? (unsigned long long)p.U * p.bf_slices
                                                       : (p.user_list ? *p.user_count : (unsigned long long)p.U);
      misc[M_WORK] = (u < n_work) ? (int)u : -1;
      misc[M_USER] = (u < n_work) ? (int)((p.mode == 2) ? u / p.bf_slices : (p.user_list ? (unsigned long long)p.user_list[u] : u)) : -1;
    }
    team_barrier();
    const int64_t user = misc[M_USER];
    const int64_t work = misc[M_WORK];
    if (user < 0) break;
    PHASE_MARK(5);

    // ================= per-user setup =================
    // (1) beam, start level, history codes, pad mask
    if (tt == 0) {
      int beam = p.beam;
      if (p.widen && p.consumed_off) {   // Recommender.recommendItems, Recommender.scala:28-33
        int nc = (int)(p.consumed_off[user + 1] - p.consumed_off[user]);
        int w = (nc + p.topk) / 2;
        beam = w > beam ? w : beam;
        if (2 * beam > CAP) beam = CAP / 2;      // host sizes CAP so that this never triggers
      }
      int level = 31 - __clz(beam);               // floor(log2(beam)); getLevelStart, :210-216
      int start = (1 << level) - 1;
      int n_iter;
      if (p.mode == 0) n_iter = p.max_level - level + 1;   // (level to tree.maxLevel)
      else if (p.mode == 1) n_iter = p.otm_leaf_level - level;   // (startLevel until leafLevel)
      else {
        const int64_t lo_ = (work % p.bf_slices) * p.bf_per_slice;
        int64_t len = p.bf_n_leaf - lo_;
        if (len > p.bf_per_slice) len = p.bf_per_slice;
        if (len < 0) len = 0;
        n_iter = (int)((len + p.bf_chunk - 1) / p.bf_chunk);
      }
      if (n_iter < 0) n_iter = 0;
      if (n_iter > 34 && p.mode != 2) n_iter = 34;
      misc[M_BEAM] = beam; misc[M_START] = start; misc[M_NITER] = n_iter; misc[M_LEAFTOT] = 0;
      misc[M_NCAND] = 0; misc[M_LVOFF] = 0; misc[M_KEPT] = 0; misc[M_NPOOL] = 0; misc[M_GMAX] = 0; misc[M_GSP] = DM_G32;
      if (p.mode == 2) { misc[M_LVOFF] = -1; misc[M_LVOFF + 1] = -1; }
      unsigned pm = 0, pm_hi = 0;
      for (int j = 0; j < L; j++) {
        int32_t code;
        int32_t id = p.seq[user * L + j];
        if (p.mode == 1) code = id;             // OTM: already node ids, -1 = pad
        else if (id == 0) code = -1;            // TDMTree.idToCode, TDMTree.scala:35-56
        else if (id < p.non_leaf_offset && id >= 0 && p.id_to_code[id] >= 0) code = p.id_to_code[id];
        else {
          int32_t t = (int32_t)((uint32_t)id - (uint32_t)p.non_leaf_offset);
          code = (t > p.max_code) ? -1 : t;
        }
        if (code < -1 || code >= p.num_index) code = -1;   // host validates; keep the gather in range
        if (code == -1) { if (j < 16) pm |= 1u << j; else pm_hi |= 1u << (j - 16); }
        misc[j < 16 ? M_SEQ + j : M_SEQ_HI + j - 16] = code;
      }
      misc[M_PADMASK] = p.use_mask ? pm : 0u;
      if (KT > 1) misc[M_PADMASK_HI] = p.use_mask ? pm_hi : 0u;
    }
    team_barrier();
    PHASE_MARK(6);
    // (2) history rows straight into A-fragment registers (lane (r, g) holds K[r][16jc+4g .. +3]);
    //     the same float4s ARE the K^T B-fragments of the score GEMM.  Then on the matrix cores:
    //       T1 = K att_w^T   (Attention.linearLayer applied per history row, S/nn/Attention.scala:32)
    //       G  = T1 W1b^T    (the attention half of linear1, T/model/DIN.scala:33-34)
    {
      const int r = lane & 15, g = lane >> 4;
      float *T1s = (float *)(slotp + lo.y_keys);          // [16][E + 4]
      float *Gfw = (float *)(slotp + lo.x_gfrag);
      // one pass per key tile (history positions 16 kt_ .. 16 kt_ + 15); the T1 scratch is reused
      for (int kt_ = 0; kt_ < KT; kt_++) {
        const int hpos = 16 * kt_ + r;
        const int32_t kcode = (hpos < L) ? misc[kt_ == 0 ? M_SEQ + r : M_SEQ_HI + r] : -1;
        f32x4 ka[NJ];
        if (kcode >= 0) {
          const f32x4 *src = (const f32x4 *)(p.emb + (int64_t)kcode * E) + g;    // LookupTable.scala:35-40
#pragma unroll
          for (int jc = 0; jc < NJ; jc++) ka[jc] = src[4 * jc];
        } else {
#pragma unroll
          for (int jc = 0; jc < NJ; jc++) ka[jc] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        f32x4 *Kfw = (f32x4 *)(slotp + lo.x_kfrag) + kt_ * KBLK;
        if (tw == 0 && r < KCOLS) {
          if (SPLIT) {
            // the lane's floats of k-step s (ka[2s], ka[2s+1]) are exactly its 8 k-slots of the 16x16x32 A operand
            dm_h8 *Khw = (dm_h8 *)(slotp + lo.x_kfrag) + kt_ * KBLK;
#pragma unroll
            for (int s = 0; s < NS; s++) {
              dm_h8 hi, lw;
              dm_split8(ka[(2 * s) % NJ], ka[(2 * s + 1) % NJ], p.emb_scale, hi, lw);
              Khw[(s * 4 + g) * KCOLS + r] = hi;
              Khw[((NS + s) * 4 + g) * KCOLS + r] = lw;
            }
          } else {
#pragma unroll
            for (int jc = 0; jc < NJ; jc++) Kfw[(jc * 4 + g) * KCOLS + r] = ka[jc];
          }
        }
        for (int nt = tw; nt < NT; nt += TW) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int jc = 0; jc < NJ; jc++) {
            f32x4 bq = p.afrag[(jc * NT + nt) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[jc][t], bq[t], acc, 0, 0, 0);
          }
#pragma unroll
          for (int rr = 0; rr < 4; rr++) T1s[(4 * g + rr) * (E + 4) + 16 * nt + r] = acc[rr];
        }
        team_barrier();
        PHASE_MARK(7);
        f32x4 ta[NJ];
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) ta[jc] = *(const f32x4 *)(T1s + r * (E + 4) + 16 * jc + 4 * g);
        for (int nt = tw; nt < NT; nt += TW) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int jc = 0; jc < NJ; jc++) {
            f32x4 bq = p.bfrag[(jc * NT + nt) * 64 + lane];
#pragma unroll
            for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[jc][t], bq[t], acc, 0, 0, 0);
          }
          // C layout: acc[rr] = G[pos 16 kt_ + 4g+rr][feature 16nt+r]  ->  the A fragment of k-step 4 kt_ + g (positions 4g..4g+3 of the
          // key tile), at the lane slot (k index rr, feature r).  b1 is folded in here (every row's p sum to 1).
          float gm = 0.0f;
          if (g < KQ) {
            const float bb = B1[16 * nt + r];
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
              const float gv = (16 * kt_ + 4 * g + rr < L) ? acc[rr] + bb : 0.0f;
              Gfw[((4 * kt_ + g) * NT + nt) * 64 + rr * 16 + r] = gv;
              gm = __builtin_fmaxf(gm, __builtin_fabsf(gv));
            }
          }
          if (SPLIT) {
            unsigned gbits = __float_as_uint(gm);
            gbits = gbits < 0x7f800000u ? gbits : 0x7f800000u;     // NaN counts as "out of range"
            for (int o = 32; o > 0; o >>= 1) { const unsigned t_ = (unsigned)__shfl_xor((int)gbits, o); gbits = t_ > gbits ? t_ : gbits; }
            if (lane == 0) atomicMax((unsigned *)&misc[M_GMAX], gbits);
          }
        }
        if (kt_ + 1 < KT) team_barrier();      // every wave has its T1 fragments: the scratch takes the next key tile
      }
      if (SPLIT) {
        // The attention half of linear1 also goes to the fp16 pipe: (G + b1) * 2^sg as fp16 hi / lo planes against
        // p * 2^sp, sg + sp = the accumulator scale.  sg puts max |G + b1| into [2^13, 2^14); if p * 2^sp would then
        // leave the fp16 range (G + b1 more than 2 max|emb| max|W1a| in magnitude) the user keeps the fp32-input product.
        team_barrier();
        const unsigned gb = (unsigned)misc[M_GMAX];
        const int S = (int)((__float_as_uint(p.acc_scale) >> 23) & 0xff) - 127;           // acc_scale = 2^S
        int sp = DM_G32;
        if (gb < 0x7f800000u) {
          const int e = gb ? (int)(gb >> 23) - 126 : -126;                                // max = f * 2^e, f in [0.5, 1)
          sp = S - (14 - e);
          if (sp < -10) sp = -10;
          if (sp > 15) sp = DM_G32;
        }
        // this thread's entries: idx = tt + TT * q -> (key tile, feature tile, lane') = idx / NENT, (idx / 64) % NT, idx % 64; a one-wave
        // team (TT = 64) owns KT * NT of them
        constexpr int NENT = NT * 64;
        constexpr int NQ = KT * NT;
        float gv[NQ][4];
        if (sp != DM_G32) {
          const float gs = __uint_as_float((unsigned)(S - sp + 127) << 23);             // 2^sg
#pragma unroll
          for (int q = 0; q < NQ; q++) {
            const int idx = tt + TT * q;
            if (idx >= KT * NENT) break;
            const int t_ = idx / NENT, nt_ = (idx >> 6) % NT, m_ = idx & 15, g_ = (idx >> 4) & 3;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int pos = g_ + 4 * i;                                                  // k-slot (g_, i) of the 16x16x32 operand
              gv[q][i] = ((pos >> 2) < KQ) ? Gfw[((4 * t_ + (pos >> 2)) * NT + nt_) * 64 + (pos & 3) * 16 + m_] * gs : 0.0f;
            }
          }
          team_barrier();   // every fp32 value has been read: the planes overwrite the region
          typedef float f32x2_ __attribute__((ext_vector_type(2)));
#pragma unroll
          for (int q = 0; q < NQ; q++) {
            const int idx = tt + TT * q;
            if (idx >= KT * NENT) break;
            const dm_h2 h01 = __builtin_convertvector((f32x2_){gv[q][0], gv[q][1]}, dm_h2);
            const dm_h2 h23 = __builtin_convertvector((f32x2_){gv[q][2], gv[q][3]}, dm_h2);
            const dm_h2 l01 = __builtin_convertvector((f32x2_){gv[q][0] - (float)h01[0], gv[q][1] - (float)h01[1]}, dm_h2);
            const dm_h2 l23 = __builtin_convertvector((f32x2_){gv[q][2] - (float)h23[0], gv[q][3] - (float)h23[1]}, dm_h2);
            dm_h8 o;
            o[0] = h01[0]; o[1] = h01[1]; o[2] = h23[0]; o[3] = h23[1]; o[4] = l01[0]; o[5] = l01[1]; o[6] = l23[0]; o[7] = l23[1];
            ((dm_h8 *)Gfw)[idx] = o;
          }
        } else {
          for (int i = tt; i < KQT * NT * 64; i += TT) Gfw[i] *= p.acc_scale;             // fp32-input product, scaled accumulator
        }
        if (tt == 0) misc[M_GSP] = sp;
      }
    }
    team_barrier();   // T1 scratch in region Y is dead from here on
    // (6) initial frontier: codes [start, 2*start+1) that exist, pred 0 (Recommender.scala:53-56)
    {
      const int start = misc[M_START];
      const int n_iter0 = misc[M_NITER];
      int32_t *A0 = (int32_t *)(slotp + lo.y_acode0);
      int base = 0;
      for (int r0 = 0; r0 < CAP / 2; r0 += 4 * TT) {      // start+1 <= beam <= CAP/2
        unsigned bits = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          int i = r0 + 4 * tt + j;
          int64_t code = (int64_t)start + i;
          bool ok = n_iter0 > 0 && i <= start && p.mode != 2;
          if (ok && p.mode == 0) ok = code < p.n_slots && dm_bit(p.exists_bits, code);
          bits |= ok ? (1u << j) : 0u;
        }
        int total;
        int before = team_scan4(bits, total);
#pragma unroll
        for (int j = 0; j < 4; j++)
          if ((bits >> j) & 1u) {
            int q = base + before + __popc(bits & ((1u << j) - 1));
            A0[q] = start + r0 + 4 * tt + j; A_val[q] = 0.0f;
          }
        base += total;
      }
      if (tt == 0) misc[M_NCAND] = base;
    }
    team_barrier();
    PHASE_MARK(0);

    const int n_iter = misc[M_NITER];
    const int beam = misc[M_BEAM];
    const unsigned padmask = (unsigned)misc[M_PADMASK];
    const unsigned padmask_hi = KT > 1 ? (unsigned)misc[M_PADMASK_HI] : 0u;
    (void)padmask_hi;
    // (read into an SGPR: the branch on it encloses MFMAs and must be uniform for the compiler as well)
    const int gsp = SPLIT ? __builtin_amdgcn_readfirstlane(misc[M_GSP]) : DM_G32;   // split scorer: exponent of the scale on p, or fp32 P x G
    const float pscale = gsp != DM_G32 ? __uint_as_float((unsigned)(gsp + 127) << 23) : 1.0f;
    int cur = 0;   // which A_code buffer holds the current candidates
    // frontier size and leaf count are carried in registers (identical in every thread of the team):
    // re-reading them from LDS would race with thread 0 updating them when a phase has no barrier
    int n_cand = misc[M_NCAND];
    int leaf_tot = 0;

    // ================= level loop =================
    for (int it = 0; it < n_iter; it++) {
      int32_t *Acur = (int32_t *)(slotp + (cur ? lo.y_acode1 : lo.y_acode0));
      int32_t *Anext = (int32_t *)(slotp + (cur ? lo.y_acode0 : lo.y_acode1));
      const int n = n_cand;
      const bool first = (it == 0);
      int m_nl = n;             // non-leaf candidates (compacted at the front of Acur / A_val)
      int leaf_base = leaf_tot;
      int nchild = 0;
      if (p.mode == 2) {
        // brute force: the next chunk of this slice's leaf codes is the candidate list
        const int64_t lo_ = (work % p.bf_slices) * p.bf_per_slice + (int64_t)it * p.bf_chunk;
        int64_t hi_ = (work % p.bf_slices + 1) * p.bf_per_slice;
        if (hi_ > p.bf_n_leaf) hi_ = p.bf_n_leaf;
        int rows = (int)(hi_ - lo_ < p.bf_chunk ? hi_ - lo_ : p.bf_chunk);
        if (rows < 0) rows = 0;
        for (int i = tt; i < rows; i += TT) Anext[i] = p.bf_leaf_codes[lo_ + i];
        nchild = rows;
      } else {
      // ---- P1: split leaves / non-leaves, in order (Recommender.scala:62-70) ----
      if (p.mode == 0) {
        if (p.leaf_fast) {
          // a candidate list sits on ONE level; it is all leaves exactly at max_level
          if (it == n_iter - 1) {
            for (int i = tt; i < n; i += TT) {
              int q = leaf_base + i;
              if (q < p.ws_cap) { p.ws_code[wsb + q] = Acur[i]; p.ws_score[wsb + q] = A_val[i]; }
            }
            leaf_base += n; m_nl = 0;
          }
        } else {
          int nl = 0;
          for (int r0 = 0; r0 < n; r0 += 4 * TT) {
            unsigned lbits = 0, nbits = 0;
            int32_t cc[4]; float vv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
              int i = r0 + 4 * tt + j;
              bool valid = i < n;
              cc[j] = valid ? Acur[i] : 0; vv[j] = valid ? A_val[i] : 0.0f;
              bool isleaf = valid && dm_bit(p.leaf_bits, cc[j]);
              lbits |= isleaf ? (1u << j) : 0u;
              nbits |= (valid && !isleaf) ? (1u << j) : 0u;
            }
            int tl, tn;
            int bl = team_scan4(lbits, tl);      // barrier inside: every read of this round is done
            int bn = team_scan4(nbits, tn);
#pragma unroll
            for (int j = 0; j < 4; j++) {
              if ((nbits >> j) & 1u) { int q = nl + bn + __popc(nbits & ((1u << j) - 1)); Acur[q] = cc[j]; A_val[q] = vv[j]; }
              if ((lbits >> j) & 1u) {
                int q = leaf_base + bl + __popc(lbits & ((1u << j) - 1));
                if (q < p.ws_cap) { p.ws_code[wsb + q] = cc[j]; p.ws_score[wsb + q] = vv[j]; }
              }
            }
            nl += tn; leaf_base += tl;
            if (TW == 1) wave_sync();
          }
          m_nl = nl;
          team_barrier();
        }
        leaf_tot = leaf_base;
        if (tt == 0) misc[M_LVOFF + it + 1] = leaf_base;
      }
      // ---- P2: stable top-beam (Recommender.scala:74-87 / CandidateSearcher.scala:117-120) ----
      const bool do_sort = (p.mode == 0) ? (m_nl > beam) : !first;
      const int nb = do_sort ? (m_nl < beam ? m_nl : beam) : m_nl;
      if (do_sort) {
        int P = 2;
        while (P < m_nl) P <<= 1;
        if (TW == 1 && P <= 64) {
          const unsigned long long k1 = (lane < m_nl) ? (((unsigned long long)dm_desc_key(A_val[lane]) << 32) | (unsigned)lane) : ~0ull;
          const unsigned long long ks = sort64(k1);
          if (lane < p.pcap) keys[lane] = ks;
        } else if (P <= 256 * TW) {
          // keys (descending score key, position) are built straight into the sort registers
          unsigned long long key[4];
          const int i0 = tw * 256 + 4 * lane;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const int i = i0 + e;
            key[e] = (i < m_nl) ? (((unsigned long long)dm_desc_key(A_val[i < CAP ? i : 0]) << 32) | (unsigned)i) : ~0ull;
          }
          PHASE_MARK(9);
          reg_sort(key, P);
          PHASE_MARK(10);
          if (i0 < p.pcap) {
            *(ulonglong2 *)(keys + i0) = make_ulonglong2(key[0], key[1]);
            *(ulonglong2 *)(keys + i0 + 2) = make_ulonglong2(key[2], key[3]);
          }
        } else {
          if (P < 2 * TW) P = 2 * TW;
          const int chunk = P / TW;
          for (int i = tw * chunk + lane; i < (tw + 1) * chunk; i += 64)
            keys[i] = (i < m_nl) ? (((unsigned long long)dm_desc_key(A_val[i]) << 32) | (unsigned)i) : ~0ull;
          bitonic_sort(P);
        }
        team_barrier();
        PHASE_MARK(11);
      }
      PHASE_MARK(8);
      // ---- P3: children 2c+1, 2c+2 of the beam, in beam order, existence-filtered (:88-92) ----
      for (int r0 = 0; r0 < 2 * nb; r0 += 4 * TT) {
        unsigned bits = 0;
        int64_t ch[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          int k = r0 + 4 * tt + j;
          bool valid = k < 2 * nb;
          int64_t c = 0;
          if (valid) {
            int pi = k >> 1;
            int32_t pc = do_sort ? Acur[(uint32_t)keys[pi]] : Acur[pi];
            c = (int64_t)pc * 2 + 1 + (k & 1);
          }
          bool ok = valid;
          if (ok && p.mode == 0) ok = c < p.n_slots && dm_bit(p.exists_bits, c);
          if (ok && c >= p.num_index) ok = false;   // outside the table: the reference would throw; host validates
          ch[j] = c;
          bits |= ok ? (1u << j) : 0u;
        }
        int total;
        int before = team_scan4(bits, total);
#pragma unroll
        for (int j = 0; j < 4; j++)
          if ((bits >> j) & 1u) Anext[nchild + before + __popc(bits & ((1u << j) - 1))] = (int32_t)ch[j];
        nchild += total;
      }
      }   // mode != 2
      n_cand = nchild;
      cur ^= 1;
      team_barrier();
      PHASE_MARK(1);

      // ---- P4: score the children, 16-row tiles dealt round-robin to the team's waves ----
      __builtin_amdgcn_s_setprio(0);
      {
        const int32_t *codes = Anext;
        const int ncs = nchild;
        const int tot = (ncs + 15) >> 4;
        const int r = lane & 15, g = lane >> 4;
        // gathered embedding rows, straight to VGPRs in A-fragment order: lane (r, g) holds
        // Q[row r][16jc + 4g .. +3]; the k order inside the MFMA chain is permuted identically in B.
        auto gather = [&](f32x4 (&q)[NJ], int tile) {
          int row = tile * 16 + r;
          int32_t code = codes[row < ncs ? row : ncs - 1];
          const f32x4 *src = (const f32x4 *)(p.emb + (int64_t)code * E) + g;
#pragma unroll
          for (int jc = 0; jc < NJ; jc++) q[jc] = src[4 * jc];
        };
        // split scorer: a tile's fp16 hi / lo operands come straight from the pre-split table (dm_build_emb_split_kernel): per row
        // and k-step the lane group g finds [hi 8 halfs | lo 8 halfs], 32 contiguous bytes — no per-tile conversion on the VALU
        auto gather_split = [&](dm_h8 (&h)[NS], dm_h8 (&l)[NS], int tile) {
          int row = tile * 16 + r;
          int32_t code = codes[row < ncs ? row : ncs - 1];
          const dm_h8 *src = p.emb_split + (int64_t)code * (E / 4) + 2 * g;
#pragma unroll
          for (int s = 0; s < NS; s++) { h[s] = src[8 * s]; l[s] = src[8 * s + 1]; }
        };
        int tile = tw;
        f32x4 qa[NJ], qn[NJ];
        dm_h8 sh0[NS], sl0[NS], sh1[NS], sl1[NS];     // split scorer: operand sets of the current / next tile
        if (tile < tot) { if (SPLIT) gather_split(sh0, sl0, tile); else gather(qa, tile); }
        // A-row i = 4g' + rr' of the score product carries history position pi(i) = g' + 4 rr' (not i): the lane's four
        // scores are then positions g, g+4, g+8, g+12, and k-step rr of the attention-combine product covers the
        // CONSECUTIVE positions 4rr..4rr+3 — only ceil(L/4) steps instead of 4.
        const int kpos = (r >> 2) + 4 * (r & 3);
        const int kfi = g * KCOLS + (kpos < KCOLS - 1 ? kpos : KCOLS - 1);
        // per-lane softmax constants of the user (positions g + 4rr): x = score * smul + sadd is the scaled score for a live
        // position, exactly -FLT_MAX for a padded one (Mask.scala:20-31) and -inf for a position >= L
        float smul[KT][4], sadd[KT][4];
#pragma unroll
        for (int t = 0; t < KT; t++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const bool ispad = ((t == 0 ? padmask : padmask_hi) >> (g + 4 * rr)) & 1u, inval = 16 * t + g + 4 * rr >= L;
            smul[t][rr] = (ispad || inval) ? 0.0f : scale2;
            sadd[t][rr] = inval ? -INFINITY : (ispad ? -FLT_MAX : 0.0f);
          }
        // the loop is unrolled by two with the roles of the two row buffers swapped, so no tile ends with a 32-register copy
        auto do_tile = [&](f32x4 (&qa)[NJ], f32x4 (&qn)[NJ], dm_h8 (&qh)[NS], dm_h8 (&ql)[NS], dm_h8 (&nh)[NS], dm_h8 (&nl)[NS]) {
          const int ntile = tile + TW;
          // Every product of the tile is issued TRANSPOSED (weights / keys as the MFMA A operand, the gathered rows as
          // B): results then arrive with lane (r, g) holding 4 consecutive history positions / features OF CANDIDATE
          // ROW r, so the softmax and the final dot with w2 reduce mostly inside a lane.  On gfx950 every VALU
          // instruction takes issue cycles away from the matrix pipe (tools/mfma_microbench.hip), so the tile's VALU
          // count, not its latency, is what matters.
#ifdef DM_TILE_TIMERS
#define TILE_MARK(k) do { unsigned long long tn_ = clock64(); ttile[k] += tn_ - tt_last; tt_last = tn_; } while (0)
          unsigned long long tt_last = clock64();
#else
#define TILE_MARK(k) do {} while (0)
#endif
          // S^T = K Q^T, two interleaved accumulation chains (16x16x4 has a 40-cycle dependent latency)
          f32x4 sacc0[KT], sacc1[KT];
#pragma unroll
          for (int t = 0; t < KT; t++) { sacc0[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; sacc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
          if (SPLIT) {      // qh / ql: the tile's rows as fp16 hi / lo B operands, k-step s = columns 32s..32s+31
#pragma unroll
            for (int s = 0; s < NS; s++) {
#pragma unroll
              for (int t = 0; t < KT; t++) {
                const dm_h8 k0 = Kh[t * KBLK + s * 4 * KCOLS + kfi], k1 = Kh[t * KBLK + (NS + s) * 4 * KCOLS + kfi];
                sacc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, qh[s], sacc0[t], 0, 0, 0);
                sacc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, ql[s], sacc1[t], 0, 0, 0);
                sacc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1, qh[s], sacc1[t], 0, 0, 0);
              }
            }
          } else {
#pragma unroll
            for (int t = 0; t < KT; t++) {
              f32x4 kb[NJ];
#pragma unroll
              for (int jc = 0; jc < NJ; jc++) kb[jc] = Kf[t * KBLK + jc * 4 * KCOLS + kfi];
#ifdef DM_DBG_NO_S
              sacc0[t] = kb[0] + qa[0]; sacc1[t] = kb[1] + qa[1];
              if (false) {
#else
              if (NJ >= 2) {
#endif
#pragma unroll
                for (int jc = 0; jc < NJ; jc += 2) {
#pragma unroll
                  for (int i = 0; i < 4; i++) {
                    sacc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[jc][i], qa[jc][i], sacc0[t], 0, 0, 0);
                    sacc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[jc + (NJ >= 2 ? 1 : 0)][i], qa[jc + (NJ >= 2 ? 1 : 0)][i], sacc1[t], 0, 0, 0);
                  }
                }
              } else {
#pragma unroll
                for (int i = 0; i < 4; i++) sacc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[0][i], qa[0][i], sacc0[t], 0, 0, 0);
              }
            }
          }
          // prefetch the next tile's rows AFTER the score MFMAs are issued: they land under the softmax and
          // the main chain.  (Issued before them, hipcc's in-order vmcnt bookkeeping makes the first score
          // MFMA of every tile wait for the first of these loads.)
#ifdef DM_DBG_NO_GATHER
#pragma unroll
          for (int jc = 0; jc < NJ; jc++) qn[jc] = qa[jc];
#else
          if (SPLIT) gather_split(nh, nl, ntile < tot ? ntile : tile);
          else gather(qn, ntile < tot ? ntile : tile);   // unconditional (no branch: keeps one scheduling region)
#endif
          TILE_MARK(0);
          // softmax over the history positions 4g+rr (< L) of row r   (Mask.scala:17-35, SoftMax.scala:28-42):
          // 4 positions in the lane, the other 12 in lanes r+16, r+32, r+48
          f32x4 pr[KT];
          {
            // base-2 domain: exp(x - max) = exp2(x' - max'), x' = score * (scale * log2 e); the mask value -FLT_MAX is
            // applied after the scaling as in Mask.scala:20-31 (all-padding history -> uniform weights)
            float x[KT][4];
#pragma unroll
            for (int t = 0; t < KT; t++)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) x[t][rr] = fmaf(sacc0[t][rr] + sacc1[t][rr], smul[t][rr], sadd[t][rr]);   // scale, pad mask and position mask in one op
            float mx = __builtin_fmaxf(__builtin_fmaxf(x[0][0], x[0][1]), __builtin_fmaxf(x[0][2], x[0][3]));
            if (KT > 1) mx = __builtin_fmaxf(mx, __builtin_fmaxf(__builtin_fmaxf(x[KT - 1][0], x[KT - 1][1]), __builtin_fmaxf(x[KT - 1][2], x[KT - 1][3])));
            mx = __builtin_fmaxf(mx, dm_xor16(mx));
            mx = __builtin_fmaxf(mx, dm_xor32(mx));
            float e[KT][4];
#pragma unroll
            for (int t = 0; t < KT; t++)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) e[t][rr] = __builtin_amdgcn_exp2f(x[t][rr] - mx);   // v_exp_f32, 1 ulp; 0 for the positions >= L
            float sum = (e[0][0] + e[0][1]) + (e[0][2] + e[0][3]);
            if (KT > 1) sum += (e[KT - 1][0] + e[KT - 1][1]) + (e[KT - 1][2] + e[KT - 1][3]);
            sum += dm_xor16(sum);
            sum += dm_xor32(sum);
            const float inv = __builtin_amdgcn_rcpf(sum) * pscale;   // 1 ulp; the reference multiplies by ev.inv(sum) (SoftMax.scala:40)
#pragma unroll
            for (int t = 0; t < KT; t++)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) pr[t][rr] = e[t][rr] * inv;
          }
          TILE_MARK(1);
          // main chain: H^T = [W1a | G^T + b1] x [Q^T ; P^T], NT independent accumulators
          f32x4 acc[NT];
          if (SPLIT) {
            // per k-step and feature tile: lo*hi, hi*lo, hi*hi (small terms first), the NT accumulators interleaved so that
            // no MFMA waits on the one issued just before it
            constexpr int NB = NT < 4 ? NT : 4;   // feature tiles whose A fragments are in flight together
#pragma unroll
            for (int s = 0; s < NS; s++) {
#pragma unroll
              for (int nb = 0; nb < NT; nb += NB) {
                dm_h8 w0[NB], w1[NB];
#pragma unroll
                for (int i = 0; i < NB; i++) {
                  w0[i] = Wh[(s * NT + nb + i) * 64 + lane];
                  w1[i] = Wh[((NS + s) * NT + nb + i) * 64 + lane];
                }
#pragma unroll
                for (int i = 0; i < NB; i++)
                  acc[nb + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[i], qh[s], s == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[nb + i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < NB; i++) acc[nb + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0[i], ql[s], acc[nb + i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < NB; i++) acc[nb + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0[i], qh[s], acc[nb + i], 0, 0, 0);
              }
            }
          } else {
            f32x4 wb[2][NT];   // double-buffered A fragments: jc+1 loads fly under jc's MFMAs
#pragma unroll
            for (int nt = 0; nt < NT; nt++) wb[0][nt] = Wfrag[nt * 64 + lane];
#pragma unroll
            for (int jc = 0; jc < NJ; jc++) {
              if (jc + 1 < NJ) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) wb[(jc + 1) & 1][nt] = Wfrag[((jc + 1) * NT + nt) * 64 + lane];
              }
#pragma unroll
              for (int t = 0; t < 4; t++) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                  acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[jc & 1][nt][t], qa[jc][t],
                                                                 (jc == 0 && t == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[nt], 0, 0, 0);
              }
            }
          }
          TILE_MARK(2);
          if (SPLIT && gsp != DM_G32) {
            // one k-step of the 16x16x32 product covers every history position of a key tile: the lane's k-slots 0..3 are positions
            // g, g+4, g+8, g+12 (its own p), slots 4..7 are zero on both sides
            typedef float f32x2_ __attribute__((ext_vector_type(2)));
            const dm_h8 *Gh = (const dm_h8 *)Gf;
            constexpr int NB = NT < 4 ? NT : 4;
#pragma unroll
            for (int t = 0; t < KT; t++) {
              const dm_h2 p01 = __builtin_convertvector((f32x2_){pr[t][0], pr[t][1]}, dm_h2);
              const dm_h2 p23 = __builtin_convertvector((f32x2_){pr[t][2], pr[t][3]}, dm_h2);
              const dm_h2 q01 = __builtin_convertvector((f32x2_){pr[t][0] - (float)p01[0], pr[t][1] - (float)p01[1]}, dm_h2);
              const dm_h2 q23 = __builtin_convertvector((f32x2_){pr[t][2] - (float)p23[0], pr[t][3] - (float)p23[1]}, dm_h2);
              // the LDS word of a lane is already [hi(4) | lo(4)] of (G + b1): against [p_hi | p_hi] one MFMA gives hi*hi + lo*hi,
              // against [p_lo | 0] a second one gives hi*lo — two MFMAs per feature tile, the unused half of K carries the cross term
              const dm_h8 pb0 = {p01[0], p01[1], p23[0], p23[1], p01[0], p01[1], p23[0], p23[1]};
              const dm_h8 pb1 = {q01[0], q01[1], q23[0], q23[1], 0, 0, 0, 0};
#pragma unroll
              for (int nb = 0; nb < NT; nb += NB) {
                dm_h8 gv[NB];
#pragma unroll
                for (int i = 0; i < NB; i++) gv[i] = Gh[(t * NT + nb + i) * 64 + lane];
#pragma unroll
                for (int i = 0; i < NB; i++) acc[nb + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(gv[i], pb1, acc[nb + i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < NB; i++) acc[nb + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(gv[i], pb0, acc[nb + i], 0, 0, 0);
              }
            }
          } else {
            // k-step rr of key tile t multiplies positions 16t + 4rr + g: A = (G + b1)^T fragments written at user setup, B = the
            // lane's own p (fetching these one k-step ahead was measured: no gain)
#pragma unroll
            for (int t = 0; t < KT; t++)
#pragma unroll
              for (int rr = 0; rr < KQ; rr++) {
                float gb[NT];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) gb[nt] = Gf[((4 * t + rr) * NT + nt) * 64 + lane];
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                  acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gb[nt], pr[t][rr], acc[nt], 0, 0, 0);
              }
          }
          TILE_MARK(3);
          // epilogue: relu(h) . w2 + b2 (b1 rides in G: the p of a row sum to 1)   (Linear.scala:41-48, ReLU.scala:30-44)
          // acc[nt][rr] = h[row r][feature 16nt + 4g + rr]
          typedef float f32x2 __attribute__((ext_vector_type(2)));
          f32x2 part2 = {0.f, 0.f};
#ifdef DM_DBG_NO_EPI
          for (int nt = 0; nt < NT; nt++) part2[0] += acc[nt][0];
          if (false)
#endif
#pragma unroll
          for (int nt = 0; nt < NT; nt++) {
            const f32x4 ww = *(const f32x4 *)(W2 + 16 * nt + 4 * g);
            float hh[4];
#pragma unroll
            for (int rr = 0; rr < 4; rr++)      // relu in ONE VALU op the compiler can see (fmaxf would first canonicalise its input; inline
              hh[rr] = __builtin_amdgcn_fmed3f(acc[nt][rr], 0.0f, __builtin_inff());   // asm would hide the MFMA -> VALU hazard from it)
            part2 = __builtin_elementwise_fma((f32x2){hh[0], hh[1]}, (f32x2){ww[0], ww[1]}, part2);   // v_pk_fma_f32
            part2 = __builtin_elementwise_fma((f32x2){hh[2], hh[3]}, (f32x2){ww[2], ww[3]}, part2);
          }
          float part = part2[0] + part2[1];
          part += dm_xor16(part);
          part += dm_xor32(part);
          {
            const int orow = tile * 16 + r;
            if (g == 0 && orow < ncs) A_val[orow] = part + p.b2;
          }
          if (lane == 0) { int rows = ncs - tile * 16; my_rows += rows > 16 ? 16 : rows; }
          TILE_MARK(4);
          tile = ntile;
        };
        // the loop is unrolled by two with the roles of the two row / operand sets swapped: no tile ends with a register copy
        while (tile < tot) {
          do_tile(qa, qn, sh0, sl0, sh1, sl1);
          if (tile >= tot) break;
          do_tile(qn, qa, sh1, sl1, sh0, sl0);
        }
        PHASE_MARK(2);
      }
      // short serial phases (sort / expand / setup) outrank the co-resident team's MFMA stream:
      // they need few issue slots, and finishing them early puts this wave back on the matrix pipe
      __builtin_amdgcn_s_setprio(3);
      team_barrier();
      PHASE_MARK(3);
      if (p.mode == 2) {
        // keep every row that beats the current k-th best; sort + truncate only when the pool could overflow
        const unsigned long long T = ((unsigned long long)(unsigned)misc[M_LVOFF + 1] << 32) | (unsigned)misc[M_LVOFF];
        for (int i = tt; i < nchild; i += TT) {
          const unsigned long long key = ((unsigned long long)dm_desc_key(A_val[i]) << 32) | (unsigned)Anext[i];
          if (key < T) { int q = atomicAdd(&misc[M_NPOOL], 1); keys[q] = key; }
        }
        team_barrier();
        int n_pool = misc[M_NPOOL];
        if (n_pool + p.bf_chunk > p.pcap || it == n_iter - 1) {
          unsigned long long key[4];
          const int i0 = tw * 256 + 4 * lane;
#pragma unroll
          for (int e = 0; e < 4; e++) key[e] = (i0 + e < n_pool) ? keys[i0 + e] : ~0ull;
          team_barrier();
          reg_sort(key, p.pcap);
          if (i0 < p.pcap) {
            *(ulonglong2 *)(keys + i0) = make_ulonglong2(key[0], key[1]);
            *(ulonglong2 *)(keys + i0 + 2) = make_ulonglong2(key[2], key[3]);
          }
          team_barrier();
          if (n_pool > p.topk) n_pool = p.topk;
          if (tt == 0) {
            misc[M_NPOOL] = n_pool;
            const unsigned long long Tn = (n_pool == p.topk) ? keys[p.topk - 1] : ~0ull;
            misc[M_LVOFF] = (int)(unsigned)Tn; misc[M_LVOFF + 1] = (int)(unsigned)(Tn >> 32);
          }
          team_barrier();
        }
      }
      if (p.trace_counts && it < p.trace_levels) {
        int64_t tb = (user * p.trace_levels + it);
        if (tt == 0) p.trace_counts[tb] = nchild;
        for (int i = tt; i < nchild; i += TT) { p.trace_codes[tb * CAP + i] = Anext[i]; p.trace_scores[tb * CAP + i] = A_val[i]; }
      }
    }  // levels

    // ================= final selection =================
    if (p.mode == 2) {
      const int n_pool = misc[M_NPOOL];
      for (int i = tt; i < p.topk; i += TT) p.bf_out_keys[work * p.topk + i] = (i < n_pool) ? keys[i] : ~0ull;
      team_barrier();
      continue;
    }
    if (p.mode == 1) {
      // OTM: the leaf-level candidates in order (CandidateSearcher.scala:58-80 returns them unsorted)
      const int32_t *Acur = (const int32_t *)(slotp + (cur ? lo.y_acode1 : lo.y_acode0));
      const int nn = n_cand;
      if (tt == 0) p.out_counts[user] = nn;
      for (int i = tt; i < nn && i < p.out_stride; i += TT) {
        p.out_ids[user * p.out_stride + i] = Acur[i];
        p.out_scores[user * p.out_stride + i] = A_val[i];
      }
      team_barrier();
      continue;
    }
    // TDM: leaves are in ws in level-block order; the reference's list has the LATEST block first
    // (leafNodes ++: levelInfo.leafNodes, Recommender.scala:65-70), then drops consumed ids (:103-106),
    // then TDM.recommend does a stable sortBy(-pred).take(topk) (TDM.scala:21).
    {
      int out_n = 0;
      const int total = leaf_tot < p.ws_cap ? leaf_tot : p.ws_cap;
      const int nblk = n_iter;
      const int64_t c0 = p.consumed_off ? p.consumed_off[user] : 0;
      const int64_t c1 = p.consumed_off ? p.consumed_off[user + 1] : 0;
      int P = 2;
      while (P < total) P <<= 1;
      if (P < 2 * TW) P = 2 * TW;
      if (P <= p.pcap) {
        // sort keys (descending score key, position in the reference's list order); dropped -> +inf
        const bool in_regs = P <= 256 * TW;
        const bool small = TW == 1 && P <= 64;          // one key per lane (sort64)
        const bool lds_leaves = small && p.leaf_fast && total <= CAP;
        const int32_t *Aleaf = (const int32_t *)(slotp + (cur ? lo.y_acode0 : lo.y_acode1));
        int32_t *Sid = (int32_t *)(slotp + (cur ? lo.y_acode1 : lo.y_acode0));
        unsigned long long rkey[4] = {~0ull, ~0ull, ~0ull, ~0ull};
        const int chunk = small ? 64 : (in_regs ? 256 : P / TW);
        int kept_local = 0;
        for (int q4 = 0; q4 * 64 < chunk; q4++) {
          const int i = small ? lane : (in_regs ? (tw * 256 + 4 * lane + q4) : (tw * chunk + q4 * 64 + lane));
          unsigned long long key = ~0ull;
          if (i < total) {
            // one-wave team whose leaves all sit on the last level: they are still in the frontier arrays (codes in the buffer the
            // last iteration read, scores in A_val, list position = index) — no round trip through the global leaf list
            int32_t code = lds_leaves ? Aleaf[i] : p.ws_code[wsb + i];
            float sc = lds_leaves ? A_val[i] : p.ws_score[wsb + i];
            int32_t id = p.node_id[code];
            bool drop = false;
            for (int64_t q = c0; q < c1; q++) drop |= (p.consumed_ids[q] == id);
            int b = 0;
            while (b + 1 < nblk && i >= misc[M_LVOFF + b + 1]) b++;
            int pos = (total - misc[M_LVOFF + b + 1]) + (i - misc[M_LVOFF + b]);
            if (lds_leaves) Sid[pos] = id;
            if (!drop) { key = ((unsigned long long)dm_desc_key(sc) << 32) | (unsigned)pos; kept_local++; }
          }
          if (in_regs) {
            if (q4 == 0) rkey[0] = key; else if (q4 == 1) rkey[1] = key; else if (q4 == 2) rkey[2] = key; else rkey[3] = key;
          } else {
            keys[i] = key;
          }
        }
        if (kept_local) atomicAdd(&misc[M_KEPT], kept_local);
        if (small) {
          const unsigned long long ks = sort64(rkey[0]);
          if (lane < p.pcap) keys[lane] = ks;
        } else if (in_regs) {
          reg_sort(rkey, P);
          const int i0 = tw * 256 + 4 * lane;
          if (i0 < p.pcap) {
            *(ulonglong2 *)(keys + i0) = make_ulonglong2(rkey[0], rkey[1]);
            *(ulonglong2 *)(keys + i0 + 2) = make_ulonglong2(rkey[2], rkey[3]);
          }
        } else {
          bitonic_sort(P);
        }
        team_barrier();
        const int kept = misc[M_KEPT];
        const int nout = kept < p.topk ? kept : p.topk;
        if (lds_leaves) {
          for (int rk = tt; rk < nout; rk += TT) {
            const int pos = (int)(uint32_t)keys[rk];          // leaves of ONE level: list position == frontier index
            p.out_ids[user * p.out_stride + rk] = Sid[pos];
            p.out_scores[user * p.out_stride + rk] = A_val[pos];
          }
        } else
        for (int rk = tt; rk < nout; rk += TT) {
          int pos = (int)(uint32_t)keys[rk];
          // invert pos -> ws index: block b covers positions [total - lvoff[b+1], total - lvoff[b])
          int b = 0;
          while (b + 1 < nblk && pos < total - misc[M_LVOFF + b + 1]) b++;
          int i = misc[M_LVOFF + b] + (pos - (total - misc[M_LVOFF + b + 1]));
          p.out_ids[user * p.out_stride + rk] = p.node_id[p.ws_code[wsb + i]];
          p.out_scores[user * p.out_stride + rk] = p.ws_score[wsb + i];
        }
        out_n = nout;
      } else {
        // leaf list outgrew the LDS key area (trees with leaves on many levels): exact O(n^2) ranking
        uint32_t *khi = p.ws_khi + wsb, *klo = p.ws_klo + wsb;
        int kept_local = 0;
        for (int i = tt; i < total; i += TT) {
          int32_t code = p.ws_code[wsb + i];
          int32_t id = p.node_id[code];
          bool drop = false;
          for (int64_t q = c0; q < c1; q++) drop |= (p.consumed_ids[q] == id);
          int b = 0;
          while (b + 1 < nblk && i >= misc[M_LVOFF + b + 1]) b++;
          int pos = (total - misc[M_LVOFF + b + 1]) + (i - misc[M_LVOFF + b]);
          khi[i] = dm_desc_key(p.ws_score[wsb + i]);
          klo[i] = drop ? 0xFFFFFFFFu : (uint32_t)pos;
          kept_local += drop ? 0 : 1;
        }
        if (kept_local) atomicAdd(&misc[M_KEPT], kept_local);
        team_barrier();
        for (int i = tt; i < total; i += TT) {
          uint32_t hi = khi[i], lp = klo[i];
          if (lp == 0xFFFFFFFFu) continue;
          int rank = 0;
          for (int j = 0; j < total; j++) {
            uint32_t hj = khi[j], lj = klo[j];
            rank += (lj != 0xFFFFFFFFu) && ((hj < hi) || (hj == hi && lj < lp));
          }
          if (rank < p.topk) {
            p.out_ids[user * p.out_stride + rank] = p.node_id[p.ws_code[wsb + i]];
            p.out_scores[user * p.out_stride + rank] = p.ws_score[wsb + i];
          }
        }
        out_n = misc[M_KEPT] < p.topk ? misc[M_KEPT] : p.topk;
      }
      if (p.host_direct) {
        for (int rk = out_n + tt; rk < p.topk; rk += TT) { p.out_ids[user * p.out_stride + rk] = -1; p.out_scores[user * p.out_stride + rk] = 0.0f; }
        __threadfence_system();      // every result store of this thread has reached host memory ...
        team_barrier();              // ... for every thread of the team ...
        if (tt == 0) __hip_atomic_store(&p.out_counts[user], out_n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);     // ... before the flag
      } else if (tt == 0) p.out_counts[user] = out_n;
    }
    team_barrier();   // slot state is rewritten by the next user
  }  // users
  if (lane == 0 && my_rows) atomicAdd(p.scored_rows, my_rows);
#ifdef DM_PHASE_TIMERS
  PHASE_MARK(4);
  if (lane == 0 && p.phase_cycles) for (int k = 0; k < 12; k++) atomicAdd(p.phase_cycles + k, tph[k]);
#endif
#ifdef DM_TILE_TIMERS
  if (lane == 0 && p.phase_cycles) for (int k = 0; k < 5; k++) atomicAdd(p.phase_cycles + k, ttile[k]);
#endif
}
