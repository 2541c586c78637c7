// libdismember_hip.so — MI355X (gfx950) implementation of dismember's tree beam-search
// retrieval hot path behind the C ABI of include/dismember_hip.h.
//
// No CPU fallback lives here: every entry point that computes launches HIP kernels.
#include "../../include/dismember_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <mutex>
#include <thread>
#include <utility>
#include <cerrno>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "beam_kernel.hip.inc"
#include "beam_kernel_w.hip.inc"
#include "beam_kernel_f64.hip.inc"
#include "rows_kernel.hip.inc"
#include "train_kernel.hip.inc"
#include "train_grouped_f64.hip.inc"
#include "dr_kernel.hip.inc"
#include "dr_sliced.hip.inc"

#define DM_VERSION 100

#include "dev_mem.hip.inc"
#define DM_LAZY_COPIES_PART 1      // struct LazyCopies
#include "lazy_copies.hip.inc"
#define DM_ADAM_VEC_PART 1         // struct TrainVec
#include "adam_vec.hip.inc"
// ------------------------------------------------------------------ context
struct dm_dr_state;
static void dm_dr_free(dm_dr_state *s);

// what the last gradient exchange on a handle moved (comm.hip.inc; dm_train_sync_stats)
struct dm_sync_stats { uint64_t rows_mine, rows_total, bytes_sent, bytes_recv; int host_syncs, nranks, transport; };

// what the last dm_jtm_optimize_cached on a handle did (jtm_sharded.hip.inc; dm_jtm_optimize_stats)
struct dm_jtm_stats {
  int nranks = 1, transport = -1, steps_replicated = 0, steps_node_sharded = 0;
  uint64_t items_scored = 0, items_rebalanced = 0, weight_bytes = 0, proj_bytes = 0;
  double scoring_s = 0, rebalance_s = 0, exchange_s = 0;
};

// what the last dm_otm_train_batch on a handle did (otm_train.hip.inc; dm_otm_train_stats)
struct dm_otm_stats {
  uint64_t users = 0, target_rows = 0, train_rows = 0;
  int levels = 0;
  double targets_s = 0, beam_s = 0, fwdbwd_s = 0, exchange_s = 0, adam_s = 0;
};

// The handle's counter block on the device (dm_ctx::d_ctr): the kernels get the address of a field, the host never dereferences it.
struct SearchCounters {
  unsigned long long rows;             // candidate rows scored by the last search (dm_last_scored_rows)
  unsigned long long queue_head;       // work-queue head of the persistent beam kernels
  unsigned long long dr_slow;          // Deep-Retrieval layers that took the exact path (dm_debug_dr_slow_layers)
  unsigned long long rows_sink;        // where the single-request paths count their rows: never zeroed, never read
  unsigned long long unused4;
  unsigned long long dr_wave_count;    // user-layers the one-wave cut handed to the block version, and one byte counter per
  unsigned long long dr_wave_reasons;  // reason (dm_debug_dr_wave_fallbacks)
  unsigned long long unused7;
};
// drs_select_wave_kernel (dr_sliced.hip.inc) reaches the two fallback counters as slow_count + 3 and slow_count + 4
static_assert(offsetof(SearchCounters, dr_wave_count) == offsetof(SearchCounters, dr_slow) + 3 * 8 &&
              offsetof(SearchCounters, dr_wave_reasons) == offsetof(SearchCounters, dr_slow) + 4 * 8 && sizeof(SearchCounters) == 64,
              "the kernels address the block by slot");

struct dm_ctx {
  int device = 0;
  int n_cu = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // dm_clone: a clone reads the tree, the weights and every derived copy of its parent (same device memory) through its own stream,
  // request arenas and workspace.  model_epoch counts the changes of anything a clone mirrors; mu serialises the lazy rebuilds.
  dm_ctx *parent = nullptr;
  std::atomic<int> n_clones{0};
  std::atomic<uint64_t> model_epoch{1};
  uint64_t seen_epoch = 0;
  uint64_t ids_epoch = 1;      // generation of the id maps (dm_load_id_maps) and the tree bitmaps (dm_load_tree_tdm)
  uint64_t seen_ids_epoch = 0; // clone: the owner's generation its host copies were taken at
  std::recursive_mutex mu;
  // tree (codeNodeMap as bitmaps + dense node-id array)
  bool tree_loaded = false, ids_loaded = false, leaves_at_max_only = true;
  int max_level = 0;
  int64_t n_slots = 0, n_leaf_nodes = 0;
  uint32_t *d_exists = nullptr, *d_leaf = nullptr;
  int32_t *d_level_last = nullptr;                          // per-level existence bounds (dm_level_bounds_bits), [DM_N_LEVEL_BOUNDS]
  std::array<int32_t, DM_N_LEVEL_BOUNDS> level_last{};      //   and their host copy
  int32_t *d_node_id = nullptr, *d_id_to_code = nullptr, *d_leaf_codes = nullptr;
  int32_t non_leaf_offset = -1, max_code = -1;
  std::vector<int32_t> h_id_to_code;
  std::vector<uint32_t> h_exists;      // host copy of the existence bitmap (negative sampling)
  // weights
  bool w_loaded = false;
  int dtype = DM_F32, embed = 0;
  int embed_log = 0;           // the MODEL's embed size; embed is the kernels' (16 / 32 / 64 / 128): other sizes are zero-padded at load
  int64_t num_index = 0;
  void *d_compact = nullptr;   // as loaded (float or double)
  float *d_emb32 = nullptr;    // f32 table (aliases d_compact for DM_F32)
  bool emb32_owned = false;
  f32x4 *d_wfrag = nullptr;
  f32x4 *d_afrag = nullptr, *d_bfrag = nullptr;
  f32x4 *d_attA = nullptr, *d_w1aA = nullptr, *d_w1bA = nullptr;   // A-fragment order (rows kernel)
  float *d_b1 = nullptr, *d_w2 = nullptr;
  float b2 = 0.f;
  void *d_att_wT_t = nullptr, *d_l1T_t = nullptr;  // transposes in the loaded dtype (general forward)
  // which scorer the loaded weights are (dm_get_scorer_kind).  DeepFM (deepfm.hip.inc): d_compact holds [emb ; l1.W ; l1.b ; l2.W ; l2.b]
  // with every E-wide block padded to `embed`, none of the DIN copies above exists, and b2 is l2.b
  int scorer_kind = DM_KIND_DIN;
  int dfm_L = 0;               // DeepFM: the history length l1.W is sized by
  float *d_dfm_frag = nullptr; // DeepFM: [0 ; W1a ; 0] as MFMA B fragments, and l2.W over the same padded columns
  float *d_dfm_w2p = nullptr;
  float *d_dfm_fragS = nullptr; // DeepFM: W1s as MFMA B fragments (dfm_jtm_derive_kernel), for the per-history set-up of the pair scorer
  struct dm_dfm_train *dfm_tr = nullptr;   // DeepFM training state (dm_deepfm_train_init, dfm_train.hip.inc): the owner's, never mirrored by a clone
  struct dm_dfm_otm_tree *dfm_otree = nullptr;   // DeepFM: what dm_deepfm_otm_tree_prepare keeps (dfm_otm_tree.hip.inc): the owner's, dropped with the weights
  LazyCopies lazy;             // the copies rebuilt on first use after a weight change, and their stale flags (lazy_copies.hip.inc)
  int scorer_mode = DM_SCORER_AUTO;      // dm_set_scorer_mode
  bool beam_w = true;          // split scorer on the one-wave-per-SIMD kernel (beam_kernel_w.hip.inc); DM_BEAM_W=0 in the environment selects the LDS-fed kernel
  double jtm_score_s = 0, jtm_rebal_s = 0;   // dm_jtm_last_step_seconds
  DevGrow dfm_jtm_ws;          // DeepFM pair scorer (dfm_jtm.hip.inc): s and aux of one slice of histories
  DevGrow scratch64;           // fp64 beam kernel (beam_kernel_f64.hip.inc): per-team K / G fragment scratch
  // training state (dm_train_init)
  bool train_ready = false;
  TrainVec train;                // gradient, Adam moments, active rows, options and time step of the compact vector (adam_vec.hip.inc)
  void *d_loss = nullptr;        // in the loaded dtype
  void *d_tr64 = nullptr;        // f64 model: A fragments of att.W, W1a, W1b and of their transposes for the training kernels
  void *d_tail32 = nullptr;      // f64 model: f32 copy of the small matrices (source of the f32 mirror's fragments)
  double last_loss = 0.0;
  f32x4 *d_attTA = nullptr, *d_w1aTA = nullptr, *d_w1bTA = nullptr;
  unsigned *d_touch_bits = nullptr;
  int32_t *d_touch_list = nullptr;
  unsigned long long *d_touch_cnt = nullptr;
  int adam_last_sparse = 0; unsigned long long adam_last_rows = 0;
  size_t touch_cap = 0, touch_ub = 0;   // list capacity; host-side upper bound of its length since the last Adam step
  // measurement
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  std::vector<int> ev_kind;    // per pair: what it was recorded as (EvKind, host_request.hip.inc)
  bool time_direct = false;    // DM_TIME_DIRECT=1: the single-request path, which launches without an event pair, records one too (probes)
  bool direct_ok = true;       // host-mapped single-request path enabled (DM_NO_DIRECT=1 turns it off)
  bool last_g_table = false;   // ... and whether that search's setup read the per-row table (dm_debug_g_table)
  char last_kernel[64] = "";   // the search kernel of the last beam search (measurement: dm_last_beam_kernel)
  SearchCounters *d_ctr = nullptr;
  unsigned long long *d_phase = nullptr;   // 8 debug counters
  // Deep-Retrieval model (dm_dr_load_model)
  dm_dr_state *dr = nullptr;
  // request arena of the host-buffer entry points (grow only: no hipMalloc / hipFree on the request path)
  DevGrow req;
  char *h_stage = nullptr;     // pinned staging block for small host-buffer requests (one upload, one download per call)
  char *d_stage = nullptr;     // the same block as the kernels address it (hipHostGetDevicePointer): single-request path
  size_t stage_bytes = 0;
  // pipelined host-buffer searches (host_pipe_*): a second, non-blocking stream for the result downloads + one event per chunk
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> chunk_ev;
  // cached search workspace
  DevGrow ws;
  // device-side negative sampler (sampler.hip.inc): per-level code / cumulative-probability tables, per-call scratch
  int32_t *d_lv_codes = nullptr;
  double *d_lv_cdf = nullptr;
  int64_t *d_lv_start = nullptr;
  DevGrow samp;
  // multi-GPU exchange (comm.hip.inc): the attached communicator (not owned) and the staging area of dm_train_sync_gradients
  DevGrow defer;                 // users the W kernel hands to the LDS-fed kernel: [count u64 | queue head u64 | ids]
  // JTM: the catalogue's training rows kept on the device across gap steps (dm_jtm_cache_rows)
  int64_t *d_jtm_off = nullptr;
  int32_t *d_jtm_ritem = nullptr, *d_jtm_rids = nullptr;
  int32_t *d_jtm_rseq = nullptr;       // the rows' history CODES [rows][L] and pad masks [rows] (built once per cached catalogue and id map:
  unsigned *d_jtm_rmask = nullptr;     //  they do not change between the gap steps unless the ancestors are taken per level — hierarchical mode)
  uint64_t jtm_rseq_ids_epoch = 0;     // id-map generation the codes were built from
  int64_t jtm_rseq_num_index = 0;      // ... and the table size they were bounds-checked against
  std::vector<int64_t> jtm_off;
  int64_t jtm_i_lo = 0, jtm_i_hi = 0, jtm_R_base = 0;      // the items whose rows are on this device (dm_jtm_cache_rows_range) and their first row
  int jtm_L = 0;
  struct dm_comm *comm = nullptr;
  dm_sync_stats sync_stats{};
  dm_jtm_stats jtm_stats{};
  dm_otm_stats otm_stats{};
  DevGrow sync;
  DevGrow dra, dra_io;           // the M-step's path assignment (dr_mstep_assign.hip.inc): every array of a call; the host entries' uploads and results
};

static std::string g_create_err;

#define HIPCHK(h, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      char b_[512];                                                                       \
      snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      (h)->err = b_;                                                                      \
      return DM_ERR_HIP;                                                                  \
    }                                                                                     \
  } while (0)

static int fail(dm_ctx *h, int code, const std::string &msg) {
  if (h) h->err = msg; else g_create_err = msg;
  return code;
}

// The one embed-size dispatch of the kernel templates: f(std::integral_constant<int, E>) for E = 16 / 32 / 64 / 128, from MIN_E up
// (the split-fp16 kernels start at 32: no smaller instance exists, none is instantiated here); any other size fails with the caller's
// message.  Development builds (tools/build_probe.sh DM_DEV_LIGHT ...) compile the E = 128 instances only — a third of the compile
// time while iterating on one kernel.  Never the product build: models of other embedding sizes fail with "unsupported".
template <int MIN_E = 16, typename F>
static int dispatch_E(dm_ctx *h, int E, const char *unsupported, F &&f) {
#ifndef DM_DEV_LIGHT
  if constexpr (MIN_E <= 16) { if (E == 16) return f(std::integral_constant<int, 16>{}); }
  if (E == 32) return f(std::integral_constant<int, 32>{});
  if (E == 64) return f(std::integral_constant<int, 64>{});
#endif
  if (E == 128) return f(std::integral_constant<int, 128>{});
  return fail(h, DM_ERR_UNSUPPORTED, unsupported);
}

// The DeepFM kernel templates are also instantiated per number of 16-column tiles: f(integral_constant<E>, integral_constant<NCT>), NCT = 1 .. 3
template <typename F>
static int dispatch_E_NCT(dm_ctx *h, int E, int NCT, const char *unsupported, F &&f) {
  return dispatch_E(h, E, unsupported, [&](auto e) {
    return NCT == 1 ? f(e, std::integral_constant<int, 1>{}) : NCT == 2 ? f(e, std::integral_constant<int, 2>{}) : f(e, std::integral_constant<int, 3>{});
  });
}

// LookupTable.embeddingLookup validates every index first (LookupTable.scala:29-53): -1 is the padding index, anything else outside
// [0, num_index) fails with the reference's message, which names `noun` i / div (the row, pair or history that holds ids[i])
static int check_lookup_ids(dm_ctx *h, const int32_t *ids, int64_t n, int64_t div, const char *noun) {
  for (int64_t i = 0; i < n; i++)
    if (ids[i] < -1 || ids[i] >= h->num_index) {
      char b[160]; snprintf(b, sizeof b, "embeddingLookup failed, valid index range is [0, %lld), %s %lld got %d", (long long)h->num_index, noun, (long long)(i / div), ids[i]);
      return fail(h, DM_ERR_INDEX, b);
    }
  return DM_OK;
}

// The OTM and training entry points' own check of host ids: every ids[i] in [lowest, num_index), or "<who>: <noun> outside the
// embedding table".  lowest = -1 admits the padding id; node codes that must exist (targets) pass 1.
static int check_table_ids(dm_ctx *h, const char *who, const char *noun, const int32_t *ids, int64_t n, int32_t lowest) {
  for (int64_t i = 0; i < n; i++)
    if (ids[i] < lowest || ids[i] >= h->num_index) return fail(h, DM_ERR_INDEX, std::string(who) + ": " + noun + " outside the embedding table");
  return DM_OK;
}

// ------------------------------------------------------------ small kernels
__global__ void dm_f64_to_f32_kernel(const double *in, float *out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (float)in[i];
}

__global__ void dm_pad_rowmask_kernel(const int32_t *pad_flat, int64_t n_pad, int L, unsigned *rowmask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pad) {
    int64_t idx = pad_flat[i];
    atomicOr(&rowmask[idx / L], 1u << (idx % L));
  }
}

// General DIN forward, one wave per row, any (code, history, mask) per row:
// Module.forward of tdm/.../model/DIN.scala:18-42 for arbitrary batches (the beam kernels
// use the per-user restructured form instead).  T = float | double.
template <typename T>
struct DinFwdParams {
  const T *emb, *att_wT, *l1T, *b1, *w2;  // att_wT [E k][E o], l1T [2E k][E o]
  T b2;
  int E, L;
  int64_t B;
  const int32_t *codes, *seqs;
  const unsigned *rowmask;
  T *out;
  T sm_scale;                  // 1 / sqrt(embedSize) of the model (the table may be zero-padded to E)
};

template <typename T>
__device__ __forceinline__ T dm_wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void dm_din_forward_kernel(DinFwdParams<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem_fw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = p.E, L = p.L;
  T *q = (T *)smem_fw + (size_t)wave * (3 * E + 32);
  T *comb = q + E, *att = comb + E, *sc = att + E;
  const T scale = p.sm_scale;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < p.B; row += (int64_t)gridDim.x * 4) {
    const int32_t code = p.codes[row];
    for (int e = lane; e < E; e += 64) q[e] = code >= 0 ? p.emb[(int64_t)code * E + e] : (T)0;
    __builtin_amdgcn_wave_barrier();
    const unsigned mask = p.rowmask ? p.rowmask[row] : 0u;
    for (int j = 0; j < L; j++) {
      const int32_t c = p.seqs[row * L + j];
      T part = 0;
      if (c >= 0)
        for (int e = lane; e < E; e += 64) part += q[e] * p.emb[(int64_t)c * E + e];
      T s = dm_wave_sum(part) * scale;
      if ((mask >> j) & 1u) s = (T)(-FLT_MAX);
      if (lane == 0) sc[j] = s;
    }
    __builtin_amdgcn_wave_barrier();
    T mx = sc[0];
    for (int j = 1; j < L; j++) mx = sc[j] > mx ? sc[j] : mx;
    T sum;
    sum = 0;
    for (int j = 0; j < L; j++) {
      T e = sizeof(T) == 4 ? (T)expf((float)(sc[j] - mx)) : (T)exp((double)(sc[j] - mx));
      sum += e;
    }
    const T inv = (T)1 / sum;
    for (int e = lane; e < E; e += 64) comb[e] = 0;
    for (int j = 0; j < L; j++) {
      const int32_t c = p.seqs[row * L + j];
      T ex = sizeof(T) == 4 ? (T)expf((float)(sc[j] - mx)) : (T)exp((double)(sc[j] - mx));
      T pj = ex * inv;
      if (c >= 0)
        for (int e = lane; e < E; e += 64) comb[e] += pj * p.emb[(int64_t)c * E + e];
    }
    __builtin_amdgcn_wave_barrier();
    for (int o = lane; o < E; o += 64) {
      T a = 0;
      for (int k = 0; k < E; k++) a += comb[k] * p.att_wT[(size_t)k * E + o];
      att[o] = a;
    }
    __builtin_amdgcn_wave_barrier();
    T part = 0;
    for (int o = lane; o < E; o += 64) {
      T hsum = 0;
      for (int k = 0; k < E; k++) hsum += q[k] * p.l1T[(size_t)k * E + o];
      for (int k = 0; k < E; k++) hsum += att[k] * p.l1T[(size_t)(E + k) * E + o];
      hsum += p.b1[o];
      hsum = hsum > 0 ? hsum : (T)0;
      part += hsum * p.w2[o];
    }
    T logit = dm_wave_sum(part) + p.b2;
    if (lane == 0) p.out[row] = logit;
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------ helpers
static int dm_alloc(dm_ctx *h, void **p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes ? bytes : 16);       // h == nullptr: an owner without a handle (the communicator's staging block)
  if (e != hipSuccess) return fail(h, DM_ERR_HIP, std::string("hipMalloc(") + std::to_string(bytes) + " bytes) failed: " + hipGetErrorString(e));
  dm_live_add(*p, bytes ? bytes : 16);
  return DM_OK;
}
#define ALLOC(h, ptr, bytes)                                   \
  do {                                                         \
    int rc_ = dm_alloc((h), (void **)&(ptr), (bytes));         \
    if (rc_ != DM_OK) return rc_;                              \
  } while (0)

// The 256 KB pinned staging block of the small-request paths.  It is also what the single-request kernels read and write in place
// and whose count words the host polls, so it is allocated COHERENT explicitly (fine-grained: device stores become visible to the
// host without a kernel boundary) and the kernels get the address hipHostGetDevicePointer reports, not the host pointer.
static int ensure_stage(dm_ctx *h) {
  if (h->h_stage && h->stage_bytes >= (256u << 10)) return DM_OK;
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  h->h_stage = nullptr; h->d_stage = nullptr; h->stage_bytes = 0;
  if (hipHostMalloc((void **)&h->h_stage, 256u << 10, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess)
    return fail(h, DM_ERR_HIP, "hipHostMalloc failed");
  void *dp = nullptr;
  if (hipHostGetDevicePointer(&dp, h->h_stage, 0) != hipSuccess || !dp) {
    (void)hipHostFree(h->h_stage); h->h_stage = nullptr;
    return fail(h, DM_ERR_HIP, "hipHostGetDevicePointer failed");
  }
  h->d_stage = (char *)dp; h->stage_bytes = 256u << 10;
  return DM_OK;
}

#include "host_request.hip.inc"

// Mask.scala:10 — scale = 1 / sqrt(embedSize) of the model as loaded (zero padding of the table does not change it)
static double sm_scale64(const dm_ctx *h) { return 1.0 / sqrt((double)(h->embed_log > 0 ? h->embed_log : h->embed)); }
static float sm_scale32(const dm_ctx *h) { return (float)sm_scale64(h); }

static int level_start_int(int candidate_num, int *start, int *level) {
  if (candidate_num <= 0) return DM_ERR_INVALID;
  int lv = 0;
  while ((2 << lv) <= candidate_num) lv++;   // floor(log2)
  *level = lv;
  *start = (1 << lv) - 1;
  return DM_OK;
}

// ------------------------------------------------------------------ C ABI
// (every dm_* below is declared extern "C" by include/dismember_hip.h)

int dm_version(void) { return DM_VERSION; }

int dm_device_count(int *count) {
  if (!count) return DM_ERR_INVALID;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; g_create_err = hipGetErrorString(e); return DM_ERR_HIP; }
  *count = n;
  return DM_OK;
}

const char *dm_last_error(dm_handle_t h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int dm_create(int device_id, dm_handle_t *out) {
  if (!out) return fail(nullptr, DM_ERR_INVALID, "dm_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, DM_ERR_HIP, std::string("dm_create: no HIP device available (") +
                                         (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                                         "); this library has no CPU fallback");
  if (device_id < 0 || device_id >= n) return fail(nullptr, DM_ERR_INVALID, "dm_create: device_id out of range");
  dm_ctx *h = new dm_ctx();
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess) { delete h; return fail(nullptr, DM_ERR_HIP, "hipSetDevice failed"); }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) { delete h; return fail(nullptr, DM_ERR_HIP, "hipGetDeviceProperties failed"); }
  h->n_cu = prop.multiProcessorCount;
  if (env_str("DM_BEAM_W")) h->beam_w = env_on("DM_BEAM_W");
  if (env_on("DM_NO_DIRECT")) h->direct_ok = false;
  if (env_on("DM_TIME_DIRECT")) h->time_direct = true;
  if (hipStreamCreate(&h->stream) != hipSuccess) { delete h; return fail(nullptr, DM_ERR_HIP, "hipStreamCreate failed"); }
  if (dm_alloc(h, (void **)&h->d_ctr, sizeof(SearchCounters)) != DM_OK) { delete h; return fail(nullptr, DM_ERR_HIP, "hipMalloc failed"); }
  (void)hipMemset(h->d_ctr, 0, sizeof(SearchCounters));
  if (dm_alloc(h, (void **)&h->d_phase, 128) == DM_OK) (void)hipMemset(h->d_phase, 0, 128);
  *out = h;
  return DM_OK;
}

static inline void model_changed(dm_ctx *h) { h->model_epoch.fetch_add(1); }
static int clone_enter(dm_ctx *c);
// entry points that evaluate DIN (after DM_CLONE_ENTER: a clone mirrors its owner's scorer): refused while a DeepFM model is loaded
static const char *scorer_name(const dm_ctx *h) { return h->scorer_kind == DM_KIND_DEEPFM ? "DeepFM" : "DIN"; }
#define DM_DIN_ONLY(h, who) do { if ((h)->scorer_kind != DM_KIND_DIN) return fail((h), DM_ERR_UNSUPPORTED, std::string(who) + ": the loaded scorer is " + scorer_name(h) + "; this entry point evaluates DIN (a DeepFM model serves dm_deepfm_forward and dm_tdm_beam_search*)"); } while (0)
// entry points that replace the model or train it: the owning handle only
#define DM_OWNER_ONLY(h, who) do { if ((h)->parent) return fail((h), DM_ERR_STATE, who ": not on a clone (dm_clone) - load and train through the owning handle"); } while (0)
// read-only entry points: a clone first brings its mirror of the parent's model up to date
#define DM_CLONE_ENTER(h) do { if ((h)->parent) { const int rc_ce_ = clone_enter(h); if (rc_ce_ != DM_OK) return rc_ce_; } } while (0)

static void free_tree(dm_ctx *h) {
  model_changed(h);
  dm_release(h->d_lv_codes, h->d_lv_cdf, h->d_lv_start, h->d_exists, h->d_leaf, h->d_node_id, h->d_leaf_codes, h->d_level_last);
  h->tree_loaded = false;
}
// the training state of dm_train_init: its buffers, and the flags that say they exist
static void free_training(dm_ctx *h) {
  h->train.release();
  dm_release(h->d_loss, h->d_tr64, h->d_attTA, h->d_w1aTA, h->d_w1bTA, h->d_touch_bits, h->d_touch_list, h->d_touch_cnt);
  h->train_ready = false; h->touch_cap = 0; h->touch_ub = 0;
}
static void dfm_train_release(dm_ctx *h);
static void dfm_otm_tree_release(dm_ctx *h);
static void free_weights(dm_ctx *h) {
  model_changed(h);
  dfm_train_release(h);
  dfm_otm_tree_release(h);
  if (h->emb32_owned) dm_release(h->d_emb32);
  h->d_emb32 = nullptr; h->emb32_owned = false;
  dm_release(h->d_compact, h->d_wfrag, h->d_afrag, h->d_bfrag, h->d_attA, h->d_w1aA, h->d_w1bA, h->d_b1, h->d_w2, h->d_att_wT_t, h->d_l1T_t);
  h->lazy.released();
  dm_release(h->d_dfm_frag, h->d_dfm_w2p, h->d_dfm_fragS, h->d_tail32);
  h->scorer_kind = DM_KIND_DIN; h->dfm_L = 0;
  free_training(h);
  h->w_loaded = false;
}

// Everything a clone mirrors from its parent: the tree, the id maps, the weights and every derived copy (fragment orders, split planes,
// the pre-split table, the f32 mirror of an f64 model, the fp64 fragments).  One list drives the mirror and the clone's tear-down.
#define DM_SHARED_FIELDS(X)                                                                                                              \
  X(tree_loaded) X(ids_loaded) X(leaves_at_max_only) X(max_level) X(n_slots) X(n_leaf_nodes) X(d_exists) X(d_leaf) X(d_node_id)          \
  X(d_level_last) X(level_last)                                                                                                          \
  X(d_id_to_code) X(d_leaf_codes) X(non_leaf_offset) X(max_code) X(w_loaded) X(dtype) X(embed) X(embed_log) X(num_index) X(d_compact)    \
  X(d_emb32) X(d_wfrag) X(d_afrag) X(d_bfrag) X(d_attA) X(d_w1aA) X(d_w1bA) X(d_b1) X(d_w2) X(b2) X(d_att_wT_t) X(d_l1T_t) X(d_tail32)   \
  X(lazy) X(d_lv_codes) X(d_lv_cdf) X(d_lv_start) X(scorer_kind) X(dfm_L) X(d_dfm_frag) X(d_dfm_w2p) X(d_dfm_fragS)

static void clone_mirror(dm_ctx *c, dm_ctx *p) {
#define X(f) c->f = p->f;
  DM_SHARED_FIELDS(X)
#undef X
  if (c->seen_ids_epoch != p->ids_epoch || c->h_exists.size() != p->h_exists.size()) {      // (host vectors: O(catalogue), copied when the tree / id maps changed, not after every Adam step)
    c->h_id_to_code = p->h_id_to_code;
    c->h_exists = p->h_exists;
    c->seen_ids_epoch = p->ids_epoch;
  }
  c->emb32_owned = false;
  c->lazy.clone_view();
  c->seen_epoch = p->model_epoch.load();
}
static void clone_forget(dm_ctx *c) {         // the clone owns none of it
  dm_ctx z;
#define X(f) c->f = z.f;
  DM_SHARED_FIELDS(X)
#undef X
  c->emb32_owned = false;
}

static void jtm_drop_cache(dm_ctx *h);
int dm_destroy(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  if (h->n_clones.load() > 0) return fail(h, DM_ERR_STATE, "dm_destroy: the handle still has clones (dm_clone): destroy them first");
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->parent) { clone_forget(h); h->parent->n_clones.fetch_sub(1); h->parent = nullptr; }
  free_tree(h); free_weights(h); dm_dr_free(h->dr);
  dm_release(h->d_id_to_code, h->d_ctr, h->d_phase);
  for (DevGrow *g : {&h->ws, &h->req, &h->sync, &h->samp, &h->defer, &h->scratch64, &h->dfm_jtm_ws, &h->dra, &h->dra_io}) g->release();
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  jtm_drop_cache(h);
  for (auto &pr : h->ev_pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (auto &e_ : h->chunk_ev) (void)hipEventDestroy(e_);
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return DM_OK;
}

int dm_synchronize(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_level_start(int candidate_num, int *start_code, int *level) {
  if (!start_code || !level) return DM_ERR_INVALID;
  return level_start_int(candidate_num, start_code, level);
}

// Per-level existence bounds of the bitmap `ex` over codes [0, n_slots): out[l], l = 0 .. DM_N_LEVEL_BOUNDS - 1, is the largest
// existing code of level l when the level's existing codes are exactly the prefix [2^l - 1, last] of its code range (every
// left-filled heap, TreeBuilder's trees among them), 2^l - 2 when the level holds no node, and DM_LEVEL_USE_BITS when the level has
// a gap.  With a bound, "code c of level l exists" is c <= out[l]: a compare against a number that holds while the tree is loaded.
static void dm_level_bounds_bits(const uint32_t *ex, int64_t n_slots, int32_t *out) {
  for (int l = 0; l < DM_N_LEVEL_BOUNDS; l++) {
    const int64_t first = ((int64_t)1 << l) - 1, end = std::min<int64_t>(2 * first + 1, n_slots);
    if (l > 30) { out[l] = DM_LEVEL_USE_BITS; continue; }          // (no int32 code lives there)
    int64_t count = 0, last = first - 1;
    for (int64_t c = first; c < end;) {
      const uint32_t w = ex[c >> 5] >> (c & 31);
      const int span = (int)std::min<int64_t>(32 - (c & 31), end - c);
      const uint32_t m = span == 32 ? w : (w & ((1u << span) - 1u));
      if (m) { count += __builtin_popcount(m); last = c + 31 - __builtin_clz(m); }
      c += span;
    }
    out[l] = count == 0 ? (int32_t)(first - 1) : count == last - first + 1 ? (int32_t)last : DM_LEVEL_USE_BITS;
  }
}
// debug (not part of the public header): the bounds of a list of node codes, without a handle or a device
extern "C" int dm_debug_level_bounds(const int32_t *codes, int64_t n_nodes, int32_t *out) {
  if (!codes || !out || n_nodes < 0) return DM_ERR_INVALID;
  int64_t mc = -1;
  for (int64_t i = 0; i < n_nodes; i++) {
    if (codes[i] < 0) return DM_ERR_INVALID;
    if (codes[i] > mc) mc = codes[i];
  }
  std::vector<uint32_t> ex((size_t)((mc + 1 + 31) / 32 + 1), 0);
  for (int64_t i = 0; i < n_nodes; i++) ex[(size_t)(codes[i] >> 5)] |= 1u << (codes[i] & 31);
  dm_level_bounds_bits(ex.data(), mc + 1, out);
  return DM_OK;
}

int dm_load_tree_tdm(dm_handle_t h, const int32_t *codes, const int32_t *node_ids, const uint8_t *is_leaf,
                     int64_t n_nodes, int max_level) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_tree_tdm");
  if (!codes || !node_ids || !is_leaf || n_nodes <= 0 || max_level < 0 || max_level > 30)
    return fail(h, DM_ERR_INVALID, "dm_load_tree_tdm: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  int64_t mc = -1;
  for (int64_t i = 0; i < n_nodes; i++) {
    if (codes[i] < 0) return fail(h, DM_ERR_INVALID, "dm_load_tree_tdm: negative code");
    if (codes[i] > mc) mc = codes[i];
  }
  const int64_t n_slots = mc + 1;
  const int64_t words = (n_slots + 31) / 32 + 1;
  std::vector<uint32_t> ex(words, 0), lf(words, 0);
  std::vector<int32_t> nid(n_slots, 0), leaf_codes;
  bool at_max_only = true;
  const int64_t first_max = ((int64_t)1 << max_level) - 1;
  for (int64_t i = 0; i < n_nodes; i++) {
    int64_t c = codes[i];
    ex[c >> 5] |= 1u << (c & 31);
    nid[c] = node_ids[i];
    if (is_leaf[i]) { lf[c >> 5] |= 1u << (c & 31); leaf_codes.push_back((int32_t)c); if (c < first_max) at_max_only = false; }
    else if (c >= first_max) at_max_only = false;   // a non-leaf on the last level: take the general path
  }
  free_tree(h);
  ALLOC(h, h->d_exists, words * 4);
  ALLOC(h, h->d_leaf, words * 4);
  ALLOC(h, h->d_node_id, n_slots * 4);
  ALLOC(h, h->d_leaf_codes, leaf_codes.size() * 4);
  ALLOC(h, h->d_level_last, DM_N_LEVEL_BOUNDS * 4);
  dm_level_bounds_bits(ex.data(), n_slots, h->level_last.data());
  HIPCHK(h, hipMemcpy(h->d_level_last, h->level_last.data(), DM_N_LEVEL_BOUNDS * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_exists, ex.data(), words * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_leaf, lf.data(), words * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_node_id, nid.data(), n_slots * 4, hipMemcpyHostToDevice));
  if (!leaf_codes.empty())
    HIPCHK(h, hipMemcpy(h->d_leaf_codes, leaf_codes.data(), leaf_codes.size() * 4, hipMemcpyHostToDevice));
  h->h_exists = ex;
  h->ids_epoch++;              // (clones re-copy their host vectors; per-row code caches built against the old tree are dropped)
  h->n_slots = n_slots; h->n_leaf_nodes = (int64_t)leaf_codes.size(); h->max_level = max_level;
  h->leaves_at_max_only = at_max_only; h->tree_loaded = true;
  return DM_OK;
}

int dm_load_id_maps(dm_handle_t h, const int32_t *leaf_item_ids, const int32_t *leaf_codes, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_id_maps");
  if (!leaf_item_ids || !leaf_codes || n <= 0) return fail(h, DM_ERR_INVALID, "dm_load_id_maps: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  int32_t mid = -1, mcode = -1;
  for (int64_t i = 0; i < n; i++) {
    if (leaf_item_ids[i] > mid) mid = leaf_item_ids[i];
    if (leaf_codes[i] > mcode) mcode = leaf_codes[i];
  }
  if (mid < 0) return fail(h, DM_ERR_INVALID, "dm_load_id_maps: no non-negative item id");
  model_changed(h);
  h->ids_epoch++;
  h->non_leaf_offset = mid + 1;   // DistTree.scala:35
  h->max_code = mcode;            // DistTree.scala:36
  h->h_id_to_code.assign((size_t)h->non_leaf_offset, -1);
  for (int64_t i = 0; i < n; i++)
    if (leaf_item_ids[i] >= 0) h->h_id_to_code[leaf_item_ids[i]] = leaf_codes[i];
  dm_release(h->d_id_to_code);
  ALLOC(h, h->d_id_to_code, h->h_id_to_code.size() * 4);
  HIPCHK(h, hipMemcpy(h->d_id_to_code, h->h_id_to_code.data(), h->h_id_to_code.size() * 4, hipMemcpyHostToDevice));
  h->ids_loaded = true;
  return DM_OK;
}

int dm_tdm_id_to_code(dm_handle_t h, const int32_t *item_ids, int n, int32_t *codes, int32_t *mask_pos, int *n_mask) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!h->ids_loaded) return fail(h, DM_ERR_STATE, "dm_tdm_id_to_code: id maps not loaded");
  if (!item_ids || !codes || !mask_pos || !n_mask || n < 0) return fail(h, DM_ERR_INVALID, "dm_tdm_id_to_code: bad arguments");
  int nm = 0;
  for (int i = 0; i < n; i++) {
    int32_t id = item_ids[i];
    if (id == 0) { mask_pos[nm++] = i; codes[i] = -1; }
    else if (id < h->non_leaf_offset && id >= 0 && h->h_id_to_code[id] >= 0) codes[i] = h->h_id_to_code[id];
    else {
      int32_t t = (int32_t)((uint32_t)id - (uint32_t)h->non_leaf_offset);
      if (t > h->max_code) { mask_pos[nm++] = i; codes[i] = -1; } else codes[i] = t;
    }
  }
  *n_mask = nm;
  return DM_OK;
}

// Embedding sizes the kernels are built for; any other size up to 128 is zero-padded to the next one at load (S/nn/Attention.scala,
// T/model/DIN.scala take any embedSize).  Zero columns / rows change no product: q.k, att.W k, W1 [q ; att] and w2 . h keep their
// values, the padded hidden units are relu(0) = 0, and training leaves the padding at zero (its gradients are products with zero
// inputs; Adam moves a parameter whose gradient history is zero by 0 / (0 + eps)).  Only the softmax scale 1 / sqrt(embedSize)
// (Mask.scala:10) must stay the model's: sm_scale64().
static int native_embed(int E) { return E <= 0 ? 0 : E <= 16 ? 16 : E <= 32 ? 32 : E <= 64 ? 64 : E <= 128 ? 128 : 0; }
static int64_t compact_len_for(int64_t num_index, int64_t E) { return num_index * E + 3 * E * E + 2 * E + 1; }

template <typename T>
static void pad_compact(const T *src, int E, int Ep, int64_t NI, T *dst) {       // dst: compact_len_for(NI, Ep) elements, zeroed here
  memset(dst, 0, (size_t)compact_len_for(NI, Ep) * sizeof(T));
  for (int64_t r = 0; r < NI; r++) memcpy(dst + r * Ep, src + r * E, (size_t)E * sizeof(T));
  const T *s_att = src + NI * E, *s_l1 = s_att + (int64_t)E * E, *s_b1 = s_l1 + (int64_t)E * 2 * E, *s_w2 = s_b1 + E;
  T *d_att = dst + NI * Ep, *d_l1 = d_att + (int64_t)Ep * Ep, *d_b1 = d_l1 + (int64_t)Ep * 2 * Ep, *d_w2 = d_b1 + Ep;
  for (int o = 0; o < E; o++) {
    memcpy(d_att + (int64_t)o * Ep, s_att + (int64_t)o * E, (size_t)E * sizeof(T));
    memcpy(d_l1 + (int64_t)o * 2 * Ep, s_l1 + (int64_t)o * 2 * E, (size_t)E * sizeof(T));                  // W1a half
    memcpy(d_l1 + (int64_t)o * 2 * Ep + Ep, s_l1 + (int64_t)o * 2 * E + E, (size_t)E * sizeof(T));        // W1b half
  }
  memcpy(d_b1, s_b1, (size_t)E * sizeof(T));
  memcpy(d_w2, s_w2, (size_t)E * sizeof(T));
  d_w2[Ep] = s_w2[E];
}
template <typename T>
static void unpad_compact(const T *src, int E, int Ep, int64_t NI, T *dst) {     // src padded, dst: compact_len_for(NI, E) elements
  for (int64_t r = 0; r < NI; r++) memcpy(dst + r * E, src + r * Ep, (size_t)E * sizeof(T));
  const T *s_att = src + NI * Ep, *s_l1 = s_att + (int64_t)Ep * Ep, *s_b1 = s_l1 + (int64_t)Ep * 2 * Ep, *s_w2 = s_b1 + Ep;
  T *d_att = dst + NI * E, *d_l1 = d_att + (int64_t)E * E, *d_b1 = d_l1 + (int64_t)E * 2 * E, *d_w2 = d_b1 + E;
  for (int o = 0; o < E; o++) {
    memcpy(d_att + (int64_t)o * E, s_att + (int64_t)o * Ep, (size_t)E * sizeof(T));
    memcpy(d_l1 + (int64_t)o * 2 * E, s_l1 + (int64_t)o * 2 * Ep, (size_t)E * sizeof(T));
    memcpy(d_l1 + (int64_t)o * 2 * E + E, s_l1 + (int64_t)o * 2 * Ep + Ep, (size_t)E * sizeof(T));
  }
  memcpy(d_b1, s_b1, (size_t)E * sizeof(T));
  memcpy(d_w2, s_w2, (size_t)E * sizeof(T));
  d_w2[E] = s_w2[Ep];
}

#include "model_weights.hip.inc"
#define DM_LAZY_COPIES_PART 2      // predicates, build kernels, ensure_*
#include "lazy_copies.hip.inc"

// A clone's read-only entry points start here.  Fast path: the parent's model has not changed since the mirror was taken (one atomic
// load).  Otherwise, under the parent's lock: the copies this clone's scorer needs are brought up to date ON THE PARENT (its stream,
// its buffers; no-ops when clean), the parent's stream is drained, and the mirror is retaken.  Weight updates through the parent must
// not overlap a clone's search in flight — the reference's workers wait for each other the same way (LocalOptimizer.scala:73-80).
static int clone_enter(dm_ctx *c) {
  dm_ctx *p = c->parent;
  if (c->seen_epoch == p->model_epoch.load()) return DM_OK;
  std::lock_guard<std::recursive_mutex> lock(p->mu);
  if (hipSetDevice(p->device) != hipSuccess) return fail(c, DM_ERR_HIP, "dm_clone: hipSetDevice failed");
  for (int pass = 0; pass < 2; pass++) {
    clone_mirror(c, p);                         // (first pass: the model's shape, so that the scorer choice below is this clone's)
    if (!p->w_loaded) break;
    if (p->scorer_kind == DM_KIND_DEEPFM) {      // no lazily rebuilt copies: what dm_load_weights_deepfm made is all there is
      if (hipStreamSynchronize(p->stream) != hipSuccess) return fail(c, DM_ERR_HIP, "dm_clone: the parent's stream failed");
      break;
    }
    int rc = DM_OK;
    if (use_f64_beam(c)) rc = ensure_frags64(p);        // (decided on the clone: the parent's model with the clone's own scorer setting)
    else {
      rc = ensure_f32_mirror(p);
      if (rc == DM_OK && use_split(c)) { rc = ensure_split(p); if (rc == DM_OK) rc = ensure_rows_split(p); }
    }
    if (rc != DM_OK) { c->err = p->err; return rc; }
    if (hipStreamSynchronize(p->stream) != hipSuccess) return fail(c, DM_ERR_HIP, "dm_clone: the parent's stream failed");
  }
  return DM_OK;
}

int dm_clone(dm_handle_t h, dm_handle_t *out) {
  if (!h || !out) return DM_ERR_INVALID;
  *out = nullptr;
  dm_ctx *root = h->parent ? h->parent : h;      // a clone of a clone shares the same owner
  dm_handle_t c = nullptr;
  int rc = dm_create(root->device, &c);
  if (rc != DM_OK) return fail(h, rc, g_create_err);
  c->parent = root;
  c->scorer_mode = h->scorer_mode;
  root->n_clones.fetch_add(1);
  rc = clone_enter(c);
  if (rc != DM_OK) { h->err = c->err; root->n_clones.fetch_sub(1); c->parent = nullptr; dm_destroy(c); return rc; }
  *out = c;
  return DM_OK;
}

template <typename T>
__global__ void dm_fill_normal_kernel(T *out, int64_t n, float mean, float std, unsigned long long seed) {
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
  for (; i < n; i += stride) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i / 2 + 1);   // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u1 = ((float)(unsigned)(z >> 40) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
    const float u2 = (float)(unsigned)((z >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.2831853071795864f * u2, &sn, &cs);
    out[i] = (T)(mean + std * r * cs);            // the f64 fill holds the f32 values, widened
    if (i + 1 < n) out[i + 1] = (T)(mean + std * r * sn);
  }
}

__global__ void dm_fill_tree_level_kernel(float *emb, int E, int64_t first, int64_t count, float rho, float sd, unsigned long long seed) {
  // one thread per PAIR of floats of the level's rows; row c = rho * row(parent) + sd * noise
  const int64_t n2 = count * E / 2;
  const float cn = sqrtf(1.0f - rho * rho);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n2; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = first + (2 * t) / E;
    const int e = (int)((2 * t) % E);
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(row * (E / 2) + e / 2 + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u1 = ((float)(unsigned)(z >> 40) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(unsigned)((z >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.2831853071795864f * u2, &sn, &cs);
    float p0 = 0.f, p1 = 0.f, c = 1.0f;
    if (row > 0) { const int64_t par = (row - 1) >> 1; p0 = emb[par * E + e]; p1 = emb[par * E + e + 1]; c = cn; }
    emb[row * E + e] = rho * p0 + c * sd * r * cs;
    emb[row * E + e + 1] = rho * p1 + c * sd * r * sn;
  }
}

int dm_fill_tree_normal(dm_handle_t h, float *d_emb, int E, int depth, float rho, float std, uint64_t seed) {
  if (!h) return DM_ERR_INVALID;
  if (!d_emb || E <= 0 || (E & 1) || depth < 0 || depth > 30 || rho < 0.f || rho >= 1.f) return fail(h, DM_ERR_INVALID, "dm_fill_tree_normal: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  for (int l = 0; l <= depth; l++) {
    const int64_t first = ((int64_t)1 << l) - 1, count = (int64_t)1 << l;
    int64_t blocks = (count * E / 2 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    const int rc = LAUNCH(h, dm_fill_tree_level_kernel, dim3((unsigned)blocks), dim3(256), 0, d_emb, E, first, count, rho, std, seed);
    if (rc != DM_OK) return rc;
  }
  return DM_OK;
}

int dm_fill_normal(dm_handle_t h, float *d_ptr, int64_t n, float mean, float std, uint64_t seed) {
  if (!h) return DM_ERR_INVALID;
  if (!d_ptr || n < 0) return fail(h, DM_ERR_INVALID, "dm_fill_normal: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  if (n == 0) return DM_OK;
  return LAUNCH(h, dm_fill_normal_kernel<float>, dim3(4096), dim3(256), 0, d_ptr, n, mean, std, seed);
}

int dm_fill_normal_f64(dm_handle_t h, double *d_ptr, int64_t n, float mean, float std, uint64_t seed) {
  if (!h) return DM_ERR_INVALID;
  if (!d_ptr || n < 0) return fail(h, DM_ERR_INVALID, "dm_fill_normal_f64: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  if (n == 0) return DM_OK;
  return LAUNCH(h, dm_fill_normal_kernel<double>, dim3(4096), dim3(256), 0, d_ptr, n, mean, std, seed);
}

static bool fwd64_ready(dm_ctx *h, int L);                 // train_host.hip.inc
static int rows_fwd64(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const unsigned *d_rowmask, int64_t B, int L, double *d_out);
template <typename T>
static int din_forward_t(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const unsigned *d_rowmask, int64_t B,
                         int L, T *d_out, int64_t B_request = 0) {
  // B_request > 0: these B rows are one chunk of a request of that many rows, and the kernel is chosen for the REQUEST: the two f64 kernels
  // round differently, and a result must not depend on where the caller's chunks end (dm_otm_child_weights)
  if constexpr (sizeof(T) == 8) {
    // f64 models, batches of rows: the matrix-pipe forward (train_host.hip.inc: rows_fwd64 — the training kernel's forward half on
    // v_mfma_f64_16x16x4_f64) instead of the one-wave-per-row kernel below, which stays for single rows and for clones
    // (round 6: 34 M rows/s -> 10x; dm_din_forward, OTM child weights, evaluators).  DM_FWD64_SCALAR=1 keeps the scalar kernel.
    static const bool scalar_only = env_on("DM_FWD64_SCALAR");
    if (!scalar_only && (B_request > 0 ? B_request : B) >= 256 && fwd64_ready(h, L)) return rows_fwd64(h, d_codes, d_seqs, d_rowmask, B, L, (double *)d_out);
  }
  DinFwdParams<T> p;
  const T *base = (const T *)h->d_compact;
  const int E = h->embed;
  p.emb = base; p.att_wT = (const T *)h->d_att_wT_t; p.l1T = (const T *)h->d_l1T_t;
  const T *l1_b = base + h->num_index * E + (int64_t)E * E + (int64_t)E * 2 * E;
  p.b1 = l1_b; p.w2 = l1_b + E;
  T b2;
  HIPCHK(h, hipMemcpy(&b2, l1_b + 2 * E, sizeof(T), hipMemcpyDeviceToHost));
  p.b2 = b2; p.E = E; p.L = L; p.B = B; p.codes = d_codes; p.seqs = d_seqs; p.rowmask = d_rowmask; p.out = d_out;
  p.sm_scale = (T)sm_scale64(h);
  int64_t blocks = (B + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  size_t lds = (size_t)4 * (3 * E + 32) * sizeof(T);
  return LAUNCH(h, dm_din_forward_kernel<T>, dim3((unsigned)blocks), dim3(256), lds, p);
}

template <int E>
static int launch_rows_E(dm_ctx *h, const RowsParams &p) {
  const int lds = 2 * E * E * 4;
  int64_t tiles = (p.B + 15) / 16;
  int64_t blocks = (tiles + DM_NWAVES - 1) / DM_NWAVES;
  if (blocks > h->n_cu) blocks = h->n_cu;
  if (blocks < 1) blocks = 1;
  return LAUNCH_LDS(h, dm_din_rows_kernel<E>, dim3((unsigned)blocks), dim3(DM_BLOCK), lds, p);
}

// the two launches below: an event pair of kind 30 around a general-rows launch (dm_kernel_timing_get_kind: the roofline of JTM's scorer
// in bench.py)
template <int E, int LC>
static int launch_rows_split_EL(dm_ctx *h, const RowsSplitParams &p, int64_t blocks) {
  const int lds = 4 * E * E * 2 + DM_NWAVES * 2 * (DM_MAXL + 2) * 16 * 4 + 2 * E * 4;      // weight planes + the per-wave index staging + b1, w2
  HIPCHK(h, lds_opt_in(dm_din_rows_split_l_kernel<E, LC>, lds));      // (a host call: ahead of the event pair, not inside it)
  return timed(h, EV_ROWS, true, [&] { return LAUNCH(h, (dm_din_rows_split_l_kernel<E, LC>), dim3((unsigned)blocks), dim3(DM_BLOCK), lds, p); });
}

// History lengths with a counted-load instance (rows_kernel.hip.inc: dm_din_rows_split_l_kernel); every other length takes the generic
// kernel — the same arithmetic in the same order, bit-identical results (tests/test_gpu_precision.py).  DM_ROWS_GENERIC=1 forces it.
template <int E>
static int launch_rows_split_E(dm_ctx *h, const RowsSplitParams &p) {
  int64_t tiles = (p.B + 15) / 16;
  int64_t blocks = (tiles + DM_NWAVES - 1) / DM_NWAVES;
  if (blocks > h->n_cu) blocks = h->n_cu;
  if (blocks < 1) blocks = 1;
  static const bool generic_only = env_on("DM_ROWS_GENERIC");
  if (!generic_only) {
    switch (p.L) {
      case 8: return launch_rows_split_EL<E, 8>(h, p, blocks);
      case 10: return launch_rows_split_EL<E, 10>(h, p, blocks);
      case 16: return launch_rows_split_EL<E, 16>(h, p, blocks);
      default: break;
    }
  }
  const int lds = 4 * E * E * 2;
  HIPCHK(h, lds_opt_in(dm_din_rows_split_kernel<E>, lds));
  return timed(h, EV_ROWS, true, [&] { return LAUNCH(h, dm_din_rows_split_kernel<E>, dim3((unsigned)blocks), dim3(DM_BLOCK), lds, p); });
}

// f32 general-rows forward on device buffers (asynchronous on the handle's stream)
static int din_rows_dev(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const unsigned *d_rowmask, int64_t B,
                        int L, float *d_out, int seq_div = 1) {
  // the default arithmetic for E = 32 / 64 / 128 (DM_SCORER_F32 keeps the fp32-input kernel below).  While a training loop keeps
  // moving the weights (AUTO mode) a batch below ~4 M rows is cheaper on the fp32-input kernel than the table scan for the new scale.
  if (use_split(h) && !(weights_in_motion(h) && B < ((int64_t)1 << 22))) {
    int rc = ensure_rows_split(h);
    if (rc != DM_OK) return rc;
    RowsSplitParams q;
    q.emb = h->d_emb32; q.planes = (const dm_h8 *)h->lazy.d_rows_split; q.b1 = h->d_b1; q.w2 = h->d_w2; q.b2 = h->b2;
    q.emb_scale = ldexpf(1.0f, h->lazy.sh_e); q.out_unscale = ldexpf(1.0f, -(h->lazy.sh_e + h->lazy.sh_r));
    q.num_index = h->num_index; q.codes = d_codes; q.seqs = d_seqs; q.rowmask = d_rowmask; q.B = B; q.L = L; q.out = d_out;
    q.sm_scale = sm_scale32(h); q.seq_div = seq_div;
    return dispatch_E<32>(h, h->embed, "unsupported embed size", [&](auto e) { return launch_rows_split_E<decltype(e)::value>(h, q); });
  }
  RowsParams p;
  p.emb = h->d_emb32; p.attA = h->d_attA; p.w1aA = h->d_w1aA; p.w1bA = h->d_w1bA; p.b1 = h->d_b1; p.w2 = h->d_w2;
  p.b2 = h->b2; p.num_index = h->num_index; p.codes = d_codes; p.seqs = d_seqs; p.rowmask = d_rowmask; p.B = B; p.L = L;
  p.out = d_out; p.sm_scale = sm_scale32(h); p.seq_div = seq_div;
  return dispatch_E(h, h->embed, "unsupported embed size", [&](auto e) { return launch_rows_E<decltype(e)::value>(h, p); });
}

int dm_din_forward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, const int32_t *pad_flat_idx,
                   int64_t n_pad, int64_t B, int L, void *logits) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, "dm_din_forward: weights not loaded");
  DM_DIN_ONLY(h, "dm_din_forward");
  if (!codes || !seqs || !logits || B < 0 || L <= 0 || L > 32 || n_pad < 0 || (n_pad > 0 && !pad_flat_idx))
    return fail(h, DM_ERR_INVALID, "dm_din_forward: bad arguments (L must be 1..32)");
  if (B == 0) return DM_OK;
  int rc;
  if ((rc = check_lookup_ids(h, codes, B, 1, "row")) != DM_OK || (rc = check_lookup_ids(h, seqs, B * L, L, "row")) != DM_OK) return rc;
  for (int64_t i = 0; i < n_pad; i++)
    if (pad_flat_idx[i] < 0 || pad_flat_idx[i] >= B * L) return fail(h, DM_ERR_INDEX, "dm_din_forward: mask index outside [0, B*L)");
  HIPCHK(h, hipSetDevice(h->device));
  int32_t *d_codes = nullptr, *d_seqs = nullptr, *d_pad = nullptr;
  unsigned *d_mask = nullptr;
  void *d_out = nullptr;
  const size_t esz = h->dtype == DM_F32 ? 4 : 8;
  DevTemps t(h);
  if ((rc = t.alloc(d_codes, B * 4)) != DM_OK || (rc = t.alloc(d_seqs, B * L * 4)) != DM_OK || (rc = t.alloc(d_mask, B * 4)) != DM_OK ||
      (rc = t.alloc(d_out, B * esz)) != DM_OK) return rc;
  if (hipMemcpyAsync(d_codes, codes, B * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(d_seqs, seqs, B * L * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemsetAsync(d_mask, 0, B * 4, h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, "dm_din_forward: upload failed");
  if (n_pad > 0) {
    if (t.alloc(d_pad, n_pad * 4) != DM_OK) return DM_ERR_HIP;
    if (hipMemcpyAsync(d_pad, pad_flat_idx, n_pad * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, "upload failed");
    if ((rc = LAUNCH(h, dm_pad_rowmask_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, d_pad, n_pad, L, d_mask)) != DM_OK) return rc;
  }
  rc = h->dtype == DM_F32 ? (L <= DM_MAXL ? din_rows_dev(h, d_codes, d_seqs, d_mask, B, L, (float *)d_out)
                                          : din_forward_t<float>(h, d_codes, d_seqs, d_mask, B, L, (float *)d_out))
                          : din_forward_t<double>(h, d_codes, d_seqs, d_mask, B, L, (double *)d_out);
  if (rc != DM_OK) return rc;
  if (hipMemcpyAsync(logits, d_out, B * esz, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, std::string("dm_din_forward: ") + hipGetErrorString(hipGetLastError()));
  return DM_OK;
}

// ------------------------------------------------------------ beam search
struct SearchPlan {
  int nteams, cap, pcap, grid, ws_cap, lds;
  bool wkernel = false;        // the one-wave-per-SIMD kernel with W1a in the AccVGPRs (beam_kernel_w.hip.inc)
  bool split = false;          // scorer arithmetic of this search: the split-fp16 copies (split_for_call) or the fp32 inputs
  int ev_kind = EV_MAIN;       // what its launch is recorded as; only EV_MAIN names the search's kernel (dm_last_beam_kernel)
};

// AUTO mode inside a training loop (weights_in_motion): a search small next to the split copies' refresh keeps the fp32-input kernel
static bool split_for_call(const dm_ctx *h, int64_t U, int max_beam) {
  if (!use_split(h)) return false;
  if (split_refresh_pending(h)) {
    const bool patchable = split_patchable(h);                       // only the Adam step's active rows are stale
    const double rows_ = (double)split_refresh_rows(h);
    const double rebuild_s = 3.0e-5 + 3.0 * rows_ * h->embed * 4 / (patchable ? 1.0e12 : 3.0e12);   // launches + read-back, then scan + read + write
    const double extra_s = (double)U * max_beam * 7.0e-9;                             // fp32-input kernel: ~7 ns more per (user, beam slot)
    if (extra_s < rebuild_s) return false;
  }
  return true;
}

// Histories of 17 .. 32 positions run inside the fused LDS-fed kernel (two key tiles, beam_kernel.hip.inc) whenever its frontier fits
// LDS beside the second key tile; the per-level pipelines (tdm_pipeline.hip.inc, otm64.hip.inc) remain for beams beyond that and for
// A/B runs (DM_LONG_PIPELINE=1).
static bool long_history_pipeline(const dm_ctx *h, int max_beam, int L) {
  if (L <= DM_MAXL) return false;
  if (env_on("DM_LONG_PIPELINE")) return true;          // read per call: the tests run both routes in one process
  int cap, pcap;
  frontier_caps(max_beam, &cap, &pcap);
  // (sized for the split scorer's layout; the fp32-input layout of the same request is no larger)
  return dm_beam_lds(h->embed, 1, cap, pcap, 4, true, 2).total > 160 * 1024;
}

// The LDS-fed kernel runs teams of 8 / nteams waves: the largest team count, halving from `from`, whose dm_beam_lds layout fits the
// 160 KB of a CU (*lds: that layout's size), or 0 when not even one team fits
static int beam_teams_that_fit(int E, int from, int cap, int pcap, int kq, bool split, int kt, int *lds) {
  for (int cand = from; cand >= 1; cand >>= 1) {
    const BeamLds l = dm_beam_lds(E, cand, cap, pcap, kq, split, kt);
    if (l.total <= 160 * 1024) { *lds = l.total; return cand; }
  }
  return 0;
}

static int plan_search(dm_ctx *h, int max_beam, int64_t U, int L, int n_levels, bool tdm, SearchPlan *pl) {
  int cap, pcap;
  frontier_caps(max_beam, &cap, &pcap);
  const int kt = L > DM_MAXL ? 2 : 1;          // histories of 17 .. 32 positions: the LDS-fed kernel's two-key-tile instance
  const int kq = kt > 1 ? 4 : (L + 3) / 4;
  int nteams = 0;
  *pl = SearchPlan{};
  pl->split = split_for_call(h, U, max_beam);
  if (pl->split && h->beam_w && kt == 1) {
    // split-fp16 scorer: one-wave teams, four per workgroup, W1a in registers; falls back when the frontier outgrows LDS
    BeamWLds l = dm_beamw_lds(h->embed, cap, pcap, kq);
    if (l.total <= 160 * 1024) { nteams = DMW_NWAVES; pl->lds = l.total; pl->wkernel = true; }
  }
  // LDS-fed kernel.  A frontier of at most 256 slots fits ONE wave's register sort, so small beams
  // (the reference's serving default is candidateNum 20) run as eight one-wave teams: no team barriers at all on the latency
  // chain sort -> expand -> gather -> score of a level, and eight users per CU in flight instead of four
  if (!nteams) nteams = beam_teams_that_fit(h->embed, pcap <= 256 ? 8 : 4, cap, pcap, kq, pl->split, kt, &pl->lds);
  if (!nteams) return fail(h, DM_ERR_UNSUPPORTED, "beam too large for the LDS frontier (about 2*beam*28 bytes + weights must fit 160 KiB)");
  int64_t groups = (U + nteams - 1) / nteams;
  int grid = (int)(groups < h->n_cu ? groups : h->n_cu);
  if (grid < 1) grid = 1;
  pl->nteams = nteams; pl->cap = cap; pl->pcap = pcap; pl->grid = grid;
  pl->ws_cap = tdm ? (h->leaves_at_max_only ? cap : cap * (n_levels + 1)) : 16;
  return DM_OK;
}

// The second pass of a search on the one-wave-per-SIMD kernel: the LDS-fed split kernel over the users the first pass deferred.  Its own
// frontier layout, from four teams down; the workspace was sized for the first pass's grid x 4 one-wave teams, and the second pass may
// use at most as many (block, team) slots.
static int plan_deferred_pass(dm_ctx *h, const SearchPlan &pl, int L, SearchPlan *pl2) {
  *pl2 = pl;
  pl2->wkernel = false;
  pl2->ev_kind = EV_DEFERRED;
  pl2->nteams = beam_teams_that_fit(h->embed, 4, pl.cap, pl.pcap, (L + 3) / 4, pl.split, 1, &pl2->lds);
  if (!pl2->nteams) return fail(h, DM_ERR_UNSUPPORTED, "beam too large for the LDS frontier");
  if (pl2->grid * pl2->nteams > pl.grid * pl.nteams) pl2->grid = pl.grid * pl.nteams / pl2->nteams;
  if (pl2->grid < 1) pl2->grid = 1;
  return DM_OK;
}

static int ensure_ws(dm_ctx *h, size_t bytes) {
  return h->ws.reserve(h, bytes);
}

template <int E, int KQ, bool SPLIT, int KT = 1>
static int launch_beam_EK(dm_ctx *h, const BeamParams &p_in, const SearchPlan &pl) {
  BeamParams p = p_in;
  p.static_users = (p.mode != 2 && !p.user_list && p.U <= (int64_t)pl.grid * pl.nteams) ? 1 : 0;
  if (pl.ev_kind == EV_MAIN) {
    if (KT == 1) snprintf(h->last_kernel, sizeof(h->last_kernel), "dm_beam_kernel<%d, %d, %s>", E, KQ, SPLIT ? "true" : "false");
    else snprintf(h->last_kernel, sizeof(h->last_kernel), "dm_beam_kernel<%d, %d, %s, %d>", E, KQ, SPLIT ? "true" : "false", KT);
  }
  HIPCHK(h, lds_opt_in(dm_beam_kernel<E, KQ, SPLIT, KT>, pl.lds));
  return timed(h, pl.ev_kind, !(p.host_direct && !h->time_direct), [&] {      // single-request path: the launch and nothing else
    return LAUNCH(h, (dm_beam_kernel<E, KQ, SPLIT, KT>), dim3(pl.grid), dim3(DM_BLOCK), pl.lds, p);
  });
}

// FOLD: the attention-combine product in one MFMA per feature tile — its three terms per history position fit the 32 contraction
// slots of v_mfma_f32_16x16x32_f16 exactly when 3 L <= 32 (beam_kernel_w.hip.inc, dmw_fold_slot)
template <int E, int KQ, bool FOLD>
static int launch_beam_w_EK(dm_ctx *h, const BeamParams &p, const SearchPlan &pl) {
  snprintf(h->last_kernel, sizeof(h->last_kernel), "dm_beam_w_kernel<%d, %d, %s>", E, KQ, FOLD ? "true" : "false");
  HIPCHK(h, lds_opt_in(dm_beam_w_kernel<E, KQ, FOLD>, pl.lds));
  return timed(h, EV_MAIN, true, [&] { return LAUNCH(h, (dm_beam_w_kernel<E, KQ, FOLD>), dim3(pl.grid), dim3(DMW_BLOCK), pl.lds, p); });
}
template <int E>
static int launch_beam_w_E(dm_ctx *h, const BeamParams &p, const SearchPlan &pl) {
  const bool fold = 3 * p.L <= 32;
  static_assert(3 * DMW_FOLD_MAXL <= 32 && 3 * (DMW_FOLD_MAXL + 1) > 32, "the slot map covers exactly the lengths that fold");
  switch ((p.L + 3) / 4) {
    case 1: return launch_beam_w_EK<E, 1, true>(h, p, pl);
    case 2: return launch_beam_w_EK<E, 2, true>(h, p, pl);
    case 3: return fold ? launch_beam_w_EK<E, 3, true>(h, p, pl) : launch_beam_w_EK<E, 3, false>(h, p, pl);
    default: return launch_beam_w_EK<E, 4, false>(h, p, pl);
  }
}

template <int E, bool SPLIT>
static int launch_beam_E(dm_ctx *h, const BeamParams &p, const SearchPlan &pl) {
  if (p.L > DM_MAXL) return launch_beam_EK<E, 4, SPLIT, 2>(h, p, pl);          // 17 .. 32 history positions: two key tiles
  switch ((p.L + 3) / 4) {
    case 1: return launch_beam_EK<E, 1, SPLIT>(h, p, pl);
    case 2: return launch_beam_EK<E, 2, SPLIT>(h, p, pl);
    case 3: return launch_beam_EK<E, 3, SPLIT>(h, p, pl);
    default: return launch_beam_EK<E, 4, SPLIT>(h, p, pl);
  }
}

static int launch_beam(dm_ctx *h, BeamParams &p, const SearchPlan &pl) {
  // the host-polled epilogue (results, system-scope fence, count as the flag) exists for the TDM final selection only: the mode-1 (OTM)
  // epilogue stores its counts before the ids and without a fence
  if (p.host_direct && p.mode != 0) return fail(h, DM_ERR_STATE, "launch_beam: the host-mapped single-request path is a mode-0 (TDM) path");
  h->last_g_table = false;
  {   // f64 model trained since the f32 copies were made: refresh them, then take b2 again (fill_common read it before the rebuild)
    const int rc_ = ensure_f32_mirror(h);
    if (rc_ != DM_OK) return rc_;
    p.b2 = h->b2;
  }
  // the brute-force recall oracle (mode 2) always scores with the fp32-input MFMA
  if (h->scorer_mode == DM_SCORER_SPLIT_F16 && h->embed % 32 != 0)
    return fail(h, DM_ERR_UNSUPPORTED, "the split-fp16 scorer needs an embedding size of 32, 64 or 128");
  if (pl.split && p.mode != 2) {
    int rc = ensure_split(h);
    if (rc != DM_OK) return rc;
    p.wsplit = (const dm_h8 *)h->lazy.d_wsplit;
    p.emb_split = (const dm_h8 *)h->lazy.d_emb_split;
    fill_split_scales(h, p);
    if (pl.wkernel) {
      // users the W kernel cannot score in fp16 throughout are queued in [count | next | ids ...] and scored by the LDS-fed kernel
      const size_t need = 16 + (size_t)p.U * 4;
      { const int rc_d = h->defer.reserve(h, need, need / 4); if (rc_d != DM_OK) return rc_d; }
      HIPCHK(h, hipMemsetAsync(h->defer.p, 0, 16, h->stream));
      p.defer_count = (unsigned long long *)h->defer.p;
      p.defer_users = (int32_t *)((char *)h->defer.p + 16);
      { const int rc_g = g_table_for_search(h, &p.g_table); if (rc_g != DM_OK) return rc_g; }
      // DM_LEVEL_BOUNDS (read per call, like DM_G_TABLE: the tests run both routes in one process) = 0: the existence tests of
      // the expand and of the initial frontier read the bitmap on every level; unset or 1: the per-level bounds where a level has one
      p.level_last = env_off("DM_LEVEL_BOUNDS") ? nullptr : h->d_level_last;
      h->last_g_table = p.g_table != nullptr;
      const char *const no_split = "the split-fp16 scorer needs an embedding size of 32, 64 or 128";
      int rc = dispatch_E<32>(h, h->embed, no_split, [&](auto e) { return launch_beam_w_E<decltype(e)::value>(h, p, pl); });
      if (rc != DM_OK) return rc;
      // second pass (an empty list costs one launch): same parameters, the list as the work queue, its own plan
      SearchPlan pl2;
      if ((rc = plan_deferred_pass(h, pl, p.L, &pl2)) != DM_OK) return rc;
      BeamParams p2 = p;
      p2.nteams = pl2.nteams;
      p2.user_count = (const unsigned long long *)h->defer.p;
      p2.user_list = (const int32_t *)((char *)h->defer.p + 16);
      p2.next_user = (unsigned long long *)((char *)h->defer.p + 8);
      p2.defer_count = nullptr; p2.defer_users = nullptr; p2.g_table = nullptr;      // (the LDS-fed kernel keeps its own setup)
      return dispatch_E<32>(h, h->embed, no_split, [&](auto e) { return launch_beam_E<decltype(e)::value, true>(h, p2, pl2); });
    }
    return dispatch_E<32>(h, h->embed, "the split-fp16 scorer needs an embedding size of 32, 64 or 128",
                          [&](auto e) { return launch_beam_E<decltype(e)::value, true>(h, p, pl); });
  }
  return dispatch_E(h, h->embed, "unsupported embed size", [&](auto e) { return launch_beam_E<decltype(e)::value, false>(h, p, pl); });
}

int dm_set_scorer_mode(dm_handle_t h, int mode) {
  if (!h) return DM_ERR_INVALID;
  if (mode != DM_SCORER_F32 && mode != DM_SCORER_SPLIT_F16 && mode != DM_SCORER_AUTO && mode != DM_SCORER_F64) return fail(h, DM_ERR_INVALID, "dm_set_scorer_mode: unknown mode");
  DM_DIN_ONLY(h, "dm_set_scorer_mode");      // (the DeepFM scorer has one arithmetic: fp32)
  if (mode == DM_SCORER_F64 && h->w_loaded && h->dtype != DM_F64)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_set_scorer_mode: the fp64 scorer needs f64 weights");
  if (mode == DM_SCORER_SPLIT_F16 && h->w_loaded && h->embed % 32 != 0)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_set_scorer_mode: the split-fp16 scorer needs an embedding size of 32, 64 or 128");
  h->scorer_mode = mode;
  if (h->parent) h->seen_epoch = 0;      // a clone: its next call makes sure the parent holds the copies this setting reads
  return DM_OK;
}

int dm_get_scorer_mode(dm_handle_t h, int *mode, int *effective, int *shift_emb, int *shift_w) {
  if (!h || !mode) return DM_ERR_INVALID;
  *mode = h->scorer_mode;
  if (effective) *effective = (h->w_loaded && use_f64_beam(h)) ? DM_SCORER_F64 : (h->w_loaded && use_split(h)) ? DM_SCORER_SPLIT_F16 : DM_SCORER_F32;
  if (shift_emb) *shift_emb = h->lazy.sh_e;
  if (shift_w) *shift_w = h->lazy.sh_w;
  return DM_OK;
}

static void fill_common(dm_ctx *h, BeamParams &p) {
  memset(&p, 0, sizeof p);
  p.emb = h->d_emb32; p.wfrag = h->d_wfrag; p.afrag = h->d_afrag; p.bfrag = h->d_bfrag; p.b1 = h->d_b1; p.w2 = h->d_w2;
  p.b2 = h->b2; p.num_index = h->num_index;
  p.exists_bits = h->d_exists; p.leaf_bits = h->d_leaf; p.node_id = h->d_node_id; p.id_to_code = h->d_id_to_code;
  p.n_slots = h->n_slots; p.non_leaf_offset = h->non_leaf_offset; p.max_code = h->max_code; p.max_level = h->max_level;
  p.scored_rows = &h->d_ctr->rows;
  p.sm_scale = sm_scale32(h);
  p.phase_cycles = h->d_phase;
  p.next_user = &h->d_ctr->queue_head;
}

// the frontier shape and its global-memory workspace (four arrays of grid x nteams x ws_cap words in h->ws), as the plan sized them
static int fill_frontier(dm_ctx *h, BeamParams &p, const SearchPlan &pl) {
  const size_t per = (size_t)pl.grid * pl.nteams * pl.ws_cap;
  const int rc = ensure_ws(h, per * 16);
  if (rc != DM_OK) return rc;
  p.nteams = pl.nteams; p.cap = pl.cap; p.pcap = pl.pcap;
  p.ws_code = (int32_t *)h->ws.p; p.ws_score = (float *)h->ws.p + per; p.ws_khi = (uint32_t *)h->ws.p + 2 * per;
  p.ws_klo = (uint32_t *)h->ws.p + 3 * per; p.ws_cap = pl.ws_cap;
  return DM_OK;
}

// before a search: the work-queue head restarts, and so does the scored-rows counter unless this search is a later chunk of one request
static hipError_t reset_search_counters(dm_ctx *h, bool keep_rows) {
  return keep_rows ? hipMemsetAsync(&h->d_ctr->queue_head, 0, sizeof h->d_ctr->queue_head, h->stream)
                   : hipMemsetAsync(h->d_ctr, 0, offsetof(SearchCounters, dr_slow), h->stream);      // rows + queue_head
}

// result rows before a search whose kernels write the live slots only: ids -1, scores 0 (score_bytes each), counts 0
static hipError_t prefill_results(dm_ctx *h, int64_t U, size_t stride, int32_t *d_ids, void *d_scores, size_t score_bytes, int32_t *d_counts) {
  hipError_t e = hipMemsetAsync(d_ids, 0xFF, (size_t)U * stride * 4, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_scores, 0, (size_t)U * stride * score_bytes, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, (size_t)U * 4, h->stream);
  return e;
}

static int tdm_pipeline_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, const dm_tdm_search_opts *o, int max_beam,
                            const int64_t *d_coff, const int32_t *d_cids, int32_t *d_ids, float *d_scores, int32_t *d_counts,
                            int trace_levels, int cap, int32_t *d_tc, float *d_ts, int32_t *d_tn);
static int dfm_pipeline_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, const dm_tdm_search_opts *o, int max_beam,
                            const int64_t *d_coff, const int32_t *d_cids, int32_t *d_ids, float *d_scores, int32_t *d_counts,
                            int trace_levels, int cap, int32_t *d_tc, float *d_ts, int32_t *d_tn);
// the searches that run level by level (tdm_pipeline.hip.inc) instead of inside one fused kernel: every search of a DeepFM model, and
// DIN histories of 17 .. 32 positions whose frontier does not fit LDS beside two key tiles
static bool level_pipeline(const dm_ctx *h, int max_beam, int L) {
  return h->scorer_kind == DM_KIND_DEEPFM || long_history_pipeline(h, max_beam, L);
}

static int tdm_search_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, const dm_tdm_search_opts *o, int max_beam,
                          const int64_t *d_coff, const int32_t *d_cids, int32_t *d_ids, float *d_scores, int32_t *d_counts,
                          int trace_levels, int32_t *d_tc, float *d_ts, int32_t *d_tn, bool keep_rows, bool *direct = nullptr) {
  if (!h->tree_loaded || !h->ids_loaded || !h->w_loaded) return fail(h, DM_ERR_STATE, "tdm beam search: tree, id maps and weights must be loaded first");
  if (U < 0 || L <= 0 || L > DM_PIPE_MAXL || !o || o->beam <= 0 || o->topk <= 0) return fail(h, DM_ERR_INVALID, "tdm beam search: bad arguments (L must be 1..32)");
  if (U == 0) return DM_OK;          // an empty batch is not an error
  if (h->n_slots > h->num_index) return fail(h, DM_ERR_INDEX, "tdm beam search: tree codes exceed the embedding table (embeddingLookup would fail)");
  if (h->max_code >= h->num_index) return fail(h, DM_ERR_INDEX, "tdm beam search: id map codes exceed the embedding table");
  const bool dfm = h->scorer_kind == DM_KIND_DEEPFM;
  if (dfm && o->use_mask) return fail(h, DM_ERR_INVALID, "tdm beam search: DeepFM has no mask (TDM.scala:26-29): use_mask must be 0");
  if (dfm && L != h->dfm_L) return fail(h, DM_ERR_INVALID, "tdm beam search: L = " + std::to_string(L) + " but the DeepFM model was built for seq_len " + std::to_string(h->dfm_L));
  if (level_pipeline(h, max_beam, L)) {
    if (direct) { *direct = false; return DM_OK; }          // (the caller takes the staged path and comes back)
    HIPCHK(h, prefill_results(h, U, o->topk, d_ids, d_scores, 4, d_counts));
    int cap_;
    frontier_caps(max_beam, &cap_, nullptr);
    return (dfm ? dfm_pipeline_dev : tdm_pipeline_dev)(h, d_seq, U, L, o, max_beam, d_coff, d_cids, d_ids, d_scores, d_counts, trace_levels, cap_, d_tc, d_ts, d_tn);
  }
  int start, level;
  level_start_int(o->beam, &start, &level);
  int n_levels = h->max_level - level + 1;
  if (n_levels < 0) n_levels = 0;
  SearchPlan pl;
  int rc = plan_search(h, max_beam, U, L, n_levels, true, &pl);
  if (rc != DM_OK) return rc;
  BeamParams p;
  fill_common(h, p);
  if ((rc = fill_frontier(h, p, pl)) != DM_OK) return rc;
  p.seq = d_seq; p.U = U; p.L = L; p.use_mask = o->use_mask; p.beam = o->beam; p.topk = o->topk;
  p.widen = (o->widen_consumed && d_coff) ? 1 : 0;
  p.consumed_off = d_coff; p.consumed_ids = d_cids; p.mode = 0; p.leaf_fast = h->leaves_at_max_only ? 1 : 0;
  p.out_ids = d_ids; p.out_scores = d_scores; p.out_counts = d_counts; p.out_stride = o->topk;
  p.trace_codes = d_tc; p.trace_scores = d_ts; p.trace_counts = d_tn; p.trace_levels = trace_levels;
  if (direct) {
    // single-request path (tdm_search_host): request and results live in host-mapped pinned memory, one team per user without the
    // work queue, the kernel fills every output slot and publishes the counts last — ONE launch, no memsets, no copies, no events
    *direct = *direct && !pl.wkernel && U <= (int64_t)pl.grid * pl.nteams && !d_coff && !d_tn;
    if (!*direct) return DM_OK;             // nothing launched: the caller takes the staged path
    p.host_direct = 1;
    p.scored_rows = &h->d_ctr->rows_sink;     // nothing is zeroed on this path: keep dm_last_scored_rows' counter out of it
    return launch_beam(h, p, pl);
  }
  HIPCHK(h, reset_search_counters(h, keep_rows));
  HIPCHK(h, prefill_results(h, U, o->topk, d_ids, d_scores, 4, d_counts));
  return launch_beam(h, p, pl);
}

// ---- pipelined host-buffer searches.  The reference-shaped entry points take and return host arrays; at serving batch sizes the results
// are the bulk of a call (131 072 users x 200 x 8 B = 210 MB) and used to come down AFTER the kernel, through pageable memory: 98.6 ms per
// call against 77.5 ms for the kernel alone (round-4 bench).  Large requests are now cut into chunks of users: every chunk's kernel is
// enqueued up front on the handle's stream with an event behind it, and the host thread downloads chunk k on a second, non-blocking
// stream as soon as its event fires — under the kernels of the chunks behind it.  Only the last chunk's download is exposed.
// DM_HOST_PIPELINE=0 keeps the one-launch path (A/B).
// Chunk k covers users [off[k], off[k + 1]): equal chunks of about 24 MB of results, then a SHORT last one (its download is the only
// one nothing hides; 8 192 users still fill the persistent grid eight users deep).  n = 1: the request is not cut.
static int host_pipe_plan(size_t bytes_per_user, int64_t U, int64_t *off /* [18] */) {
  static const bool disabled = env_off("DM_HOST_PIPELINE");
  off[0] = 0; off[1] = U;
  const size_t out_bytes = bytes_per_user * (size_t)U;
  if (disabled || U < 16384 || out_bytes < (32u << 20)) return 1;
  const int64_t last = U >= 65536 ? 8192 : 4096;
  const int64_t rest = U - last;
  int n = (int)((bytes_per_user * (size_t)rest + (24u << 20) - 1) / (24u << 20));
  if (n > 16) n = 16;
  if ((int64_t)n > rest / 4096) n = (int)(rest / 4096);
  if (n < 1) n = 1;
  const int64_t Uc = (((rest + n - 1) / n) + 255) / 256 * 256;
  int k = 0;
  for (; k < n && (int64_t)k * Uc < rest; k++) off[k] = (int64_t)k * Uc;
  off[k] = rest; off[k + 1] = U;
  return k + 1;
}

static int host_max_beam(const dm_tdm_search_opts *o, const int64_t *coff, int64_t U) {
  int mb = o->beam;
  if (o->widen_consumed && coff)
    for (int64_t u = 0; u < U; u++) {
      int64_t w = ((coff[u + 1] - coff[u]) + o->topk) / 2;   // Recommender.scala:31
      if (w > mb) mb = (int)w;
    }
  return mb;
}

int dm_tdm_beam_search_dev(dm_handle_t h, const int32_t *d_seq_item_ids, int64_t U, int L, const dm_tdm_search_opts *opts,
                           const int64_t *d_consumed_off, const int32_t *d_consumed_ids, int32_t *d_out_item_ids,
                           float *d_out_scores, int32_t *d_out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!d_seq_item_ids || !opts || !d_out_item_ids || !d_out_scores || !d_out_counts) return fail(h, DM_ERR_INVALID, "dm_tdm_beam_search_dev: NULL argument");
  HIPCHK(h, hipSetDevice(h->device));
  int mb = opts->beam;
  if (opts->widen_consumed && d_consumed_off) {
    std::vector<int64_t> coff((size_t)U + 1);
    HIPCHK(h, hipMemcpy(coff.data(), d_consumed_off, (U + 1) * 8, hipMemcpyDeviceToHost));
    mb = host_max_beam(opts, coff.data(), U);
  }
  return tdm_search_dev(h, d_seq_item_ids, U, L, opts, mb, d_consumed_off, d_consumed_ids, d_out_item_ids, d_out_scores,
                        d_out_counts, 0, nullptr, nullptr, nullptr, false);
}

static int tdm_search_host(dm_ctx *h, const int32_t *seq, int64_t U, int L, const dm_tdm_search_opts *opts,
                           const int64_t *coff, const int32_t *cids, int32_t *out_ids, float *out_scores,
                           int32_t *out_counts, int max_levels, int32_t *tc, float *ts, int32_t *tn) {
  if (U == 0 && L > 0 && opts && opts->beam > 0 && opts->topk > 0) return DM_OK;          // an empty batch is not an error
  if (!seq || !opts || !out_ids || !out_scores || !out_counts || U <= 0 || L <= 0) return fail(h, DM_ERR_INVALID, "dm_tdm_beam_search: bad arguments");
  if (opts->beam <= 0 || opts->topk <= 0) return fail(h, DM_ERR_INVALID, "dm_tdm_beam_search: beam and topk must be positive");
  if ((coff == nullptr) != (cids == nullptr) && coff && coff[U] > 0) return fail(h, DM_ERR_INVALID, "dm_tdm_beam_search: consumed_off / consumed_ids must both be given");
  HIPCHK(h, hipSetDevice(h->device));
  const int mb = host_max_beam(opts, coff, U);
  int cap;
  frontier_caps(mb, &cap, nullptr);
  const size_t topk = (size_t)opts->topk;
  const int64_t nc = coff ? coff[U] : 0;
  // trace buffers (parity instrumentation) are per call, not arena space: a large trace does not enlarge h->req for good
  ReqLayout lay(h, h->req, 2, U, (size_t)L * 4, topk, 4);
  if (tn) lay.trace(max_levels, cap, 4, true);
  if (coff) lay.extras((size_t)(U + 1) * 8, (size_t)(nc > 0 ? nc : 1) * 4);
  int rc = lay.commit(out_ids, out_scores, out_counts, tc, ts, tn);
  if (rc != DM_OK) return rc;
  int32_t *d_seq = lay.d<int32_t>(lay.SEQ), *d_ids = lay.d<int32_t>(lay.IDS), *d_counts = lay.d<int32_t>(lay.COUNTS), *d_cids = lay.d<int32_t>(lay.X1);
  int64_t *d_coff = lay.d<int64_t>(lay.X0);
  float *d_scores = lay.d<float>(lay.SCORES);
  if (lay.fits_stage() && (rc = lay.stage(seq)) != DM_OK) return rc;
  if (lay.staged && h->direct_ok && U <= 8) {
    // Single-request path (the reference's serving loop: one user per call, examples/.../tdm/package.scala:114-124)
    lay.arm_direct();
    bool direct = true;
    rc = tdm_search_dev(h, lay.stage_ptr(d_seq), U, L, opts, mb, nullptr, nullptr, lay.stage_ptr(d_ids), lay.stage_ptr(d_scores),
                        lay.stage_ptr(d_counts), 0, nullptr, nullptr, nullptr, false, &direct);
    if (rc != DM_OK) return rc;
    if (direct) return lay.wait_direct("tdm beam search");
    // the plan did not allow it (one-wave-per-SIMD kernel, too many users for the grid): fall through to the staged path
  }
  if (lay.upload(seq) != hipSuccess) return fail(h, DM_ERR_HIP, "upload failed");
  int64_t off[18];
  const int n_chunks = (lay.staged || coff || tn || level_pipeline(h, mb, L)) ? 1 : host_pipe_plan(lay.result_bytes_per_user(), U, off);
  if (n_chunks > 1) {      // chunks of users, downloads under the kernels behind them (host_pipe_plan)
    int launched;
    rc = launch_chunks(h, n_chunks, off, [&](int k, int64_t u0, int64_t uk) {
      return tdm_search_dev(h, d_seq + u0 * L, uk, L, opts, mb, nullptr, nullptr, d_ids + u0 * topk, d_scores + u0 * topk, d_counts + u0, 0, nullptr, nullptr, nullptr, k > 0);
    }, &launched);
    const hipError_t e = download_chunks(h, lay.outs, 3, off, launched);
    if (rc == DM_OK && e != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string("tdm beam search (pipelined download): ") + hipGetErrorString(e));
    return rc;
  }
  if (coff) {
    if (hipMemcpyAsync(d_coff, coff, (size_t)(U + 1) * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, "upload failed");
    if (nc > 0 && hipMemcpyAsync(d_cids, cids, (size_t)nc * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, "upload failed");
  }
  DevTemps trace(h);
  int32_t *d_tc = nullptr, *d_tn = nullptr; float *d_ts = nullptr;
  if (tn) {
    if ((rc = trace.alloc(d_tc, lay.array_bytes(lay.TC))) != DM_OK || (rc = trace.alloc(d_ts, lay.array_bytes(lay.TS))) != DM_OK ||
        (rc = trace.alloc(d_tn, lay.array_bytes(lay.TN))) != DM_OK) return rc;
    lay.trace_at(d_tc, d_ts, d_tn);
    if (lay.clear_trace() != hipSuccess) return fail(h, DM_ERR_HIP, "memset failed");
  }
  if ((rc = tdm_search_dev(h, d_seq, U, L, opts, mb, d_coff, d_cids, d_ids, d_scores, d_counts, tn ? max_levels : 0, d_tc, d_ts, d_tn, false)) != DM_OK) return rc;
  const hipError_t e = lay.finish();
  return e == hipSuccess ? DM_OK : fail(h, DM_ERR_HIP, std::string("tdm beam search: ") + hipGetErrorString(e));
}

int dm_tdm_beam_search(dm_handle_t h, const int32_t *seq_item_ids, int64_t U, int L, const dm_tdm_search_opts *opts,
                       const int64_t *consumed_off, const int32_t *consumed_ids, int32_t *out_item_ids, float *out_scores,
                       int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  return tdm_search_host(h, seq_item_ids, U, L, opts, consumed_off, consumed_ids, out_item_ids, out_scores, out_counts, 0,
                         nullptr, nullptr, nullptr);
}

int dm_tdm_beam_search_trace(dm_handle_t h, const int32_t *seq_item_ids, int64_t U, int L, const dm_tdm_search_opts *opts,
                             int32_t *out_item_ids, float *out_scores, int32_t *out_counts, int max_levels,
                             int32_t *trace_codes, float *trace_scores, int32_t *trace_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (max_levels <= 0 || !trace_codes || !trace_scores || !trace_counts) return fail(h, DM_ERR_INVALID, "dm_tdm_beam_search_trace: bad trace arguments");
  return tdm_search_host(h, seq_item_ids, U, L, opts, nullptr, nullptr, out_item_ids, out_scores, out_counts, max_levels,
                         trace_codes, trace_scores, trace_counts);
}

static int otm64_search_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, int beam, int leaf_level, int32_t *d_ids,
                            double *d_sc64, float *d_sc32, int32_t *d_counts, int max_levels, int cap, int32_t *d_tc,
                            double *d_ts64, float *d_ts32, int32_t *d_tn);
static int otm64_search_host(dm_ctx *h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                             int32_t *out_node_ids, double *out_sc64, float *out_sc32, int32_t *out_counts, int max_levels,
                             int32_t *tc, double *ts64, float *ts32, int32_t *tn);

// OTM search on device buffers: d_ids / d_scores [U][2*beam], d_counts [U]; optional level traces (device)
static int otm_search_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int L, int beam, int leaf_level, int32_t *d_ids,
                          float *d_scores, int32_t *d_counts, int max_levels, int32_t *d_tc, float *d_ts, int32_t *d_tn,
                          const SearchPlan &pl, bool keep_rows) {
  const int stride = 2 * beam;
  BeamParams p;
  fill_common(h, p);
  const int rc = fill_frontier(h, p, pl);
  if (rc != DM_OK) return rc;
  HIPCHK(h, prefill_results(h, U, stride, d_ids, d_scores, 4, d_counts));
  HIPCHK(h, reset_search_counters(h, keep_rows));
  p.seq = d_seq; p.U = U; p.L = L; p.use_mask = 1; p.beam = beam; p.topk = stride; p.mode = 1; p.otm_leaf_level = leaf_level;
  p.out_ids = d_ids; p.out_scores = d_scores; p.out_counts = d_counts; p.out_stride = stride;
  p.trace_codes = d_tc; p.trace_scores = d_ts; p.trace_counts = d_tn; p.trace_levels = d_tn ? max_levels : 0;
  return launch_beam(h, p, pl);
}

static int otm_check(dm_ctx *h, int64_t U, int L, int beam, int leaf_level, const char *who) {
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": weights not loaded");
  DM_DIN_ONLY(h, who);
  if (U < 0 || L <= 0 || L > DM_PIPE_MAXL || beam <= 0 || leaf_level <= 0 || leaf_level > 30)
    return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments (L must be 1..32)");
  if ((((int64_t)1) << (leaf_level + 1)) - 1 > h->num_index) return fail(h, DM_ERR_INDEX, std::string(who) + ": leaf level exceeds the embedding table");
  return DM_OK;
}

// device-resident request (serving loops that keep their batches in HBM; the counterpart of dm_tdm_beam_search_dev).
// History codes outside the table are treated as padding by the kernel (the host entry point rejects them).
int dm_otm_beam_search_dev(dm_handle_t h, const int32_t *d_seq_codes, int64_t U, int L, int beam, int leaf_level,
                           int32_t *d_out_node_ids, float *d_out_scores, int32_t *d_out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  int rc = otm_check(h, U, L, beam, leaf_level, "dm_otm_beam_search_dev");
  if (rc != DM_OK) return rc;
  if (U == 0) return DM_OK;
  if (!d_seq_codes || !d_out_node_ids || !d_out_scores || !d_out_counts) return fail(h, DM_ERR_INVALID, "dm_otm_beam_search_dev: NULL argument");
  HIPCHK(h, hipSetDevice(h->device));
  if (use_f64_beam(h) || long_history_pipeline(h, beam, L)) {      // (long histories beyond the fused kernel's LDS: the per-level pipeline in the model's type)
    return otm64_search_dev(h, d_seq_codes, U, L, beam, leaf_level, d_out_node_ids, nullptr, d_out_scores, d_out_counts, 0, 0, nullptr,
                            nullptr, nullptr, nullptr);
  }
  int start, level;
  level_start_int(beam, &start, &level);
  SearchPlan pl;
  if ((rc = plan_search(h, beam, U, L, leaf_level - level, false, &pl)) != DM_OK) return rc;
  return otm_search_dev(h, d_seq_codes, U, L, beam, leaf_level, d_out_node_ids, d_out_scores, d_out_counts, 0, nullptr, nullptr, nullptr, pl, false);
}

static int otm_search_host(dm_ctx *h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                           int32_t *out_node_ids, float *out_scores, int32_t *out_counts, int max_levels, int32_t *tc,
                           float *ts, int32_t *tn) {
  int rc = otm_check(h, U, L, beam, leaf_level, "dm_otm_beam_search");
  if (rc != DM_OK) return rc;
  if (U == 0) return DM_OK;          // an empty batch is not an error
  if (!seq_codes || !out_node_ids || !out_scores || !out_counts) return fail(h, DM_ERR_INVALID, "dm_otm_beam_search: bad arguments");
  if ((rc = check_table_ids(h, "dm_otm_beam_search", "history code", seq_codes, U * L, -1)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  int start, level;
  level_start_int(beam, &start, &level);
  SearchPlan pl;
  if ((rc = plan_search(h, beam, U, L, leaf_level - level, false, &pl)) != DM_OK) return rc;
  const size_t stride = (size_t)2 * beam;
  ReqLayout lay(h, h->req, 2, U, (size_t)L * 4, stride, 4);
  if (tn) lay.trace(max_levels, pl.cap, 4);
  if ((rc = lay.commit(out_node_ids, out_scores, out_counts, tc, ts, tn)) != DM_OK) return rc;
  int32_t *d_seq = lay.d<int32_t>(lay.SEQ), *d_ids = lay.d<int32_t>(lay.IDS), *d_counts = lay.d<int32_t>(lay.COUNTS);
  float *d_scores = lay.d<float>(lay.SCORES);
  HIPCHK(h, lay.upload(seq_codes));
  int64_t off[18];
  const int n_chunks = tn ? 1 : host_pipe_plan(lay.result_bytes_per_user(), U, off);
  if (n_chunks > 1) {      // chunks of users, downloads under the kernels behind them (host_pipe_plan)
    int launched;
    rc = launch_chunks(h, n_chunks, off, [&](int k, int64_t u0, int64_t uk) {
      SearchPlan plk;
      const int rc_ = plan_search(h, beam, uk, L, leaf_level - level, false, &plk);
      return rc_ != DM_OK ? rc_ : otm_search_dev(h, d_seq + u0 * L, uk, L, beam, leaf_level, d_ids + u0 * stride, d_scores + u0 * stride, d_counts + u0, 0, nullptr, nullptr, nullptr, plk, k > 0);
    }, &launched);
    const hipError_t e = download_chunks(h, lay.outs, 3, off, launched);
    if (rc == DM_OK && e != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string("dm_otm_beam_search (pipelined download): ") + hipGetErrorString(e));
    return rc;
  }
  if (tn) HIPCHK(h, lay.clear_trace());
  if ((rc = otm_search_dev(h, d_seq, U, L, beam, leaf_level, d_ids, d_scores, d_counts, max_levels, lay.d<int32_t>(lay.TC), lay.d<float>(lay.TS), lay.d<int32_t>(lay.TN), pl, false)) != DM_OK) return rc;
  HIPCHK(h, lay.finish());
  return DM_OK;
}

int dm_otm_beam_search(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                       int32_t *out_node_ids, float *out_scores, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (use_f64_beam(h) || long_history_pipeline(h, beam, L))      // f64 weights: the reference's arithmetic (otm64.hip.inc), scores rounded to float on the way out
    return otm64_search_host(h, seq_codes, U, L, beam, leaf_level, out_node_ids, nullptr, out_scores, out_counts, 0, nullptr, nullptr, nullptr, nullptr);
  return otm_search_host(h, seq_codes, U, L, beam, leaf_level, out_node_ids, out_scores, out_counts, 0, nullptr, nullptr, nullptr);
}

int dm_otm_beam_search_trace(dm_handle_t h, const int32_t *seq_codes, int64_t U, int L, int beam, int leaf_level,
                             int32_t *out_node_ids, float *out_scores, int32_t *out_counts, int max_levels,
                             int32_t *trace_codes, float *trace_scores, int32_t *trace_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (max_levels <= 0 || !trace_codes || !trace_scores || !trace_counts) return fail(h, DM_ERR_INVALID, "dm_otm_beam_search_trace: bad trace arguments");
  if (use_f64_beam(h) || long_history_pipeline(h, beam, L))
    return otm64_search_host(h, seq_codes, U, L, beam, leaf_level, out_node_ids, nullptr, out_scores, out_counts, max_levels, trace_codes,
                             nullptr, trace_scores, trace_counts);
  return otm_search_host(h, seq_codes, U, L, beam, leaf_level, out_node_ids, out_scores, out_counts, max_levels, trace_codes,
                         trace_scores, trace_counts);
}


// Brute force over every leaf with the same fused scorer (mode 2 of the beam kernel): the
// build-defined oracle for recall@k.  Order: score descending, then leaf code ascending.
int dm_tdm_bruteforce_topk(dm_handle_t h, const int32_t *seq_item_ids, int64_t U, int L, int topk, int use_mask,
                           int32_t *out_item_ids, float *out_scores, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  if (!h->tree_loaded || !h->ids_loaded || !h->w_loaded) return fail(h, DM_ERR_STATE, "dm_tdm_bruteforce_topk: tree, id maps and weights must be loaded first");
  DM_DIN_ONLY(h, "dm_tdm_bruteforce_topk");
  if (U == 0 && L > 0 && L <= DM_PIPE_MAXL && topk > 0 && topk <= 256) return DM_OK;          // an empty batch is not an error
  if (!seq_item_ids || !out_item_ids || !out_scores || !out_counts || U <= 0 || L <= 0 || L > DM_PIPE_MAXL || topk <= 0 || topk > 256)
    return fail(h, DM_ERR_INVALID, "dm_tdm_bruteforce_topk: bad arguments (L must be 1..32, topk 1..256)");
  if (h->n_slots > h->num_index) return fail(h, DM_ERR_INDEX, "dm_tdm_bruteforce_topk: tree codes exceed the embedding table");
  HIPCHK(h, hipSetDevice(h->device));
  const int pcap = 512;
  const int chunk = ((pcap - topk) / 16) * 16;
  const int cap = chunk < 32 ? 32 : chunk;
  const int kt = L > DM_MAXL ? 2 : 1;
  const int kq = kt > 1 ? 4 : (L + 3) / 4;
  int lds = 0;
  const int nteams = beam_teams_that_fit(h->embed, 4, cap, pcap, kq, false, kt, &lds);
  if (!nteams) return fail(h, DM_ERR_UNSUPPORTED, "dm_tdm_bruteforce_topk: LDS budget exceeded");
  // enough (user, slice) work items to fill every team a few times over
  int64_t slices = (4 * (int64_t)h->n_cu * nteams + U - 1) / U;
  const int64_t max_slices = (h->n_leaf_nodes + chunk - 1) / chunk;
  if (slices > max_slices) slices = max_slices;
  if (slices < 1) slices = 1;
  int64_t per = (h->n_leaf_nodes + slices - 1) / slices;
  per = ((per + 15) / 16) * 16;
  slices = (h->n_leaf_nodes + per - 1) / per;
  const int64_t n_work = U * slices;
  if (n_work >= (1ll << 31)) return fail(h, DM_ERR_UNSUPPORTED, "dm_tdm_bruteforce_topk: too many work items");
  int32_t *d_seq = nullptr;
  unsigned long long *d_keys = nullptr;
  int rc = DM_OK;
  std::vector<unsigned long long> keys((size_t)n_work * topk);
  DevTemps t(h);
  if ((rc = ensure_ws(h, 1024)) != DM_OK) return rc;
  if ((rc = t.alloc(d_seq, (size_t)U * L * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_keys, keys.size() * 8)) != DM_OK) return rc;
  hipError_t e = hipMemcpyAsync(d_seq, seq_item_ids, (size_t)U * L * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = reset_search_counters(h, false);
  if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_tdm_bruteforce_topk: upload failed");
  BeamParams p;
  fill_common(h, p);
  p.seq = d_seq; p.U = U; p.L = L; p.use_mask = use_mask; p.beam = 2; p.topk = topk; p.mode = 2;
  p.nteams = nteams; p.cap = cap; p.pcap = pcap; p.out_stride = topk;
  p.bf_leaf_codes = h->d_leaf_codes; p.bf_n_leaf = h->n_leaf_nodes; p.bf_slices = (int)slices; p.bf_chunk = chunk;
  p.bf_per_slice = per; p.bf_out_keys = d_keys;
  p.ws_code = (int32_t *)h->ws.p; p.ws_score = (float *)h->ws.p; p.ws_khi = (uint32_t *)h->ws.p; p.ws_klo = (uint32_t *)h->ws.p;
  p.ws_cap = 0;
  SearchPlan pl;          // mode 2 always scores with the fp32-input MFMA: split stays false
  pl.nteams = nteams; pl.cap = cap; pl.pcap = pcap; pl.lds = lds; pl.ws_cap = 0;
  int64_t groups = (n_work + nteams - 1) / nteams;
  pl.grid = (int)(groups < h->n_cu ? groups : h->n_cu);
  if ((rc = launch_beam(h, p, pl)) != DM_OK) return rc;
  e = hipMemcpyAsync(keys.data(), d_keys, keys.size() * 8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, DM_ERR_HIP, std::string("dm_tdm_bruteforce_topk: ") + hipGetErrorString(e));
  std::vector<int32_t> nid((size_t)h->n_slots);
  if (hipMemcpy(nid.data(), h->d_node_id, nid.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DM_ERR_HIP, "node id download failed");
  // merge the per-slice winners (keys are unique: descending-score key << 32 | leaf code)
  std::vector<unsigned long long> row((size_t)slices * topk);
  for (int64_t u = 0; u < U; u++) {
    std::copy(keys.begin() + u * slices * topk, keys.begin() + (u + 1) * slices * topk, row.begin());
    const size_t kk = std::min<size_t>(topk, row.size());
    std::partial_sort(row.begin(), row.begin() + kk, row.end());
    int n = 0;
    for (size_t i = 0; i < kk; i++) {
      if (row[i] == ~0ull) break;
      const uint32_t code = (uint32_t)row[i], dk = (uint32_t)(row[i] >> 32);
      const uint32_t asc = ~dk;
      const uint32_t bits = (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
      float sc; memcpy(&sc, &bits, 4);
      out_item_ids[u * topk + n] = nid[code];
      out_scores[u * topk + n] = sc;
      n++;
    }
    for (int i = n; i < topk; i++) { out_item_ids[u * topk + i] = -1; out_scores[u * topk + i] = 0.f; }
    out_counts[u] = n;
  }
  return rc;
}

#include "jtm_rebalance_dev.hip.inc"
#include "jtm_host.hip.inc"
#define DM_ADAM_VEC_PART 2         // TrainVec's methods, adam_step
#include "adam_vec.hip.inc"
#include "train_host.hip.inc"
#include "sampler.hip.inc"
#include "dr_host.hip.inc"
#include "dr_train.hip.inc"
#include "dr_train_grouped.hip.inc"
#include "dr_rerank_train.hip.inc"
#include "dr_mstep.hip.inc"
#include "dr_mstep_stream.hip.inc"
#include "dr_mstep_assign.hip.inc"
#include "dr_train_set.hip.inc"
#include "otm64.hip.inc"
#include "tdm_pipeline.hip.inc"
#include "deepfm.hip.inc"
#include "dfm_train.hip.inc"
#include "dfm_train_grouped.hip.inc"
#include "train_grouped_csr.hip.inc"
#include "comm.hip.inc"
#include "rows_sync.hip.inc"
#include "dfm_train_sync.hip.inc"
#include "dr_train_sync.hip.inc"
#include "dfm_jtm.hip.inc"
#include "jtm_sharded.hip.inc"
#include "train_grouped_host.hip.inc"
#include "dfm_otm.hip.inc"
#include "dfm_otm_tree.hip.inc"
#include "otm_train.hip.inc"
#include "checkpoint.hip.inc"
#include "tree_file.hip.inc"
#include "cluster.hip.inc"

// ---- device memory helpers
int dm_dev_alloc(dm_handle_t h, size_t bytes, void **dptr) {
  if (!h || !dptr) return DM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  return dm_alloc(h, dptr, bytes);
}
int dm_dev_free(dm_handle_t h, void *dptr) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, dm_free_one(dptr));
  return DM_OK;
}
int dm_memcpy_h2d(dm_handle_t h, void *dst, const void *src, size_t bytes) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return DM_OK;
}
int dm_memcpy_d2h(dm_handle_t h, void *dst, const void *src, size_t bytes) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return DM_OK;
}

// ---- measurement
int dm_kernel_timing_reset(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ev_used = 0;
  return DM_OK;
}
int dm_kernel_timing_get(dm_handle_t h, int *launches, double *total_ms) {
  if (!h || !launches || !total_ms) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double tot = 0;
  int n = 0;
  for (size_t i = 0; i < h->ev_used; i++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev_pool[i].first, h->ev_pool[i].second) != hipSuccess) { (void)hipGetLastError(); continue; }     // (see dm_kernel_timing_get_kind)
    tot += ms; n++;
  }
  *launches = n; *total_ms = tot;
  return DM_OK;
}
const char *dm_last_beam_kernel(dm_handle_t h) { return h ? h->last_kernel : ""; }
// debug entry (not in the public header): did the last search on the one-wave-per-SIMD kernel read the setup table, is the owner's
// table current, and its size
extern "C" int dm_debug_g_table(dm_handle_t h, int *used_last, int *current, unsigned long long *bytes) {
  if (!h || !used_last || !current || !bytes) return DM_ERR_INVALID;
  dm_ctx *o = h->parent ? h->parent : h;
  std::lock_guard<std::recursive_mutex> lk_(o->mu);
  *used_last = h->last_g_table ? 1 : 0;
  *current = (o->lazy.d_g_table && !o->lazy.g_table_dirty) ? 1 : 0;
  *bytes = o->lazy.d_g_table ? (unsigned long long)o->lazy.g_table_bytes : 0ull;
  return DM_OK;
}
int dm_kernel_timing_get_kind(dm_handle_t h, int kind, int *launches, double *total_ms) {
  if (!h || !launches || !total_ms) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double tot = 0;
  int n = 0;
  for (size_t i = 0; i < h->ev_used; i++) {
    if (h->ev_kind[i] != kind) continue;
    float ms = 0;
    // (a pair whose stop event was never recorded — a call that failed between its two records — is skipped, not an error of this query)
    if (hipEventElapsedTime(&ms, h->ev_pool[i].first, h->ev_pool[i].second) != hipSuccess) { (void)hipGetLastError(); continue; }
    tot += ms; n++;
  }
  *launches = n; *total_ms = tot;
  return DM_OK;
}
// debug (not part of the public header): cumulative per-phase wave cycles, DM_PHASE_TIMERS builds
extern "C" int dm_debug_phase_cycles(dm_handle_t h, unsigned long long *out8) {
  if (!h || !out8 || !h->d_phase) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out8, h->d_phase, 128, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->d_phase, 0, 128));
  return DM_OK;
}
// debug (not part of the public header): Deep-Retrieval layers that fell back to the exact radix-select path
extern "C" int dm_debug_dr_slow_layers(dm_handle_t h, unsigned long long *out, int reset) {
  if (!h || !out) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, &h->d_ctr->dr_slow, 8, hipMemcpyDeviceToHost));
  if (reset) HIPCHK(h, hipMemset(&h->d_ctr->dr_slow, 0, 8));
  return DM_OK;
}
// debug: user-layers the one-wave cut of the sliced Deep-Retrieval search handed to the block version
extern "C" int dm_debug_dr_wave_fallbacks(dm_handle_t h, unsigned long long *out, int reset) {
  if (!h || !out) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, &h->d_ctr->dr_wave_count, 16, hipMemcpyDeviceToHost));      // out[0] = count, out[1] = per-reason byte counters
  if (reset) HIPCHK(h, hipMemset(&h->d_ctr->dr_wave_count, 0, 16));
  return DM_OK;
}
int dm_last_scored_rows(dm_handle_t h, int64_t *rows) {
  if (!h || !rows) return DM_ERR_INVALID;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned long long r = 0;
  HIPCHK(h, hipMemcpy(&r, &h->d_ctr->rows, 8, hipMemcpyDeviceToHost));
  *rows = (int64_t)r;
  return DM_OK;
}

