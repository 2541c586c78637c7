// Host-request layer (host code only): what the six host-buffer search front ends share — tdm_search_host and otm_search_host
// (dm_hip.hip), otm64_search_host (otm64.hip.inc), dfm_otm_search_host (dfm_otm.hip.inc), dm_dr_beam_search and dm_dr_recommend
// (dr_host.hip.inc) — and the event pair around one launch.  ReqLayout owns the layout of a request and its invariants; a front end
// keeps its own checks and its own policy — which requests are staged, served in place or cut into chunks — and calls the layout.

// ---- frontier sizing of a beam search: cap = slots of a level's candidate list (2 * beam in whole 16-row tiles, at least two tiles),
// pcap = the sort's power of two above it
static void frontier_caps(int max_beam, int *cap, int *pcap) {
  int c = ((2 * max_beam + 15) / 16) * 16;
  if (c < 32) c = 32;
  int p = 32;
  while (p < c) p <<= 1;
  *cap = c;
  if (pcap) *pcap = p;
}

// ---- what an event pair is recorded as (dm_kernel_timing_get_kind).  The numbers are read by tools and tests: they do not change.
// Deep-Retrieval's sliced search numbers its launches per layer d: EV_DR_STATS + 2 d = the statistics of layer d >= 1, EV_DR_CUT + 2 d =
// its cut (d = 0: the layer-0 launch), EV_DR_BLOCK + 2 d = the block version's second pass over the users the one-wave cut flagged.
// 40 .. 45 mean two things: the grouped fp64 training step of a DIN model and the serving / tree-learning launches of a DeepFM model (a
// handle holds one).
enum EvKind {
  EV_MAIN = 0,            // a search's main kernel, a whole Deep-Retrieval search, and every launch nobody asks for by kind
  EV_DEFERRED = 1,        // the second pass over the users the one-wave-per-SIMD beam kernel deferred
  EV_DR_STATS = 10, EV_DR_CUT = 11, EV_DR_BLOCK = 21,
  EV_ROWS = 30,           // general rows (rows_kernel.hip.inc)
  EV_DFM_USER = 40, EV_DFM_LEVEL = 41,
  EV_DFM_JTM_ROWS = 42, EV_DFM_JTM_PAIRS = 43,      // the pair scorer of JTM tree learning (dfm_jtm.hip.inc): per-history set-up, per-pair score
  EV_DFM_OTM = 42,        // the fused OTM beam search of a DeepFM model (dfm_otm.hip.inc): a call is a search or a tree-learning step, never both
  EV_DFM_OTM_TREE_SCORE = 44, EV_DFM_OTM_TREE_SUM = 45,      // OTM tree construction with a DeepFM model (dfm_otm_tree.hip.inc): unit scores, segment sums + chain
  EV_TG_SETUP = 40, EV_TG_ROWS = 41, EV_TG_WGRAD_A = 42, EV_TG_USER_BWD = 43, EV_TG_WGRAD_B = 44,
  // the Deep-Retrieval training step under DM_DR_TIME_LAUNCHES=1 (dr_train.hip.inc): forward GEMMs, softmax + cross-entropy, dX products,
  // dW / db products with their slab sums, embedding gradient (pairs, sort, segment sums), Adam
  EV_DRT_FWD = 50, EV_DRT_SOFTMAX = 51, EV_DRT_DX = 52, EV_DRT_DW = 53, EV_DRT_EMB = 54, EV_DRT_ADAM = 55,
  // the rerank model's training step (dr_rerank_train.hip.inc): user-vector GEMM, classes of the rows (sampler), sampled softmax, the
  // softmax tables' gradient (pairs, sort, segment sums), dX, dW / db with their slab sums, embedding gradient, both Adam updates
  // the DeepFM training step under DM_DFM_TIME_LAUNCHES=1 (dfm_train.hip.inc): the fused rows kernel (forward, loss, dH, dX), the l1.W / l1.b
  // product with its slab sum, embedding gradient (pairs, sort, segment sums), Adam
  EV_DFT_ROWS = 70, EV_DFT_DW = 71, EV_DFT_EMB = 72, EV_DFT_ADAM = 73,
  // its user-grouped form (dfm_train_grouped.hip.inc): the per-user set-up, the rows kernel, the per-user backward; its two l1.W products
  // are EV_DFT_DW and its embedding gradient EV_DFT_EMB
  EV_DFG_SETUP = 74, EV_DFG_ROWS = 75, EV_DFG_USER_BWD = 76,
  // its gradient exchange across ranks (dfm_train_sync.hip.inc): this rank's unique rows and its block; after the all-gather, the tails'
  // and the rows' rank-ordered sums with their bookkeeping
  EV_DFT_SYNC_PACK = 77, EV_DFT_SYNC_SUM = 78,
  // the Deep-Retrieval layer model's gradient exchange (dr_train_sync.hip.inc) under DM_DR_TIME_LAUNCHES=1: the same two brackets
  EV_DRT_SYNC_PACK = 79, EV_DRT_SYNC_SUM = 93,
  EV_DRR_FWD = 60, EV_DRR_SAMPLE = 61, EV_DRR_SOFTMAX = 62, EV_DRR_SMGRAD = 63, EV_DRR_DX = 64, EV_DRR_DW = 65, EV_DRR_EMB = 66, EV_DRR_ADAM = 67,
  // the Deep-Retrieval M-step's path scores under DM_DR_TIME_LAUNCHES=1 (dr_mstep.hip.inc): pairs of a chunk, the (item, path) sort, segment
  // heads (flags + compaction), segment sums, the sort by score, the sort by item (with its key kernel), the cut at C (flags + compaction),
  // codes / scores / offsets, occurrences.  The searches of the chunks are EV_MAIN, as everywhere
  EV_DRM_PAIRS = 80, EV_DRM_SORT = 81, EV_DRM_HEADS = 82, EV_DRM_SEGSUM = 83, EV_DRM_SCORE_SORT = 84, EV_DRM_ITEM_SORT = 85, EV_DRM_CUT = 86, EV_DRM_EMIT = 87,
  EV_DRM_OCC = 88,
  // its streaming mode (dr_mstep_stream.hip.inc), under the same switch: path codes of a chunk, the order of the samples by item (sort, runs,
  // queue sort), the per-item fold, the compaction into the CSR
  EV_DMS_CODES = 89, EV_DMS_ORDER = 90, EV_DMS_FOLD = 91, EV_DMS_EMIT = 92,
  // its greedy path assignment (dr_mstep_assign.hip.inc), under the same switch: dense path indices (sort, heads, ranks), validation + hit list,
  // the chain (one launch per iteration), random paths + the decode of the chosen positions.  (90 .. 93 were taken when these were added.)
  EV_DRA_INDEX = 94, EV_DRA_CHECK = 95, EV_DRA_CHAIN = 96, EV_DRA_RANDOM = 97,
  // the resident mapping and training set (dr_train_set.hip.inc), under the same switch: the path -> items CSR built from the table (codes,
  // sort, flags, compactions, offsets), the shuffle (keys + sort), the gather of one range of samples
  EV_DTS_CSR = 98, EV_DTS_SHUFFLE = 99, EV_DTS_GATHER = 100,
  // the ragged user-grouped DIN training step under DM_TRAIN_TIME_LAUNCHES=1 (train_grouped_csr.hip.inc): per-user set-up, the rows kernel, the
  // per-user backward, the dense gradients (column sums, three products with their slab sums), the table gradient (pairs, sort, segment sums)
  EV_DTC_SETUP = 56, EV_DTC_ROWS = 57, EV_DTC_USER_BWD = 58, EV_DTC_DW = 59, EV_DTC_EMB = 68,
};

// the next pair of the handle's pool, recorded as `kind`
static int next_events(dm_ctx *h, int kind, hipEvent_t *a, hipEvent_t *b) {
  if (h->ev_used >= 4096) h->ev_used = 0;      // a service that never reads the timings keeps a bounded pool (oldest pairs are reused)
  if (h->ev_used == h->ev_pool.size()) {
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    h->ev_pool.push_back({e0, e1});
  }
  *a = h->ev_pool[h->ev_used].first; *b = h->ev_pool[h->ev_used].second;
  if (h->ev_kind.size() <= h->ev_used) h->ev_kind.resize(h->ev_used + 1);
  h->ev_kind[h->ev_used] = kind;
  h->ev_used++;
  return DM_OK;
}

// ---- HIP-event pair around one launch (or one bracket of launches) on the handle's stream.  on = false: no pair at all, rc stays
// DM_OK and stop() does nothing.
struct LaunchTimer {
  dm_ctx *h; hipEvent_t e0 = nullptr, e1 = nullptr; int rc = DM_OK; bool on;
  explicit LaunchTimer(dm_ctx *h_, int kind = EV_MAIN, bool on_ = true) : h(h_), on(on_) {
    if (!on) return;
    rc = next_events(h, kind, &e0, &e1);
    if (rc == DM_OK && hipEventRecord(e0, h->stream) != hipSuccess) rc = fail(h, DM_ERR_HIP, "hipEventRecord failed");
  }
  int stop() { return (on && rc == DM_OK && hipEventRecord(e1, h->stream) != hipSuccess) ? fail(h, DM_ERR_HIP, "hipEventRecord failed") : rc; }
};

// ---- the one way a kernel is launched.  Every launch is followed by its own hipGetLastError(), so a refused launch (an empty grid, an
// LDS request over the limit) is reported at its site and under its own name.  The kernel comes as a function pointer and the arguments
// are converted to ITS parameter types (implicit conversions only, forwarded without a copy of their own): a wrong argument is a compile
// error, and no call site casts to steer a deduction.
//   launch_on(stream, kernel, grid, block, lds, args...)      -> hipError_t: for code that has a stream and no handle (dev_sort.hip.inc)
//   launch_lds_on(...)                                        the same after opting the kernel in to `lds` bytes of dynamic LDS (not cached)
//   lds_opt_in(kernel, lds)                                   the opt-in alone: ahead of timed(), so that the host call stays outside the pair, and
//                                                             where an occupancy query or a loop of launches follows it
//   LAUNCH(h, kernel, grid, block, lds, args...)              on h->stream -> DM_OK, or DM_ERR_HIP with the error and the site in h->err
//   LAUNCH_LDS(h, ...)                                        LAUNCH with the opt-in
//   LAUNCHCHK(h, ...)                                         LAUNCH, and the calling function returns the rc when it is not DM_OK
//   timed(h, kind, on, body)                                  an event pair of `kind` (none when !on) around body(), which returns an rc;
//                                                             a failing body leaves the pair open (dm_kernel_timing_get* skips those)
template <typename... P, typename... A>
static hipError_t launch_on(hipStream_t stream, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, A &&...args) {
  static_assert(sizeof...(P) == sizeof...(A), "launch: one argument per kernel parameter");
  static_assert((std::is_convertible<A &&, P>::value && ...), "launch: an argument does not convert to its kernel parameter");
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<P>(std::forward<A>(args))...);
  return hipGetLastError();
}
template <typename... P>
static hipError_t lds_opt_in(void (*kernel)(P...), size_t lds) {
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
template <typename... P, typename... A>
static hipError_t launch_lds_on(hipStream_t stream, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, A &&...args) {
  const hipError_t e = lds_opt_in(kernel, lds);
  return e != hipSuccess ? e : launch_on(stream, kernel, grid, block, lds, std::forward<A>(args)...);
}
static int launch_rc(dm_ctx *h, hipError_t e, const char *what, const char *file, int line) {
  if (e == hipSuccess) return DM_OK;
  char b[512];
  snprintf(b, sizeof b, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
  return fail(h, DM_ERR_HIP, b);
}
#define LAUNCH(h, kernel, ...) launch_rc(h, launch_on((h)->stream, kernel, __VA_ARGS__), "launch of " #kernel, __FILE__, __LINE__)
#define LAUNCH_LDS(h, kernel, ...) launch_rc(h, launch_lds_on((h)->stream, kernel, __VA_ARGS__), "launch of " #kernel, __FILE__, __LINE__)
#define LAUNCHCHK(h, ...) do { const int rc_ = LAUNCH(h, __VA_ARGS__); if (rc_ != DM_OK) return rc_; } while (0)      // as HIPCHK: returns from the caller

template <typename Body>
static int timed(dm_ctx *h, int kind, bool on, Body body) {
  LaunchTimer tm(h, kind, on);
  if (tm.rc != DM_OK) return tm.rc;
  const int rc = body();
  return rc != DM_OK ? rc : tm.stop();
}

// ---- environment switches.  A reader reads the environment when it is called: a site that reads once per process keeps the result in a
// function-local static, every other site reads per call (the tests flip switches inside one process).  "On" is a first character '1',
// "off" a first character '0'; env_int is 0 when the variable is unset or not positive.
static inline const char *env_str(const char *name) { return getenv(name); }
static inline bool env_on(const char *name) { const char *e = env_str(name); return e && e[0] == '1'; }
static inline bool env_off(const char *name) { const char *e = env_str(name); return e && e[0] == '0'; }
static inline long long env_int(const char *name) { const char *e = env_str(name); const long long v = e ? atoll(e) : 0; return v > 0 ? v : 0; }

// ---- request arena: the device buffers of one host-buffer request, laid out in h->req (grow only, by half again: no hipMalloc /
// hipFree on the request path once the handle has seen its largest request).  add() every buffer, commit(), then ptr<T>(offset).
struct ReqArena : DevArena {
  explicit ReqArena(dm_ctx *h) : DevArena(h->req, 2) {}
};

// ---- one result array of a request: `bytes_per_user` bytes per user at `dev` (in the arena, or a per-call buffer) go to `host`
struct HostOut { void *host; const void *dev; size_t bytes_per_user; };

// ---- request layout: the arrays of one host-buffer request in a grow-only buffer, in the one order
//   [seq | ids | scores | counts | trace codes | trace scores | trace counts | extra 0 | extra 1]
// and the three things that order is for:
//   1. the pinned staging block (ensure_stage) mirrors the head [seq .. counts]: an array at arena offset o is staged at h_stage + o,
//      and the single-request kernels address it as d_stage + o (stage_ptr);
//   2. ids, scores and counts are adjacent, so a staged download is ONE copy;
//   3. trace codes, scores and counts are adjacent, so ONE memset clears them (the kernels write the live slots only).
// Arena sizes, device pointers and the HostOut table come from the same bytes[] and cannot disagree.  A front end constructs it,
// names the optional arrays (trace, extras), commits, and states its policy in terms of fits_stage() / stage() / arm_direct().
struct ReqLayout {
  enum { SEQ, IDS, SCORES, COUNTS, TC, TS, TN, X0, X1, N };
  dm_ctx *h; DevArena ar; int64_t U;
  size_t bytes[N] = {};          // per user (X0, X1: the whole array); 0 = the array is absent
  char *dev[N] = {};             // null where absent
  size_t head_bytes = 0;         // [seq .. counts]
  bool trace_external = false, staged = false;
  HostOut outs[6] = {};          // ids, scores, counts, trace codes, trace scores, trace counts

  // ids [U][stride][id_width] int32, scores [U][stride] of score_bytes (4 or 8), counts [U]; buf grows by need / slack_div (0: exactly)
  ReqLayout(dm_ctx *h_, DevGrow &buf, size_t slack_div, int64_t U_, size_t seq_bytes, size_t stride, size_t score_bytes, size_t id_width = 1)
      : h(h_), ar(buf, slack_div), U(U_) {
    bytes[SEQ] = seq_bytes; bytes[IDS] = stride * id_width * 4; bytes[SCORES] = stride * score_bytes; bytes[COUNTS] = 4;
  }
  // level traces [U][max_levels][cap]; external: the caller owns the three buffers (trace_at), the arena holds none
  void trace(int max_levels, int cap, size_t score_bytes, bool external = false) {
    bytes[TC] = (size_t)max_levels * cap * 4; bytes[TS] = (size_t)max_levels * cap * score_bytes; bytes[TN] = (size_t)max_levels * 4;
    trace_external = external;
  }
  void extras(size_t bytes0, size_t bytes1) { bytes[X0] = bytes0; bytes[X1] = bytes1; }
  size_t array_bytes(int a) const { return a >= X0 ? bytes[a] : bytes[a] * (size_t)U; }
  size_t result_bytes_per_user() const { return bytes[IDS] + bytes[SCORES]; }

  // host_* : where the result arrays go (trace ones null without a trace)
  int commit(void *host_ids, void *host_scores, void *host_counts, void *host_tc = nullptr, void *host_ts = nullptr, void *host_tn = nullptr) {
    size_t off[N];
    for (int a = 0; a < N; a++) {
      off[a] = ar.add(trace_external && a >= TC && a <= TN ? 0 : array_bytes(a));
      if (a == COUNTS) head_bytes = ar.need;
    }
    const int rc = ar.commit(h);
    if (rc != DM_OK) return rc;
    for (int a = 0; a < N; a++) dev[a] = bytes[a] ? ar.base + off[a] : nullptr;
    void *const host[6] = {host_ids, host_scores, host_counts, host_tc, host_ts, host_tn};
    for (int i = 0; i < 6; i++) outs[i] = {host[i], dev[IDS + i], bytes[IDS + i]};
    return DM_OK;
  }
  void trace_at(void *d_tc, void *d_ts, void *d_tn) {
    dev[TC] = (char *)d_tc; dev[TS] = (char *)d_ts; dev[TN] = (char *)d_tn;
    for (int i = 3; i < 6; i++) outs[i].dev = dev[IDS + i];
  }
  template <typename T> T *d(int a) const { return (T *)dev[a]; }
  bool has_trace() const { return bytes[TN] != 0; }
  int n_outs() const { return has_trace() ? 6 : 3; }

  // small requests go up and come down through ONE pinned block: a pageable copy costs 10-15 us each, a single-user search 60 us
  bool fits_stage() const { return !has_trace() && !bytes[X0] && !bytes[X1] && head_bytes <= (256u << 10); }
  int stage(const void *seq) {
    const int rc = ensure_stage(h);
    if (rc != DM_OK) return rc;
    memcpy(h->h_stage, seq, array_bytes(SEQ));
    staged = true;
    return DM_OK;
  }
  char *host_view(const void *p) const { return h->h_stage + ((const char *)p - ar.base); }
  template <typename T> T *stage_ptr(T *p) const { return (T *)(h->d_stage + ((const char *)p - ar.base)); }
  void copy_from_stage() const {
    for (int i = 0; i < 3; i++) memcpy(outs[i].host, host_view(outs[i].dev), outs[i].bytes_per_user * (size_t)U);
  }
  hipError_t upload(const void *seq) const {
    return hipMemcpyAsync(dev[SEQ], staged ? (const void *)h->h_stage : seq, array_bytes(SEQ), hipMemcpyHostToDevice, h->stream);
  }
  hipError_t clear_trace() const {
    if (!trace_external) return hipMemsetAsync(dev[TC], 0, (size_t)(dev[TN] + array_bytes(TN) - dev[TC]), h->stream);
    hipError_t e = hipSuccess;
    for (int a = TC; a <= TN && e == hipSuccess; a++) e = hipMemsetAsync(dev[a], 0, array_bytes(a), h->stream);
    return e;
  }
  // after the search: the download (one block when staged), the synchronize, and the way out of the staging block
  hipError_t finish() const {
    hipError_t e = hipSuccess;
    if (staged) e = hipMemcpyAsync(host_view(dev[IDS]), dev[IDS], (size_t)(dev[COUNTS] + array_bytes(COUNTS) - dev[IDS]), hipMemcpyDeviceToHost, h->stream);
    else for (int i = 0; i < n_outs() && e == hipSuccess; i++) e = hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes_per_user * (size_t)U, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && staged) copy_from_stage();
    return e;
  }
  // single-request path: the kernel reads the request from the host-mapped staging block and writes whole result rows into it,
  // publishing each user's count last.  arm_direct() sets the counts to -1 before the launch; wait_direct() polls them (every 4096
  // spins a look at the stream: idle or failed with counts still missing is a kernel fault) and copies the results out.
  void arm_direct() const {
    volatile int32_t *m_cnt = (volatile int32_t *)host_view(dev[COUNTS]);
    for (int64_t u = 0; u < U; u++) m_cnt[u] = -1;
  }
  int wait_direct(const char *who) const {
    volatile int32_t *m_cnt = (volatile int32_t *)host_view(dev[COUNTS]);
    auto all_in = [&] { bool ok = true; for (int64_t u = 0; u < U; u++) ok = ok && m_cnt[u] >= 0; return ok; };
    for (long spin = 0; !all_in(); spin++)
      if ((spin & 0xFFF) == 0xFFF && hipStreamQuery(h->stream) != hipErrorNotReady) {
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (!all_in()) return fail(h, DM_ERR_HIP, std::string(who) + " (single-request path): " + (e != hipSuccess ? hipGetErrorString(e) : "kernel finished without results"));
      }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    copy_from_stage();
    return DM_OK;
  }
};

// ---- pipelined download of a request cut into chunks of users (host_pipe_plan in dm_hip.hip says why and how).
// fn(k, u0, uk) enqueues the search of chunk k = users [u0, u0 + uk); a chunk k > 0 keeps the scored-rows counter counting
// (keep_rows of the searches).  The first failure stops the launches.  *launched = the chunks whose event was recorded.
template <typename Fn>
static int launch_chunks(dm_ctx *h, int n_chunks, const int64_t *off, Fn fn, int *launched) {
  *launched = 0;
  if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  while ((int)h->chunk_ev.size() < n_chunks) {
    hipEvent_t e;
    HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->chunk_ev.push_back(e);
  }
  int rc = DM_OK;
  for (int k = 0; k < n_chunks && rc == DM_OK; k++) {
    const int64_t u0 = off[k], uk = off[k + 1] - u0;
    if (uk <= 0) break;
    rc = fn(k, u0, uk);
    if (rc == DM_OK && hipEventRecord(h->chunk_ev[(size_t)k], h->stream) != hipSuccess) rc = fail(h, DM_ERR_HIP, "host-buffer search: event record failed");
    if (rc == DM_OK) ++*launched;
  }
  return rc;
}

// downloads the launched chunks, then synchronizes BOTH streams whatever happened; the first HIP error, if any
static hipError_t download_chunks(dm_ctx *h, const HostOut *outs, int n, const int64_t *off, int launched) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < launched && e == hipSuccess; k++) {
    const int64_t u0 = off[k], uk = off[k + 1] - u0;
    e = hipStreamWaitEvent(h->copy_stream, h->chunk_ev[(size_t)k], 0);
    for (int i = 0; i < n && e == hipSuccess; i++) {
      const size_t b = outs[i].bytes_per_user;
      e = hipMemcpyAsync((char *)outs[i].host + (size_t)u0 * b, (const char *)outs[i].dev + (size_t)u0 * b, (size_t)uk * b, hipMemcpyDeviceToHost, h->copy_stream);
    }
  }
  const hipError_t e1 = h->copy_stream ? hipStreamSynchronize(h->copy_stream) : hipSuccess;
  const hipError_t e2 = hipStreamSynchronize(h->stream);
  return e != hipSuccess ? e : e1 != hipSuccess ? e1 : e2;
}
