// Host-request layer (host code only): the mechanisms the host-buffer beam-search front ends share (tdm_search_host, otm_search_host in
// dm_hip.hip, otm64_search_host in otm64.hip.inc) and the event pair around one launch.  A front end states its own policy — which
// requests are staged, served in place or cut into chunks — and calls these.

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
// 40 .. 43 mean two things: the grouped fp64 training step of a DIN model and the serving / tree-learning launches of a DeepFM model (a
// handle holds one).
enum EvKind {
  EV_MAIN = 0,            // a search's main kernel, a whole Deep-Retrieval search, and every launch nobody asks for by kind
  EV_DEFERRED = 1,        // the second pass over the users the one-wave-per-SIMD beam kernel deferred
  EV_DR_STATS = 10, EV_DR_CUT = 11, EV_DR_BLOCK = 21,
  EV_ROWS = 30,           // general rows (rows_kernel.hip.inc)
  EV_DFM_USER = 40, EV_DFM_LEVEL = 41,
  EV_DFM_JTM_ROWS = 42, EV_DFM_JTM_PAIRS = 43,      // the pair scorer of JTM tree learning (dfm_jtm.hip.inc): per-history set-up, per-pair score
  EV_DFM_OTM = 42,        // the fused OTM beam search of a DeepFM model (dfm_otm.hip.inc): a call is a search or a tree-learning step, never both
  EV_TG_SETUP = 40, EV_TG_ROWS = 41, EV_TG_WGRAD_A = 42, EV_TG_USER_BWD = 43, EV_TG_WGRAD_B = 44,
  // the Deep-Retrieval training step under DM_DR_TIME_LAUNCHES=1 (dr_train.hip.inc): forward GEMMs, softmax + cross-entropy, dX products,
  // dW / db products with their slab sums, embedding gradient (pairs, sort, segment sums), Adam
  EV_DRT_FWD = 50, EV_DRT_SOFTMAX = 51, EV_DRT_DX = 52, EV_DRT_DW = 53, EV_DRT_EMB = 54, EV_DRT_ADAM = 55,
  // the rerank model's training step (dr_rerank_train.hip.inc): user-vector GEMM, classes of the rows (sampler), sampled softmax, the
  // softmax tables' gradient (pairs, sort, segment sums), dX, dW / db with their slab sums, embedding gradient, both Adam updates
  // the DeepFM training step under DM_DFM_TIME_LAUNCHES=1 (dfm_train.hip.inc): the fused rows kernel (forward, loss, dH, dX), the l1.W / l1.b
  // product with its slab sum, embedding gradient (pairs, sort, segment sums), Adam
  EV_DFT_ROWS = 70, EV_DFT_DW = 71, EV_DFT_EMB = 72, EV_DFT_ADAM = 73,
  EV_DRR_FWD = 60, EV_DRR_SAMPLE = 61, EV_DRR_SOFTMAX = 62, EV_DRR_SMGRAD = 63, EV_DRR_DX = 64, EV_DRR_DW = 65, EV_DRR_EMB = 66, EV_DRR_ADAM = 67,
  // the Deep-Retrieval M-step's path scores under DM_DR_TIME_LAUNCHES=1 (dr_mstep.hip.inc): pairs of a chunk, the (item, path) sort, segment
  // heads (flags + compaction), segment sums, the sort by score, the sort by item (with its key kernel), the cut at C (flags + compaction),
  // codes / scores / offsets, occurrences.  The searches of the chunks are EV_MAIN, as everywhere
  EV_DRM_PAIRS = 80, EV_DRM_SORT = 81, EV_DRM_HEADS = 82, EV_DRM_SEGSUM = 83, EV_DRM_SCORE_SORT = 84, EV_DRM_ITEM_SORT = 85, EV_DRM_CUT = 86, EV_DRM_EMIT = 87,
  EV_DRM_OCC = 88,
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

// ---- request arena: the device buffers of one host-buffer request, laid out in h->req (grow only, by half again: no hipMalloc /
// hipFree on the request path once the handle has seen its largest request).  add() every buffer, commit(), then ptr<T>(offset).
struct ReqArena : DevArena {
  explicit ReqArena(dm_ctx *h) : DevArena(h->req, 2) {}
};

// ---- one result array of a request: `bytes_per_user` bytes per user at `dev` (in the arena, or a per-call buffer) go to `host`
struct HostOut { void *host; const void *dev; size_t bytes_per_user; };

// plain download: every array on `stream`; the caller synchronizes
static hipError_t download_all(dm_ctx *h, const HostOut *outs, int n, int64_t U, hipStream_t stream) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; i++) e = hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes_per_user * (size_t)U, hipMemcpyDeviceToHost, stream);
  return e;
}

// The pinned staging block (ensure_stage) mirrors the head of the arena: a buffer at arena offset o is staged at h_stage + o, and the
// single-request kernels address it as d_stage + o.
static char *stage_of(const dm_ctx *h, const void *dev) { return h->h_stage + ((const char *)dev - (const char *)h->req.p); }
static void copy_from_stage(const dm_ctx *h, const HostOut *outs, int n, int64_t U) {
  for (int i = 0; i < n; i++) memcpy(outs[i].host, stage_of(h, outs[i].dev), outs[i].bytes_per_user * (size_t)U);
}
// staged download: outs[0] .. outs[n - 1] are adjacent in the arena and come down as ONE block; the caller synchronizes, then copy_from_stage()
static hipError_t download_staged(dm_ctx *h, const HostOut *outs, int n, int64_t U) {
  const char *first = (const char *)outs[0].dev, *end = (const char *)outs[n - 1].dev + outs[n - 1].bytes_per_user * (size_t)U;
  return hipMemcpyAsync(stage_of(h, first), first, (size_t)(end - first), hipMemcpyDeviceToHost, h->stream);
}

// ---- single-request path: the kernel writes whole result rows into the host-mapped staging block and publishes each user's count
// last; the caller has set the counts to -1 and launched.  Polls the counts; every 4096 spins a look at the stream: idle (or failed)
// with counts still missing is a kernel fault.
static int wait_host_direct(dm_ctx *h, volatile int32_t *m_cnt, int64_t U, const char *who) {
  auto all_in = [&] { bool ok = true; for (int64_t u = 0; u < U; u++) ok = ok && m_cnt[u] >= 0; return ok; };
  for (long spin = 0; !all_in(); spin++)
    if ((spin & 0xFFF) == 0xFFF && hipStreamQuery(h->stream) != hipErrorNotReady) {
      const hipError_t e = hipStreamSynchronize(h->stream);
      if (!all_in()) return fail(h, DM_ERR_HIP, std::string(who) + " (single-request path): " + (e != hipSuccess ? hipGetErrorString(e) : "kernel finished without results"));
    }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return DM_OK;
}

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
