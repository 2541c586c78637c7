// Host side of the Deep-Retrieval entry points (dm_dr_*), SURVEY.md row A13.  Kernels: dr_kernel.hip.inc.

struct dm_dr_train;
struct dm_dr_rr_train;
struct dm_dr_state;
static void dr_train_release(dm_dr_state *s);
static void dr_rr_train_release(dm_dr_state *s);
struct dm_dr_state {
  bool loaded = false, has_rerank = false, paths_loaded = false;
  bool exact_only = false;            // DM_DR_EXACT_ONLY=1 at load time: always take the radix-select path (debugging)
  int dtype = DM_F32, E = 0, L = 0, K = 0, D = 0;
  int64_t num_item = 0;
  // the layer model as ONE vector [layer_emb ; W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}] (what dm_dr_adam_step moves); d_layer_emb, d_w and
  // d_b point into it.  Everything below d_zero is derived from it (dr_derive) and goes stale when it moves
  void *d_par = nullptr;
  int64_t n_par = 0;
  void *d_w[DR_MAXD] = {}, *d_b[DR_MAXD] = {};   // W_d [K x (L+d)E] with its node columns, b_d [K]
  bool derived_stale = false;        // dm_dr_adam_step moved the weights: dr_check_search derives again before the next search
  bool wseq_stale = false;           // ... and the training step refreshes d_wseq alone (its dX product reads it)
  bool x_refused = false;            // the 256 x 256 GEMM's second table copy did not fit at load
  struct dm_dr_train *tr = nullptr;  // dm_dr_train_init (dr_train.hip.inc)
  void *d_layer_emb = nullptr;       // [(num_item + K(D-1)) x E]: the first section of d_par
  void *d_wseq = nullptr;            // [D*K x L*E]: history columns of every layer's Linear
  void *d_sbias = nullptr;           // [D*K]
  void *d_zero = nullptr;            // 64 zero bytes x 4: the row a padding id gathers
  // float models, E % 64 == 0: fp16 hi / lo planes of d_wseq and the power-of-two scales of the split history GEMM
  void *d_wseq_split = nullptr;
  void *d_wseq_stages = nullptr, *d_emb_stages = nullptr;      // the 256 x 256 split GEMM's operands (dr_split_stages / dr_split_rows_kernel)
  int64_t x_min_rows = 0;                                      // DM_DR_GEMM_X_MIN_ROWS: a fixed switch-over batch size instead of dr_gemm_x_pays()
  int sh_a = 0, sh_b = 0;
  void *d_tabs[DR_MAXD * (DR_MAXD - 1) / 2] = {};   // T_{d,t} [K x K]
  void *d_rowmax[DR_MAXD * (DR_MAXD - 1) / 2] = {}; // max_k T_{d,t}[node][k] (the column-sliced search, dr_sliced.hip.inc)
  void *d_etabs[DR_MAXD * (DR_MAXD - 1) / 2] = {};  // exp(T_{d,t}[node][k] - rowmax[node])
  bool sliced = true;                 // DM_DR_SLICED=0 at load time keeps the one-workgroup-per-user kernel
  int64_t sliced_min = 512;           // batches below this take the single launch (DM_DR_SLICED_MIN_USERS: tests run the sliced path on tiny batches)
  DevGrow state;                                     // layer state + partial statistics of the sliced search
  // the rerank model as TWO vectors, one per optimizer (dm_dr_rerank_adam_step, dr_rerank_train.hip.inc): the graph's
  // [rerank_emb ; rerank_w ; rerank_b] and the criterion's [softmax_w ; softmax_b].  The five pointers below point into them; the
  // rerank path keeps no derived copies, so serving reads the trained bytes as they are
  void *d_rr_par = nullptr, *d_sm_par = nullptr;
  void *d_rr_emb = nullptr, *d_rr_w = nullptr, *d_rr_b = nullptr, *d_sm_w = nullptr, *d_sm_b = nullptr;
  struct dm_dr_rr_train *rt = nullptr;  // dm_dr_rerank_train_init
  // path -> items
  int64_t P = 0;
  int max_bucket = 0;
  long long *d_codes = nullptr;
  int64_t *d_item_off = nullptr;
  int32_t *d_items = nullptr;
  int64_t n_path_items = 0;                         // entries of d_items (dm_dr_path_items_size)
  // the resident item -> paths table [num_item x J x D] and training set (dr_train_set.hip.inc): seq [N x L], targets [N], order [N]
  int J = 0;
  int32_t *d_item_paths = nullptr;
  int64_t ts_N = 0;
  int32_t *d_ts_seq = nullptr, *d_ts_tgt = nullptr, *d_ts_order = nullptr;
  DevGrow ts_ws;                                    // the sorts of the CSR build and of the shuffle
  // scratch (grow only)
  DevGrow S, UV, io, cand;                          // io: seq ids + paths + probs + counts + outputs of one chunk
  DevGrow ms, ms_io;                                // the M-step's path scores (dr_mstep.hip.inc): every array of a call; the host entry's uploads
};

static void dm_dr_free(dm_dr_state *s) {
  if (!s) return;
  dr_train_release(s);
  dr_rr_train_release(s);
  s->d_layer_emb = nullptr;
  dm_release(s->d_par, s->d_wseq, s->d_sbias, s->d_zero, s->d_wseq_split, s->d_wseq_stages, s->d_emb_stages);
  for (auto *v : {&s->d_tabs, &s->d_rowmax, &s->d_etabs})
    for (auto &t : *v) dm_release(t);
  s->d_rr_emb = s->d_rr_w = s->d_rr_b = s->d_sm_w = s->d_sm_b = nullptr;
  dm_release(s->d_rr_par, s->d_sm_par, s->d_codes, s->d_item_off, s->d_items);
  dm_release(s->d_item_paths, s->d_ts_seq, s->d_ts_tgt, s->d_ts_order);
  for (DevGrow *g : {&s->state, &s->S, &s->UV, &s->io, &s->cand, &s->ms, &s->ms_io, &s->ts_ws}) g->release();
  delete s;
}

template <typename T>
static int dr_launch_gemm(dm_ctx *h, const DrGemmParams<T> &p, bool on = true) {
  if (p.M <= 0 || p.N <= 0) return DM_OK;
  dim3 grid((unsigned)((p.N + DR_TN - 1) / DR_TN), (unsigned)((p.M + DR_TM - 1) / DR_TM));
  return timed(h, EV_MAIN, on, [&] { return LAUNCH(h, dr_gemm_kernel<T>, grid, dim3(256), 0, p); });
}
// A search is several launches (history GEMM, layer 0, statistics and cut per layer).  An event pair around EACH of them (what
// dm_kernel_timing_get_kind reports by kind) drains the GPU between two kernels: measured 0.39 -> 0.32 ms per 1 024 users, 0.63 -> 0.55 per
// 4 096, 2.12 -> 2.07 per 16 384 without them — back-to-back kernels overlap their tails.  So by default ONE pair brackets the whole
// search (EV_MAIN: its device time), and the per-launch pairs are recorded only under DM_DR_TIME_LAUNCHES=1 (read per call: bench.py and
// tools/dr_bench.py time the search without, then run a breakdown pass with).
static inline bool dr_time_launches() { return env_on("DM_DR_TIME_LAUNCHES"); }

// the history columns of every layer, [D*K x L*E], out of the W_d (the training step refreshes these alone: its dX product reads them)
template <typename T>
static int dr_refresh_wseq(dm_ctx *h, dm_dr_state *s) {
  const int E = s->E, L = s->L, K = s->K, D = s->D;
  const size_t esz = sizeof(T);
  for (int d = 0; d < D; d++) {
    const size_t cols = (size_t)(L + d) * E;
    HIPCHK(h, hipMemcpy2DAsync((char *)s->d_wseq + (size_t)d * K * L * E * esz, (size_t)L * E * esz, s->d_w[d], cols * esz,
                               (size_t)L * E * esz, K, hipMemcpyDeviceToDevice, h->stream));
  }
  s->wseq_stale = false;
  return DM_OK;
}
#define DR_ALLOC_ONCE(h, ptr, bytes) do { if (!(ptr)) ALLOC(h, ptr, bytes); } while (0)      // dr_derive runs more than once per model

// Everything the search reads that is computed FROM the weights: the history columns d_wseq, the biases d_sbias, the node tables with their
// row maxima and exp tables, the split scales, planes and stage records.  Called after the copy-in of dm_dr_load_model and again (by
// dr_check_search) after the weights moved on the device (dm_dr_adam_step): every buffer is allocated on the first call and refilled on
// the later ones, with the same kernels on the same inputs — a model that was trained here and one loaded from the downloaded weights
// search bit for bit alike.
template <typename T>
static int dr_derive(dm_ctx *h, dm_dr_state *s) {
  const int E = s->E, L = s->L, K = s->K, D = s->D;
  const size_t esz = sizeof(T);
  const int64_t n_emb = (s->num_item + (int64_t)K * (D - 1)) * E;
  int rc;
  DR_ALLOC_ONCE(h, s->d_wseq, (size_t)D * K * L * E * esz);
  DR_ALLOC_ONCE(h, s->d_sbias, (size_t)D * K * esz);
  if ((rc = dr_refresh_wseq<T>(h, s)) != DM_OK) return rc;
  for (int d = 0; d < D; d++) {
    const size_t cols = (size_t)(L + d) * E;
    HIPCHK(h, hipMemcpyAsync((char *)s->d_sbias + (size_t)d * K * esz, s->d_b[d], K * esz, hipMemcpyDeviceToDevice, h->stream));
    for (int t = 0; t < d; t++) {           // T_{d,t}[node][k] = W_d[k, (L+t)E:(L+t+1)E] . emb(num_item + t*K + node)
      void *&tab = s->d_tabs[d * (d - 1) / 2 + t];
      DR_ALLOC_ONCE(h, tab, ((size_t)K * K + 1024) * esz);          // +1024: the beam kernel reads whole 64-wide chunks past a row's end
      HIPCHK(h, hipMemsetAsync((char *)tab + (size_t)K * K * esz, 0, 1024 * esz, h->stream));
      DrGemmParams<T> g{};
      g.A = (const T *)s->d_layer_emb + (s->num_item + (int64_t)t * K) * E; g.lda = E;
      g.gidx = nullptr; g.Lg = 0; g.E = E;
      g.B = (const T *)s->d_w[d] + (size_t)(L + t) * E; g.ldb = (int64_t)cols;
      g.bias = nullptr; g.zero = (const T *)s->d_zero;
      g.C = (T *)tab; g.ldc = K;
      g.M = K; g.N = K; g.Kd = E;
      if ((rc = dr_launch_gemm<T>(h, g)) != DM_OK) return rc;
      void *&rm = s->d_rowmax[d * (d - 1) / 2 + t];
      DR_ALLOC_ONCE(h, rm, (size_t)K * esz);
      if ((rc = LAUNCH(h, drs_rowmax_kernel<T>, dim3(256), dim3(256), 0, (const T *)tab, K, (T *)rm)) != DM_OK) return rc;
      void *&et = s->d_etabs[d * (d - 1) / 2 + t];
      DR_ALLOC_ONCE(h, et, ((size_t)K * K + 1024) * esz);
      HIPCHK(h, hipMemsetAsync((char *)et + (size_t)K * K * esz, 0, 1024 * esz, h->stream));
      if ((rc = LAUNCH(h, drs_exptab_kernel<T>, dim3(1024), dim3(256), 0, (const T *)tab, (const T *)rm, K, (T *)et)) != DM_OK) return rc;
    }
  }
  if (sizeof(T) == 4 && E % 64 == 0) {       // (the split GEMM stages 64-column tiles: a tile never straddles an embedding row)
    // split-fp16 history GEMM (dm_set_scorer_mode): scales from the largest magnitudes, W planes built once per set of weights
    if (!h->lazy.d_maxabs) ALLOC(h, h->lazy.d_maxabs, 8);
    HIPCHK(h, hipMemsetAsync(h->lazy.d_maxabs, 0, 8, h->stream));
    if ((rc = LAUNCH(h, dm_maxabs_kernel<false>, dim3(4096), dim3(256), 0, (const float *)s->d_layer_emb, nullptr, n_emb, 0, h->lazy.d_maxabs)) != DM_OK ||
        (rc = LAUNCH(h, dm_maxabs_kernel<false>, dim3(256), dim3(256), 0, (const float *)s->d_wseq, nullptr, (int64_t)D * K * L * E, 0, h->lazy.d_maxabs + 1)) != DM_OK)
      return rc;
    unsigned mb[2];
    HIPCHK(h, hipMemcpyAsync(mb, h->lazy.d_maxabs, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    s->sh_a = split_shift(mb[0]); s->sh_b = split_shift(mb[1]);
    DR_ALLOC_ONCE(h, s->d_wseq_split, (size_t)2 * D * K * L * E * 2);
    if ((rc = LAUNCH(h, dr_split_planes_kernel, dim3(1024), dim3(256), 0, (const float *)s->d_wseq, (int64_t)D * K * L * E, ldexpf(1.0f, s->sh_b),
                     (_Float16 *)s->d_wseq_split)) != DM_OK) return rc;
  }
  if (sizeof(T) == 4 && s->d_wseq_split && L <= DR_X_MAXL) {
    // operands of the 256 x 256 history GEMM: a second copy of the embedding rows (4 E bytes per row, as the fp32 table) and of the
    // history columns, as 128-byte hi/lo records.  An optimisation, allocated after everything the model needs: when the memory is not
    // there the model keeps the 128 x 128 kernel for every batch size
    if (const long long v_ = env_int("DM_DR_GEMM_X_MIN_ROWS")) s->x_min_rows = v_;
    if (!env_off("DM_DR_GEMM_X") && !s->x_refused) {      // "0": keep the 128 x 128 kernel (and save the second table copy)
      const std::string err0 = h->err;           // (an optimisation that does not fit leaves no trace, not even a last-error string)
      if ((!s->d_emb_stages && dm_alloc(h, &s->d_emb_stages, (size_t)n_emb * 4) != DM_OK) ||
          (!s->d_wseq_stages && dm_alloc(h, &s->d_wseq_stages, (size_t)D * K * L * E * 4) != DM_OK)) {
        (void)hipGetLastError();
        dm_release(s->d_emb_stages, s->d_wseq_stages);
        s->x_refused = true;                     // (a later derive of the same model does not try again)
        h->err = err0;
      } else {
        if ((rc = LAUNCH(h, dr_split_rows_kernel, dim3(8192), dim3(256), 0, (const float *)s->d_layer_emb, n_emb / E, E, ldexpf(1.0f, s->sh_a),
                         (_Float16 *)s->d_emb_stages)) != DM_OK ||
            (rc = LAUNCH(h, dr_split_stages_kernel, dim3(1024), dim3(256), 0, (const float *)s->d_wseq, D * K, L * E, ldexpf(1.0f, s->sh_b),
                         (_Float16 *)s->d_wseq_stages)) != DM_OK) return rc;
      }
    }
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  s->derived_stale = false;
  return DM_OK;
}

// number of elements of the trainable vector [layer_emb ; W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}] (LayerModel.scala:22-39)
static int64_t dr_param_count(int64_t num_item, int K, int D, int L, int E) {
  int64_t n = (num_item + (int64_t)K * (D - 1)) * E;
  for (int d = 0; d < D; d++) n += (int64_t)K * (L + d) * E + K;
  return n;
}

template <typename T>
static int dr_load_model_t(dm_ctx *h, const dm_dr_model *m) {
  dm_dr_state *s = new dm_dr_state();
  dm_dr_free(h->dr); h->dr = s;          // (drops the training state of the model that was there)
  const int E = m->embed, L = m->seq_len, K = m->num_node, D = m->num_layer;
  const bool dev = m->on_device != 0;
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  s->dtype = m->dtype; s->E = E; s->L = L; s->K = K; s->D = D; s->num_item = m->num_item;
  s->exact_only = env_str("DM_DR_EXACT_ONLY") != nullptr;
  if (env_off("DM_DR_SLICED")) s->sliced = false;
  if (const long long v_ = env_int("DM_DR_SLICED_MIN_USERS")) s->sliced_min = v_;
  const size_t esz = sizeof(T);
  const int64_t n_emb = (m->num_item + (int64_t)K * (D - 1)) * E;    // LayerModel.scala:24
  // ---- copy-in: ONE vector holds the layer model, in the order Adam sees it; the table the search gathers from is its first section
  s->n_par = dr_param_count(m->num_item, K, D, L, E);
  ALLOC(h, s->d_par, (size_t)s->n_par * esz);
  s->d_layer_emb = s->d_par;
  HIPCHK(h, hipMemcpyAsync(s->d_par, m->layer_emb, (size_t)n_emb * esz, kind, h->stream));
  int64_t off = n_emb;
  for (int d = 0; d < D; d++) {
    const int64_t nw = (int64_t)K * (L + d) * E;
    s->d_w[d] = (char *)s->d_par + (size_t)off * esz; s->d_b[d] = (char *)s->d_par + (size_t)(off + nw) * esz;
    HIPCHK(h, hipMemcpyAsync(s->d_w[d], m->layer_w[d], (size_t)nw * esz, kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_b[d], m->layer_b[d], (size_t)K * esz, kind, h->stream));
    off += nw + K;
  }
  const size_t zero_bytes = (size_t)4 * E * esz > 4096 ? (size_t)4 * E * esz : 4096;   // the 256 x 256 split GEMM steps through a zero block as long as a
  ALLOC(h, s->d_zero, zero_bytes);                                                     // row's records (4 E bytes); the other GEMMs read one row of E values
  HIPCHK(h, hipMemsetAsync(s->d_zero, 0, zero_bytes, h->stream));
  int rc;
  if (m->rerank_emb) {
    const size_t n_emb_rr = (size_t)m->num_item * E, n_w = (size_t)E * L * E;
    ALLOC(h, s->d_rr_par, (n_emb_rr + n_w + E) * esz);
    ALLOC(h, s->d_sm_par, (n_emb_rr + (size_t)m->num_item) * esz);
    s->d_rr_emb = s->d_rr_par; s->d_rr_w = (char *)s->d_rr_par + n_emb_rr * esz; s->d_rr_b = (char *)s->d_rr_w + n_w * esz;
    s->d_sm_w = s->d_sm_par; s->d_sm_b = (char *)s->d_sm_par + n_emb_rr * esz;
    HIPCHK(h, hipMemcpyAsync(s->d_rr_emb, m->rerank_emb, n_emb_rr * esz, kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_rr_w, m->rerank_w, n_w * esz, kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_rr_b, m->rerank_b, (size_t)E * esz, kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_sm_w, m->softmax_w, n_emb_rr * esz, kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_sm_b, m->softmax_b, (size_t)m->num_item * esz, kind, h->stream));
    s->has_rerank = true;
  }
  if ((rc = dr_derive<T>(h, s)) != DM_OK) return rc;
  h->ev_used = 0;
  s->loaded = true;
  return DM_OK;
}

int dm_dr_load_model(dm_handle_t h, const dm_dr_model *m) {
  if (!h) return DM_ERR_INVALID;
  if (!m || !m->layer_emb || !m->layer_w || !m->layer_b)
    return fail(h, DM_ERR_INVALID, "dm_dr_load_model: null argument");
  if (m->dtype != DM_F32 && m->dtype != DM_F64) return fail(h, DM_ERR_INVALID, "dm_dr_load_model: dtype must be DM_F32 or DM_F64");
  if (m->num_layer < 2) return fail(h, DM_ERR_INVALID, "number of layers must be at least 2");   // LayerModel.scala:12
  if (m->num_layer > DR_MAXD) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_load_model: at most 4 layers");
  if (m->embed < 16 || m->embed % 16) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_load_model: embed size must be a multiple of 16");
  if (m->seq_len < 1 || m->num_node < 1 || m->num_item < 1) return fail(h, DM_ERR_INVALID, "dm_dr_load_model: bad sizes");
  {
    double space = 1;
    for (int d = 0; d < m->num_layer; d++) space *= (double)m->num_node;
    if (space > 4.0e18) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_load_model: num_node^num_layer must fit 62 bits");
  }
  for (int d = 0; d < m->num_layer; d++)
    if (!m->layer_w[d] || !m->layer_b[d]) return fail(h, DM_ERR_INVALID, "dm_dr_load_model: null layer weights");
  const bool any_rr = m->rerank_emb || m->rerank_w || m->rerank_b || m->softmax_w || m->softmax_b;
  const bool all_rr = m->rerank_emb && m->rerank_w && m->rerank_b && m->softmax_w && m->softmax_b;
  if (any_rr && !all_rr) return fail(h, DM_ERR_INVALID, "dm_dr_load_model: give all five rerank arrays or none");
  HIPCHK(h, hipSetDevice(h->device));
  return m->dtype == DM_F32 ? dr_load_model_t<float>(h, m) : dr_load_model_t<double>(h, m);
}

int dm_dr_load_path_items(dm_handle_t h, const int32_t *path_nodes, int64_t n_paths, const int64_t *item_off,
                          const int32_t *items) {
  if (!h) return DM_ERR_INVALID;
  dm_dr_state *s = h->dr;
  if (!s || !s->loaded) return fail(h, DM_ERR_STATE, "dm_dr_load_path_items: load the model first");
  if (n_paths < 0 || (n_paths > 0 && (!path_nodes || !item_off || !items)))
    return fail(h, DM_ERR_INVALID, "dm_dr_load_path_items: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  const int D = s->D, K = s->K;
  std::vector<std::pair<long long, int64_t>> order((size_t)n_paths);
  for (int64_t i = 0; i < n_paths; i++) {
    long long code = 0;
    for (int d = 0; d < D; d++) {
      const int32_t v = path_nodes[i * D + d];
      if (v < 0 || v >= K) return fail(h, DM_ERR_INDEX, "dm_dr_load_path_items: path node outside [0, num_node)");
      code = code * K + v;
    }
    if (item_off[i + 1] < item_off[i]) return fail(h, DM_ERR_INVALID, "dm_dr_load_path_items: item_off must be non-decreasing");
    order[(size_t)i] = {code, i};
  }
  std::sort(order.begin(), order.end());
  for (int64_t i = 1; i < n_paths; i++)
    if (order[(size_t)i].first == order[(size_t)i - 1].first)
      return fail(h, DM_ERR_INVALID, "dm_dr_load_path_items: duplicate path (a Map has one entry per key)");
  std::vector<long long> codes((size_t)n_paths);
  std::vector<int64_t> off((size_t)n_paths + 1, 0);
  const int64_t n_items = n_paths ? item_off[n_paths] - item_off[0] : 0;
  std::vector<int32_t> its((size_t)n_items);
  int64_t mb = 0;
  for (int64_t i = 0; i < n_paths; i++) {
    const int64_t src = order[(size_t)i].second;
    const int64_t c = item_off[src + 1] - item_off[src];
    codes[(size_t)i] = order[(size_t)i].first;
    for (int64_t e = 0; e < c; e++) {
      const int32_t it = items[item_off[src] + e];
      if (it < 0 || it >= s->num_item) return fail(h, DM_ERR_INDEX, "dm_dr_load_path_items: item id outside [0, num_item)");
      its[(size_t)(off[(size_t)i] + e)] = it;
    }
    off[(size_t)i + 1] = off[(size_t)i] + c;
    if (c > mb) mb = c;
  }
  dm_release(s->d_codes, s->d_item_off, s->d_items);
  s->paths_loaded = false;
  ALLOC(h, s->d_codes, (size_t)n_paths * 8);
  ALLOC(h, s->d_item_off, ((size_t)n_paths + 1) * 8);
  ALLOC(h, s->d_items, (size_t)n_items * 4);
  HIPCHK(h, hipMemcpy(s->d_codes, codes.data(), (size_t)n_paths * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(s->d_item_off, off.data(), ((size_t)n_paths + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(s->d_items, its.data(), (size_t)n_items * 4, hipMemcpyHostToDevice));
  s->P = n_paths; s->n_path_items = n_items; s->max_bucket = (int)mb; s->paths_loaded = true;
  return DM_OK;
}

static int dr_pow2_ge(int v) { int n = 1; while (n < v) n <<= 1; return n; }

// beam search for users already on the device; d_paths [U][beam][D], d_probs [U][beam] (double), d_counts [U]
template <typename T>
static int dr_beam_dev_t(dm_ctx *h, const int32_t *d_seq, int64_t U, int beam, int32_t *d_paths, double *d_probs,
                         int32_t *d_counts) {
  dm_dr_state *s = h->dr;
  const int K = s->K, D = s->D, L = s->L, E = s->E;
  const int n2 = dr_pow2_ge(beam);
  const size_t lds = dr_beam_lds((int)sizeof(T), K, D, n2);
  if (lds > 160 * 1024) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_beam_search: num_node / beam too large for LDS");
  const int64_t chunk = 32768;
  int rc = s->S.reserve(h, ((size_t)(U < chunk ? U : chunk) * D * K + 64) * sizeof(T));      // + slack: the sliced search reads 8 columns at a time
  if (rc != DM_OK) return rc;
  if (sizeof(T) == 4 && !s->d_wseq_split && h->scorer_mode == DM_SCORER_SPLIT_F16)      // asked for by name: say so instead of quietly running fp32
    return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_beam_search: the split-fp16 history GEMM needs embed_size % 64 == 0 (this model: fp32 GEMM; use DM_SCORER_AUTO or DM_SCORER_F32)");
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t n = U - u0 < chunk ? U - u0 : chunk;
    const bool detail = dr_time_launches();
    rc = timed(h, EV_MAIN, !detail, [&]() -> int {      // the one pair around the whole search, whichever route it takes
      DrGemmParams<T> g{};
      g.A = (const T *)s->d_layer_emb; g.lda = 0; g.gidx = d_seq + u0 * L; g.Lg = L; g.E = E;
      g.B = (const T *)s->d_wseq; g.ldb = (int64_t)L * E; g.bias = (const T *)s->d_sbias; g.zero = (const T *)s->d_zero;
      g.C = (T *)s->S.p; g.ldc = (int64_t)D * K; g.M = n; g.N = D * K; g.Kd = L * E;
      if (sizeof(T) == 4 && s->d_wseq_split && h->scorer_mode != DM_SCORER_F32) {
        DrGemmSplitParams q{};
        q.emb = (const float *)s->d_layer_emb; q.gidx = g.gidx; q.Lg = L; q.E = E;
        q.Bp = (const _Float16 *)s->d_wseq_split; q.bias = (const float *)s->d_sbias; q.zero = (const float *)s->d_zero;
        q.C = (float *)s->S.p; q.ldc = g.ldc; q.M = n; q.N = D * K; q.Kd = L * E;
        q.a_scale = ldexpf(1.0f, s->sh_a); q.c_unscale = ldexpf(1.0f, -(s->sh_a + s->sh_b));
        q.embp = (const _Float16 *)s->d_emb_stages; q.Bt = (const _Float16 *)s->d_wseq_stages; q.zeroh = (const _Float16 *)s->d_zero;
        const bool x = s->d_emb_stages && L <= DR_X_MAXL && (s->x_min_rows > 0 ? n >= s->x_min_rows : dr_gemm_x_pays(n, q.N, h->n_cu));
        const dim3 grid((unsigned)((q.N + DR_TN - 1) / DR_TN), (unsigned)((q.M + DR_TM - 1) / DR_TM));
        rc = timed(h, EV_MAIN, detail, [&] {
          return x ? LAUNCH(h, dr_gemm_split_x_kernel, dim3(dr_gemm_x_grid(q.M, q.N)), dim3(512), 0, q) : LAUNCH(h, dr_gemm_split_kernel, grid, dim3(256), 0, q);
        });
        if (rc != DM_OK) return rc;
      } else if ((rc = dr_launch_gemm<T>(h, g, detail)) != DM_OK) return rc;
      DrBeamParams<T> p{};
      p.S = (const T *)s->S.p;
      for (int i = 0; i < DR_MAXD * (DR_MAXD - 1) / 2; i++) p.tabs[i] = (const T *)s->d_tabs[i];
      p.K = K; p.D = D; p.beam = beam; p.n2 = n2; p.U = n;
      p.fast = dr_beam_fast_ok(K, n2) && !s->exact_only ? 1 : 0; p.nl = dr_beam_nl(K, n2);
      p.slow_count = &h->d_ctr->dr_slow;
      p.phase = h->d_phase;
      p.out_paths = d_paths + u0 * beam * D; p.out_probs = d_probs + u0 * beam; p.out_counts = d_counts + u0;
      const int64_t max_grid = (int64_t)h->n_cu * 8;
      const unsigned grid = (unsigned)(n < max_grid ? n : max_grid);
      if (s->sliced && p.fast && K <= DRS_W * DRS_NS && n2 <= 64 && D <= DR_MAXD && n >= s->sliced_min) {      // (small batches: one launch beats five)
        // column-sliced search (dr_sliced.hip.inc): layer 0, then per layer a statistics launch over (user, path, slice) and a cut
        // launch over users; state and partial statistics in one grow-only block
        const size_t b_nodes = DevArena::up((size_t)n * beam * D * 4), b_prob = DevArena::up((size_t)n * beam * sizeof(T)), b_np = DevArena::up((size_t)n * 4);
        const size_t b_smax = DevArena::up((size_t)n * D * sizeof(T)), b_ps = DevArena::up((size_t)n * beam * DRS_NS * sizeof(T)), b_pb = DevArena::up((size_t)n * beam * 64 * sizeof(T));
        const size_t b_es = DevArena::up(((size_t)n * D * K + 64) * sizeof(T));
        if ((rc = s->state.reserve(h, 2 * (b_nodes + b_prob + b_np) + b_smax + b_ps + b_pb + b_es + b_np)) != DM_OK) return rc;
        char *w = (char *)s->state.p;
        int32_t *nodes[2]; T *pprob[2]; int32_t *npv[2];
        for (int i = 0; i < 2; i++) { nodes[i] = (int32_t *)w; w += b_nodes; pprob[i] = (T *)w; w += b_prob; npv[i] = (int32_t *)w; w += b_np; }
        DrsParams<T> q{};
        q.S = p.S; q.K = K; q.D = D; q.beam = beam; q.n2 = n2; q.nl = p.nl; q.U = n;
        for (int i = 0; i < DR_MAXD * (DR_MAXD - 1) / 2; i++) { q.tabs[i] = (const T *)s->d_tabs[i]; q.rowmax[i] = (const T *)s->d_rowmax[i]; q.etabs[i] = (const T *)s->d_etabs[i]; }
        q.smax = (T *)w; w += b_smax; q.part_s = (T *)w; w += b_ps; q.part_bmax = (T *)w; w += b_pb; q.ES = (T *)w; w += b_es; q.todo = (int32_t *)w;
        q.out_paths = p.out_paths; q.out_probs = p.out_probs; q.out_counts = p.out_counts; q.slow_count = p.slow_count;
        q.nodes_n = nodes[0]; q.pprob_n = pprob[0]; q.np_n = npv[0]; q.last = D == 1 ? 1 : 0;
        // under DM_DR_TIME_LAUNCHES every launch gets its own event pair; dm_kernel_timing_get_kind: EV_DR_CUT = layer 0, EV_DR_STATS + 2 d =
        // statistics of layer d, EV_DR_CUT + 2 d = its cut, EV_DR_BLOCK + 2 d = the block version's pass over the users the one-wave version
        // flagged (the history GEMM is EV_MAIN, like the single kernel of the other route)
        {
          const bool wave0 = !env_on("DM_DR_LAYER0_BLOCK");       // A/B switch: the block version (dr_beam_layer<T, 0>) for everybody
          q.only_todo = 0;
          if (wave0) {
            HIPCHK(h, hipMemsetAsync(q.todo, 0, (size_t)n * 4, h->stream));
            if ((rc = timed(h, EV_DR_CUT, detail, [&] { return LAUNCH(h, drs_layer0_wave_kernel<T>, dim3((unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)h->n_cu * 8)), dim3(256), 0, q); })) != DM_OK) return rc;
            q.only_todo = 1;                                      // the users the one-wave version flagged
          }
          HIPCHK(h, lds_opt_in(drs_layer0_kernel<T>, lds));      // (a host call: ahead of the event pair, not inside it)
          if ((rc = timed(h, wave0 ? EV_DR_BLOCK : EV_DR_CUT, detail, [&] { return LAUNCH(h, drs_layer0_kernel<T>, dim3(grid), dim3(DR_NT), lds, p, q); })) != DM_OK) return rc;
          q.only_todo = 0;
        }
        const size_t lds_sel = drs_select_lds((int)sizeof(T), D, n2, p.nl);
        const unsigned g_stats = (unsigned)(DRS_NS * h->n_cu);
        int cur = 0;
        for (int d = 1; d < D; d++) {
          q.nodes = nodes[cur]; q.pprob = pprob[cur]; q.np = npv[cur];
          q.nodes_n = nodes[cur ^ 1]; q.pprob_n = pprob[cur ^ 1]; q.np_n = npv[cur ^ 1]; q.last = d == D - 1 ? 1 : 0;
          // the cut: one wave per user when the block scores fit its registers (beam <= 64), the few users it flags redone by the block
          // version; DM_DR_SELECT_BLOCK=1 keeps the block version for everybody (A/B switch)
          const bool wave_cut = n2 <= 64 && !env_on("DM_DR_SELECT_BLOCK");
          const size_t lds_selw = 4 * ((drs_selw_lds_per_wave((int)sizeof(T), D, n2, p.nl) + 15) & ~(size_t)15);
          const unsigned g_selw = (unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)h->n_cu * 16);
          if (wave_cut) HIPCHK(h, hipMemsetAsync(q.todo, 0, (size_t)n * 4, h->stream));
#define DRS_LAYER(NT) \
          do { \
            HIPCHK(h, lds_opt_in(drs_select_kernel<T, NT>, lds_sel)); \
            if (wave_cut) HIPCHK(h, lds_opt_in(drs_select_wave_kernel<T, NT>, lds_selw)); \
            if ((rc = timed(h, EV_DR_STATS + 2 * d, detail, [&] { return LAUNCH(h, (drs_stats_kernel<T, NT>), dim3(g_stats), dim3(256), 0, q, d); })) != DM_OK) return rc; \
            q.only_todo = 0; \
            if (wave_cut) { \
              if ((rc = timed(h, EV_DR_CUT + 2 * d, detail, [&] { return LAUNCH(h, (drs_select_wave_kernel<T, NT>), dim3(g_selw), dim3(256), lds_selw, q, d); })) != DM_OK) return rc; \
              q.only_todo = 1; \
            } \
            if ((rc = timed(h, (wave_cut ? EV_DR_BLOCK : EV_DR_CUT) + 2 * d, detail, [&] { return LAUNCH(h, (drs_select_kernel<T, NT>), dim3(grid), dim3(DR_NT), lds_sel, q, d); })) != DM_OK) return rc; \
          } while (0)
          switch (d) {
            case 1: DRS_LAYER(1); break;
            case 2: DRS_LAYER(2); break;
            default: DRS_LAYER(3); break;
          }
#undef DRS_LAYER
          cur ^= 1;
        }
        return DM_OK;
      }
      HIPCHK(h, D <= 3 ? lds_opt_in(dr_beam_kernel<T, 3>, lds) : lds_opt_in(dr_beam_kernel<T, DR_MAXD>, lds));
      return timed(h, EV_MAIN, detail, [&] {
        return D <= 3 ? LAUNCH(h, (dr_beam_kernel<T, 3>), dim3(grid), dim3(DR_NT), lds, p) : LAUNCH(h, (dr_beam_kernel<T, DR_MAXD>), dim3(grid), dim3(DR_NT), lds, p);
      });
    });
    if (rc != DM_OK) return rc;
  }
  return DM_OK;
}

static int dr_check_search(dm_ctx *h, const char *who, int64_t U, int beam, bool need_rerank) {
  dm_dr_state *s = h->dr;
  if (!s || !s->loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": Deep-Retrieval model not loaded");
  if (need_rerank && !s->has_rerank) return fail(h, DM_ERR_STATE, std::string(who) + ": model was loaded without rerank arrays");
  if (need_rerank && !s->paths_loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": path -> items table not loaded");
  if (U < 0 || beam < 1 || beam > 2048) return fail(h, DM_ERR_INVALID, std::string(who) + ": beam must be in [1, 2048]");
  if (s->derived_stale) {               // the weights moved since the tables were built (dm_dr_adam_step): once per search, not per step
    HIPCHK(h, hipSetDevice(h->device));
    return s->dtype == DM_F32 ? dr_derive<float>(h, s) : dr_derive<double>(h, s);
  }
  return DM_OK;
}

int dm_dr_beam_search_dev(dm_handle_t h, const int32_t *d_seq_ids, int64_t U, int beam, int32_t *d_out_paths,
                          double *d_out_probs, int32_t *d_out_counts) {
  if (!h) return DM_ERR_INVALID;
  int rc = dr_check_search(h, "dm_dr_beam_search", U, beam, false);
  if (rc != DM_OK) return rc;
  if (U == 0) return DM_OK;
  if (!d_seq_ids || !d_out_paths || !d_out_probs || !d_out_counts) return fail(h, DM_ERR_INVALID, "dm_dr_beam_search: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  return h->dr->dtype == DM_F32 ? dr_beam_dev_t<float>(h, d_seq_ids, U, beam, d_out_paths, d_out_probs, d_out_counts)
                                : dr_beam_dev_t<double>(h, d_seq_ids, U, beam, d_out_paths, d_out_probs, d_out_counts);
}

static int dr_check_ids(dm_ctx *h, const int32_t *seq, int64_t n) {
  const int64_t ni = h->dr->num_item;
  for (int64_t i = 0; i < n; i++)
    if (seq[i] < -1 || seq[i] >= ni) return fail(h, DM_ERR_INDEX, "Deep-Retrieval: sequence id outside [-1, num_item)");
  return DM_OK;
}

int dm_dr_beam_search(dm_handle_t h, const int32_t *seq_ids, int64_t U, int beam, int32_t *out_paths, double *out_probs,
                      int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  int rc = dr_check_search(h, "dm_dr_beam_search", U, beam, false);
  if (rc != DM_OK) return rc;
  if (U == 0) return DM_OK;
  if (!seq_ids || !out_paths || !out_probs || !out_counts) return fail(h, DM_ERR_INVALID, "dm_dr_beam_search: null argument");
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, U * s->L)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ReqLayout lay(h, s->io, 0, U, (size_t)s->L * 4, (size_t)beam, 8, (size_t)s->D);          // ids = paths [U][beam][D], scores = probs
  if ((rc = lay.commit(out_paths, out_probs, out_counts)) != DM_OK) return rc;
  HIPCHK(h, lay.upload(seq_ids));
  if ((rc = dm_dr_beam_search_dev(h, lay.d<int32_t>(lay.SEQ), U, beam, lay.d<int32_t>(lay.IDS), lay.d<double>(lay.SCORES), lay.d<int32_t>(lay.COUNTS))) != DM_OK) return rc;
  HIPCHK(h, lay.finish());
  return DM_OK;
}

template <typename T>
static int dr_recommend_dev_t(dm_ctx *h, const int32_t *d_seq, int64_t U, int beam, int topk, int32_t *d_paths,
                              double *d_probs, int32_t *d_pcounts, int32_t *d_ids, double *d_scores, int32_t *d_counts) {
  dm_dr_state *s = h->dr;
  int rc = dr_beam_dev_t<T>(h, d_seq, U, beam, d_paths, d_probs, d_pcounts);
  if (rc != DM_OK) return rc;
  const int E = s->E, L = s->L;
  if ((rc = s->UV.reserve(h, (size_t)U * E * sizeof(T))) != DM_OK) return rc;
  DrGemmParams<T> g{};                       // RerankModel.inferenceUserVector (RerankModel.scala:54-68)
  g.A = (const T *)s->d_rr_emb; g.lda = 0; g.gidx = d_seq; g.Lg = L; g.E = E;
  g.B = (const T *)s->d_rr_w; g.ldb = (int64_t)L * E; g.bias = (const T *)s->d_rr_b; g.zero = (const T *)s->d_zero;
  g.C = (T *)s->UV.p; g.ldc = E; g.M = U; g.N = E; g.Kd = L * E;
  if ((rc = dr_launch_gemm<T>(h, g)) != DM_OK) return rc;
  const int n2k = dr_pow2_ge(topk);
  const size_t lds = dr_rerank_lds((int)sizeof(T), E, beam, n2k);
  if (lds > 160 * 1024) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_recommend: topk too large for LDS");
  const int64_t cap64 = (int64_t)beam * (s->max_bucket > 0 ? s->max_bucket : 1);
  if (cap64 > (1 << 24)) return fail(h, DM_ERR_UNSUPPORTED, "dm_dr_recommend: beam * largest path bucket exceeds 2^24 candidates");
  const int cap = (int)cap64;
  int64_t grid = (int64_t)h->n_cu * 8;
  if (grid > U) grid = U;
  while (grid > 1 && (size_t)grid * cap * (4 + sizeof(T)) > ((size_t)4 << 30)) grid /= 2;
  if ((rc = s->cand.reserve(h, DevArena::up((size_t)grid * cap * 4) + (size_t)grid * cap * sizeof(T))) != DM_OK) return rc;
  DrRerankParams<T> p{};
  p.paths = d_paths; p.counts = d_pcounts; p.codes = s->d_codes; p.item_off = s->d_item_off; p.items = s->d_items; p.P = s->P;
  p.UV = (const T *)s->UV.p; p.sm_w = (const T *)s->d_sm_w; p.sm_b = (const T *)s->d_sm_b;
  p.K = s->K; p.D = s->D; p.E = E; p.beam = beam; p.topk = topk; p.n2k = n2k; p.cap = cap; p.U = U;
  p.cand = (int32_t *)s->cand.p; p.score = (T *)((char *)s->cand.p + DevArena::up((size_t)grid * cap * 4));
  p.out_ids = d_ids; p.out_scores = d_scores; p.out_counts = d_counts; p.out_ncand = nullptr;
  HIPCHK(h, lds_opt_in(dr_rerank_kernel<T>, lds));
  return timed(h, EV_MAIN, true, [&] { return LAUNCH(h, dr_rerank_kernel<T>, dim3((unsigned)grid), dim3(DR_NT), lds, p); });
}

// scratch for the intermediate paths of a recommend call
static int dr_recommend_dev(dm_ctx *h, const int32_t *d_seq, int64_t U, int beam, int topk, int32_t *d_ids, double *d_scores,
                            int32_t *d_counts) {
  dm_dr_state *s = h->dr;
  const size_t b_paths = DevArena::up((size_t)U * beam * s->D * 4), b_probs = DevArena::up((size_t)U * beam * 8), b_cnt = DevArena::up((size_t)U * 4);
  int rc = ensure_ws(h, b_paths + b_probs + b_cnt);
  if (rc != DM_OK) return rc;
  double *d_probs = (double *)h->ws.p;
  int32_t *d_paths = (int32_t *)((char *)h->ws.p + b_probs);
  int32_t *d_pc = (int32_t *)((char *)h->ws.p + b_probs + b_paths);
  return s->dtype == DM_F32 ? dr_recommend_dev_t<float>(h, d_seq, U, beam, topk, d_paths, d_probs, d_pc, d_ids, d_scores, d_counts)
                            : dr_recommend_dev_t<double>(h, d_seq, U, beam, topk, d_paths, d_probs, d_pc, d_ids, d_scores, d_counts);
}

int dm_dr_recommend_dev(dm_handle_t h, const int32_t *d_seq_ids, int64_t U, int beam, int topk, int32_t *d_out_ids,
                        double *d_out_scores, int32_t *d_out_counts) {
  if (!h) return DM_ERR_INVALID;
  int rc = dr_check_search(h, "dm_dr_recommend", U, beam, true);
  if (rc != DM_OK) return rc;
  if (topk < 1 || topk > 2048) return fail(h, DM_ERR_INVALID, "dm_dr_recommend: topk must be in [1, 2048]");
  if (U == 0) return DM_OK;
  if (!d_seq_ids || !d_out_ids || !d_out_scores || !d_out_counts) return fail(h, DM_ERR_INVALID, "dm_dr_recommend: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  return dr_recommend_dev(h, d_seq_ids, U, beam, topk, d_out_ids, d_out_scores, d_out_counts);
}

int dm_dr_recommend(dm_handle_t h, const int32_t *seq_ids, int64_t U, int beam, int topk, int32_t *out_ids,
                    double *out_scores, int32_t *out_counts) {
  if (!h) return DM_ERR_INVALID;
  int rc = dr_check_search(h, "dm_dr_recommend", U, beam, true);
  if (rc != DM_OK) return rc;
  if (topk < 1 || topk > 2048) return fail(h, DM_ERR_INVALID, "dm_dr_recommend: topk must be in [1, 2048]");
  if (U == 0) return DM_OK;
  if (!seq_ids || !out_ids || !out_scores || !out_counts) return fail(h, DM_ERR_INVALID, "dm_dr_recommend: null argument");
  dm_dr_state *s = h->dr;
  if ((rc = dr_check_ids(h, seq_ids, U * s->L)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ReqLayout lay(h, s->io, 0, U, (size_t)s->L * 4, (size_t)topk, 8);
  if ((rc = lay.commit(out_ids, out_scores, out_counts)) != DM_OK) return rc;
  int32_t *d_seq = lay.d<int32_t>(lay.SEQ), *d_ids = lay.d<int32_t>(lay.IDS), *d_cnt = lay.d<int32_t>(lay.COUNTS);
  double *d_sc = lay.d<double>(lay.SCORES);
  if (U <= 8 && h->direct_ok && lay.fits_stage()) {
    // single requests (DeepRetrieval.recommend's serving loop, examples/.../dr/package.scala:107-111): request and results live in the
    // host-mapped pinned staging block — the kernels read and write it in place, no copy on either side of the three launches.
    // The stream is synchronized; no counts are polled.
    if ((rc = lay.stage(seq_ids)) != DM_OK) return rc;
    if ((rc = dr_recommend_dev(h, lay.stage_ptr(d_seq), U, beam, topk, lay.stage_ptr(d_ids), lay.stage_ptr(d_sc), lay.stage_ptr(d_cnt))) != DM_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    lay.copy_from_stage();
    return DM_OK;
  }
  HIPCHK(h, lay.upload(seq_ids));
  if ((rc = dr_recommend_dev(h, d_seq, U, beam, topk, d_ids, d_sc, d_cnt)) != DM_OK) return rc;
  HIPCHK(h, lay.finish());
  return DM_OK;
}
