// Host side of the training step (row A12) and of the multi-GPU gradient exchange (SURVEY.md §5, §8e).

static int train_check(dm_ctx *h, const char *who) {
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": weights not loaded");
  DM_DIN_ONLY(h, who);
  if (!h->train_ready) return fail(h, DM_ERR_STATE, std::string(who) + ": call dm_train_init first");
  return DM_OK;
}

static int64_t compact_len(const dm_ctx *h) { return compact_len_for(h->num_index, h->embed); }
static size_t elem_size(const dm_ctx *h) { return h->dtype == DM_F64 ? 8 : 4; }

int dm_train_init(dm_handle_t h, const dm_adam_opts *o) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_train_init");
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, "dm_train_init: weights not loaded");
  DM_DIN_ONLY(h, "dm_train_init");
  if (!o || o->lr <= 0) return fail(h, DM_ERR_INVALID, "dm_train_init: bad optimizer options");
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t n = compact_len(h);
  const size_t es = elem_size(h);
  const size_t fb = (size_t)h->embed * h->embed * 4;
  free_training(h);       // (a failure below leaves a handle that is not training, not one that trains on null buffers)
  int rc = h->train.init(h, h->num_index, h->embed, n, es, *o);
  if (rc != DM_OK) return rc;
  if (h->dtype == DM_F64) ALLOC(h, h->d_tr64, 6 * (size_t)h->embed * h->embed * 8);
  else { ALLOC(h, h->d_attTA, fb); ALLOC(h, h->d_w1aTA, fb); ALLOC(h, h->d_w1bTA, fb); }
  ALLOC(h, h->d_loss, 16);
  ALLOC(h, h->d_touch_bits, (size_t)((h->num_index + 31) / 32 + 1) * 4);
  ALLOC(h, h->d_touch_cnt, 8);
  HIPCHK(h, hipMemsetAsync(h->d_touch_bits, 0, (size_t)((h->num_index + 31) / 32 + 1) * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_touch_cnt, 0, 8, h->stream));
  h->touch_cap = 0; h->touch_ub = 0; h->train_ready = true; h->last_loss = 0.0;
  model_changed(h);      // (clones re-mirror: the lazily rebuilt copies are stale)
  h->lazy.training_started();
  return derive_small(h, DERIVE_OWN);      // d_tr64 / the transposed fragments were just allocated
}

__global__ void dm_mark_touched_kernel(const int32_t *codes, const int32_t *seqs, int64_t B, int L, unsigned *bits,
                                       int32_t *list, unsigned long long *cnt, unsigned long long cap, int64_t num_index) {
  const int64_t n = B * (1 + L);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t idx = t < B ? codes[t] : seqs[t - B];
    if (idx < 0 || idx >= num_index) continue;
    const unsigned bit = 1u << (idx & 31);
    if (bits[idx >> 5] & bit) continue;       // already listed (a batch repeats its history rows hundreds of times): no atomic
    const unsigned old = atomicOr(bits + (idx >> 5), bit);
    if (!(old & bit)) {
      const unsigned long long pos = atomicAdd(cnt, 1ull);
      if (pos < cap) list[pos] = idx;      // the host sizes the list so that this always holds (touch_ub)
    }
  }
}

template <typename T, int E>
static int launch_train_E(dm_ctx *h, TrainParamsT<T> &p, const WGradParamsT<T> &wg) {
  const bool f64 = sizeof(T) == 8;
  // fp64: one staged E x E matrix + the (p_j, dp_j) pairs of the attention backward (4 waves x ML positions x 16 rows); fp32: att.W and W1b fragments
  const int ml = p.L <= DM_MAXL ? DM_MAXL : DM_PIPE_MAXL;
  const int block = f64 ? 256 : DM_BLOCK, nw = block / 64;
  const int lds = (f64 ? E * E * 8 + 4 * ml * 16 * 2 * 8 : 2 * E * E * 4) + (f64 ? 0 : nw * ml * 16 * 4);      // + the per-wave history-code staging (f32 instances)
  int64_t tiles = (p.B + 15) / 16, blocks = (tiles + nw - 1) / nw;
  const int64_t max_blocks = h->n_cu;
  if (blocks > max_blocks) blocks = max_blocks;
  const int rc = p.L <= DM_MAXL ? LAUNCH_LDS(h, (dm_train_rows_kernel<T, E, DM_MAXL>), dim3((unsigned)blocks), dim3(block), lds, p)
                                : LAUNCH_LDS(h, (dm_train_rows_kernel<T, E, DM_PIPE_MAXL>), dim3((unsigned)blocks), dim3(block), lds, p);      // histories of 17 .. 32 positions
  if (rc != DM_OK) return rc;
  // weight gradients: 3 matrices x (NT / RT)^2 output blocks x row chunks, ~8 one-wave workgroups per SIMD, at least 128 rows each
  constexpr int NT = E / 16, RT = NT < 4 ? NT : 4, NBLK = 3 * (NT / RT) * (NT / RT);
  WGradParamsT<T> wq = wg;
  const int64_t want = std::max<int64_t>(1, (int64_t)h->n_cu * 32 / NBLK);
  wq.chunk = std::max<int64_t>(128, (((wq.B + want - 1) / want) + 7) / 8 * 8);
  const int chunks = (int)((wq.B + wq.chunk - 1) / wq.chunk);
  return LAUNCH(h, (dm_wgrad_kernel<T, E>), dim3(NBLK, chunks), dim3(64), 0, wq);
}

template <typename T>
static int train_fb_launch(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const unsigned *d_rowmask,
                           const float *d_labels, int64_t B, int L) {
  typedef typename DmTr<T>::V4 V4;
  const int E = h->embed;
  const size_t n2 = (size_t)E * E;
  TrainParamsT<T> p;
  const T *base = (const T *)h->d_compact;
  p.emb = base; p.num_index = h->num_index;
  if (sizeof(T) == 8) {
    const double *f = (const double *)h->d_tr64;
    p.attA = (const V4 *)f; p.w1aA = (const V4 *)(f + n2); p.w1bA = (const V4 *)(f + 2 * n2);
    p.attTA = (const V4 *)(f + 3 * n2); p.w1aTA = (const V4 *)(f + 4 * n2); p.w1bTA = (const V4 *)(f + 5 * n2);
    const T *tail = base + h->num_index * E + 3 * (int64_t)n2;
    p.b1 = tail; p.w2 = tail + E;
    T b2;
    HIPCHK(h, hipMemcpyAsync(&b2, tail + 2 * E, sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    p.b2 = b2;
  } else {
    p.attA = (const V4 *)h->d_attA; p.w1aA = (const V4 *)h->d_w1aA; p.w1bA = (const V4 *)h->d_w1bA;
    p.attTA = (const V4 *)h->d_attTA; p.w1aTA = (const V4 *)h->d_w1aTA; p.w1bTA = (const V4 *)h->d_w1bTA;
    p.b1 = (const T *)h->d_b1; p.w2 = (const T *)h->d_w2; p.b2 = (T)h->b2;
  }
  p.codes = d_codes; p.seqs = d_seqs; p.rowmask = d_rowmask; p.labels = d_labels; p.B = B; p.L = L; p.inv_B = (T)(1.0 / (double)B);
  p.sm_scale = (T)sm_scale64(h);
  p.grad = (T *)h->train.grad;
  T *ws = (T *)h->ws.p;
  p.DZ = ws; p.AT = ws + (size_t)B * E; p.DA = ws + 2 * (size_t)B * E; p.CB = ws + 3 * (size_t)B * E;
  p.logits = ws + 4 * (size_t)B * E;
  p.loss_acc = (T *)h->d_loss;
  WGradParamsT<T> wg;
  wg.emb = base; wg.codes = d_codes; wg.DZ = p.DZ; wg.AT = p.AT; wg.DA = p.DA; wg.CB = p.CB; wg.B = B;
  wg.num_index = h->num_index; wg.grad = (T *)h->train.grad;
  wg.chunk = 256;
  return dispatch_E(h, E, "unsupported embed size", [&](auto e) { return launch_train_E<T, decltype(e)::value>(h, p, wg); });
}

// The general-rows forward of an f64 model on the matrix pipe: the forward half of dm_train_rows_kernel<double> (same fragments, same
// arithmetic as the training forward), available while the handle holds training state (d_tr64: refreshed with every weight change,
// together with the transposes dm_din_forward_kernel<double> reads).  Logits to d_out; nothing else is written.
template <int E>
static int rows_fwd64_E(dm_ctx *h, TrainParamsT<double> &p) {
  const int ml = p.L <= DM_MAXL ? DM_MAXL : DM_PIPE_MAXL;
  const int lds = E * E * 8 + 4 * ml * 16 * 2 * 8 + (ml > 16 ? 0 : 4 * ml * 16 * 4);
  int64_t tiles = (p.B + 15) / 16, blocks = (tiles + 3) / 4;
  if (blocks > h->n_cu) blocks = h->n_cu;
  return p.L <= DM_MAXL ? LAUNCH_LDS(h, (dm_train_rows_kernel<double, E, DM_MAXL, true>), dim3((unsigned)blocks), dim3(256), lds, p)
                        : LAUNCH_LDS(h, (dm_train_rows_kernel<double, E, DM_PIPE_MAXL, true>), dim3((unsigned)blocks), dim3(256), lds, p);
}
static bool rows_fwd64_available(const dm_ctx *h, int L) { return h->dtype == DM_F64 && h->d_tr64 && L >= 1 && L <= DM_PIPE_MAXL; }
// ... and on a handle WITHOUT training state: the fragments are built on first use (freed with the weights they were made from:
// dm_load_weights_din*, dm_train_init / dm_train_free; a clone has none of its own and keeps the scalar kernel)
static bool fwd64_ready(dm_ctx *h, int L) {
  if (h->dtype != DM_F64 || L < 1 || L > DM_PIPE_MAXL || !h->w_loaded) return false;
  if (h->d_tr64) return true;
  if (h->parent) return false;
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  if (h->d_tr64) return true;
  if (dm_alloc(h, &h->d_tr64, 6 * (size_t)h->embed * h->embed * 8) != DM_OK) { h->d_tr64 = nullptr; return false; }
  if (derive_small(h, DERIVE_OWN) != DM_OK) { dm_release(h->d_tr64); return false; }
  return true;
}
static int rows_fwd64(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const unsigned *d_rowmask, int64_t B, int L, double *d_out) {
  typedef DmTr<double>::V4 V4;
  if (B <= 0) return DM_OK;
  const int E = h->embed;
  const size_t n2 = (size_t)E * E;
  TrainParamsT<double> p{};
  const double *base = (const double *)h->d_compact;
  p.emb = base; p.num_index = h->num_index;
  const double *f = (const double *)h->d_tr64;
  p.attA = (const V4 *)f; p.w1aA = (const V4 *)(f + n2); p.w1bA = (const V4 *)(f + 2 * n2);
  const double *tail = base + h->num_index * E + 3 * (int64_t)n2;
  p.b1 = tail; p.w2 = tail + E;
  double b2;
  HIPCHK(h, hipMemcpyAsync(&b2, tail + 2 * E, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  p.b2 = b2;
  p.codes = d_codes; p.seqs = d_seqs; p.rowmask = d_rowmask; p.B = B; p.L = L; p.sm_scale = sm_scale64(h); p.logits = d_out;
  return dispatch_E(h, E, "unsupported embed size", [&](auto e) { return rows_fwd64_E<decltype(e)::value>(h, p); });
}

// The touched-row list keeps growing until the next Adam step (gradients accumulate across calls): keep a host-side upper bound of its
// length and grow the list, PRESERVING its entries, before a call that may add `more` rows could overflow it.
static int train_touch_reserve(dm_ctx *h, size_t more) {
  h->touch_ub += more;
  if (h->touch_ub > (size_t)h->num_index) h->touch_ub = (size_t)h->num_index;
  if (h->touch_ub > h->touch_cap) {
    size_t cap = h->touch_cap * 2 > h->touch_ub ? h->touch_cap * 2 : h->touch_ub;
    if (cap > (size_t)h->num_index) cap = (size_t)h->num_index;
    int32_t *nl = nullptr;
    ALLOC(h, nl, cap * 4);
    if (h->d_touch_list && h->touch_cap)
      HIPCHK(h, hipMemcpyAsync(nl, h->d_touch_list, h->touch_cap * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    dm_release(h->d_touch_list);
    h->d_touch_list = nl;
    h->touch_cap = cap;
  }
  return DM_OK;
}

// all pointers device; accumulates this batch's gradients (mean BCE over the B rows) into the handle's gradient
static int train_fb_dev(dm_ctx *h, const int32_t *d_codes, const int32_t *d_seqs, const unsigned *d_rowmask,
                        const float *d_labels, int64_t B, int L, float *loss) {
  const int E = h->embed;
  const size_t es = elem_size(h);
  const size_t vec = (size_t)B * E * es;
  int rc = ensure_ws(h, 4 * vec + (size_t)B * es);
  if (rc != DM_OK) return rc;
  if ((rc = train_touch_reserve(h, (size_t)B * (1 + L))) != DM_OK) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_loss, 0, 16, h->stream));
  rc = h->dtype == DM_F64 ? train_fb_launch<double>(h, d_codes, d_seqs, d_rowmask, d_labels, B, L)
                          : train_fb_launch<float>(h, d_codes, d_seqs, d_rowmask, d_labels, B, L);
  if (rc != DM_OK) return rc;
  if ((rc = LAUNCH(h, dm_mark_touched_kernel, dim3(256), dim3(256), 0, d_codes, d_seqs, B, L, h->d_touch_bits, h->d_touch_list, h->d_touch_cnt, h->touch_cap,
                   h->num_index)) != DM_OK) return rc;
  if ((rc = h->train.mark_active(h, 256, d_codes, B, d_seqs, B * L)) != DM_OK) return rc;
  if (loss) {
    if (h->dtype == DM_F64) {
      double acc[2];
      HIPCHK(h, hipMemcpyAsync(acc, h->d_loss, 16, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->last_loss = (acc[0] - acc[1]) / (double)B;
    } else {
      float acc[2];
      HIPCHK(h, hipMemcpyAsync(acc, h->d_loss, 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->last_loss = (double)((acc[0] - acc[1]) / (float)B);       // BCECriterionWithLogits.scala:52-58, sizeAverage
    }
    *loss = (float)h->last_loss;
  }
  return DM_OK;
}

// the loss of the last dm_train_forward_backward* call that asked for one, in the model's precision
int dm_train_last_loss(dm_handle_t h, double *loss) {
  if (!h || !loss) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_last_loss");
  if (rc != DM_OK) return rc;
  *loss = h->last_loss;
  return DM_OK;
}

int dm_train_forward_backward(dm_handle_t h, const int32_t *codes, const int32_t *seqs, const int32_t *pad_flat_idx,
                              int64_t n_pad, const float *labels, int64_t B, int L, float *loss) {
  if (!h) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_forward_backward");
  if (rc != DM_OK) return rc;
  if (!codes || !seqs || !labels || B <= 0 || L <= 0 || L > DM_PIPE_MAXL || n_pad < 0 || (n_pad > 0 && !pad_flat_idx))
    return fail(h, DM_ERR_INVALID, "dm_train_forward_backward: bad arguments (L must be 1..32)");
  if ((rc = check_table_ids(h, "dm_train_forward_backward", "item index", codes, B, -1)) != DM_OK ||
      (rc = check_table_ids(h, "dm_train_forward_backward", "history index", seqs, B * L, -1)) != DM_OK) return rc;
  for (int64_t i = 0; i < n_pad; i++)
    if (pad_flat_idx[i] < 0 || pad_flat_idx[i] >= B * L) return fail(h, DM_ERR_INDEX, "dm_train_forward_backward: mask index outside [0, B*L)");
  HIPCHK(h, hipSetDevice(h->device));
  int32_t *d_codes = nullptr, *d_seqs = nullptr, *d_pad = nullptr;
  unsigned *d_mask = nullptr;
  float *d_lab = nullptr;
  DevTemps t(h);
  if ((rc = t.alloc(d_codes, B * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_seqs, B * L * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_mask, B * 4)) != DM_OK) return rc;
  if ((rc = t.alloc(d_lab, B * 4)) != DM_OK) return rc;
  hipError_t e = hipMemcpyAsync(d_codes, codes, B * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_seqs, seqs, B * L * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_lab, labels, B * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_mask, 0, B * 4, h->stream);
  if (e != hipSuccess) return fail(h, DM_ERR_HIP, "dm_train_forward_backward: upload failed");
  if (n_pad > 0) {
    if ((rc = t.alloc(d_pad, n_pad * 4)) != DM_OK) return rc;
    if (hipMemcpyAsync(d_pad, pad_flat_idx, n_pad * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(h, DM_ERR_HIP, "upload failed");
    if ((rc = LAUNCH(h, dm_pad_rowmask_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, d_pad, n_pad, L, d_mask)) != DM_OK) return rc;
  }
  float l = 0.f;
  rc = train_fb_dev(h, d_codes, d_seqs, d_mask, d_lab, B, L, &l);
  if (rc == DM_OK && loss) *loss = l;
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == DM_OK) return fail(h, DM_ERR_HIP, "dm_train_forward_backward: kernel failed");
  return rc;
}

__global__ void dm_clear_touched_kernel(const int32_t *list, int64_t n, unsigned *bits) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    atomicAnd(bits + (list[t] >> 5), ~(1u << (list[t] & 31)));
}

int dm_adam_step(dm_handle_t h, float grad_scale) {
  if (!h) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_adam_step");
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  unsigned long long cnt = 0, act = 0;
  HIPCHK(h, hipMemcpyAsync(&cnt, h->d_touch_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&act, h->train.active_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const AdamPlan plan = h->train.plan_step(act);
  h->adam_last_sparse = plan.rows_path ? 1 : 0; h->adam_last_rows = plan.rows_path ? act : (unsigned long long)h->num_index;
  h->lazy.adam_stepped(plan.rows_path, act, h->dtype == DM_F64);      // before the first launch: a step that fails half-way has still moved weights
  if ((rc = adam_step(h, h->train, plan, h->d_compact, h->dtype == DM_F64, false, grad_scale, false, 64)) != DM_OK) return rc;
  // forget which rows were touched in this step
  if (cnt > 0 && h->d_touch_list) {
    if ((rc = LAUNCH(h, dm_clear_touched_kernel, dim3(256), dim3(256), 0, h->d_touch_list, cnt, h->d_touch_bits)) != DM_OK) return rc;
  }
  HIPCHK(h, hipMemsetAsync(h->d_touch_cnt, 0, 8, h->stream));
  h->touch_ub = 0;
  // the weights moved: the derived copies in the model's own type follow at once, the lazy ones were marked stale above
  model_changed(h);      // (clones re-mirror)
  return derive_small(h, DERIVE_OWN);
}

// measurement: embedding rows the last dm_adam_step visited (== num_index when it streamed the whole table) and whether it took the
// active-rows path
int dm_adam_last_step_rows(dm_handle_t h, uint64_t *rows, int *active_rows_only) {
  if (!h || !rows || !active_rows_only) return DM_ERR_INVALID;
  *rows = h->adam_last_rows; *active_rows_only = h->adam_last_sparse;
  return DM_OK;
}

int dm_train_download(dm_handle_t h, int what, void *out, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, "dm_train_download: weights not loaded");
  DM_DIN_ONLY(h, "dm_train_download");
  const bool padded = h->embed_log != h->embed;
  if (!out || n != compact_len_for(h->num_index, h->embed_log)) return fail(h, DM_ERR_INVALID, "dm_train_download: n must be the compact vector length");
  const void *src = what == 0 ? h->d_compact : h->train.buffer(what);
  if (!src) return fail(h, DM_ERR_STATE, "dm_train_download: call dm_train_init first");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!padded) { HIPCHK(h, hipMemcpy(out, src, (size_t)n * elem_size(h), hipMemcpyDeviceToHost)); return DM_OK; }
  // a model loaded with an embed size the kernels pad (dm_load_weights_din): the caller sees the model's own layout
  std::vector<char> tmp((size_t)compact_len(h) * elem_size(h));
  HIPCHK(h, hipMemcpy(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost));
  if (h->dtype == DM_F64) unpad_compact<double>((const double *)tmp.data(), h->embed_log, h->embed, h->num_index, (double *)out);
  else unpad_compact<float>((const float *)tmp.data(), h->embed_log, h->embed, h->num_index, (float *)out);
  return DM_OK;
}

// ---- multi-GPU exchange (SURVEY.md §5): dense block by all-reduce, embedding rows as (index, row) lists ----
int dm_train_dense_block(dm_handle_t h, void **d_ptr, int64_t *n) {
  if (!h || !d_ptr || !n) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_dense_block");
  if (rc != DM_OK) return rc;
  if (h->embed_log != h->embed) return fail(h, DM_ERR_UNSUPPORTED, "dm_train_dense_block: the model's embed size is zero-padded on the device; use dm_train_sync_gradients");
  const int64_t E = h->embed;
  *d_ptr = (char *)h->train.grad + (size_t)(h->num_index * E) * elem_size(h);
  *n = 3 * E * E + 2 * E + 1;
  return DM_OK;
}

template <typename T>
__global__ void dm_gather_rows_kernel(const T *grad, const int32_t *list, int64_t n, int E, int32_t *rows_out, T *grads_out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * E; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / E;
    const int e = (int)(t % E);
    grads_out[t] = grad[(int64_t)list[i] * E + e];
    if (e == 0) rows_out[i] = list[i];
  }
}
template <typename T>
__global__ void dm_add_rows_kernel(T *grad, const int32_t *rows, const T *g, int64_t n, int E, int64_t num_index) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * E; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t rw = rows[t / E];
    if (rw >= 0 && rw < num_index) atomicAdd(grad + (int64_t)rw * E + (t % E), g[t]);
  }
}
static int launch_gather_rows(dm_ctx *h, int64_t cnt, int32_t *d_rows, void *d_grads) {
  return h->dtype == DM_F64
             ? LAUNCH(h, dm_gather_rows_kernel<double>, dim3(1024), dim3(256), 0, (const double *)h->train.grad, h->d_touch_list, cnt, h->embed, d_rows, (double *)d_grads)
             : LAUNCH(h, dm_gather_rows_kernel<float>, dim3(1024), dim3(256), 0, (const float *)h->train.grad, h->d_touch_list, cnt, h->embed, d_rows, (float *)d_grads);
}
static int launch_add_rows(dm_ctx *h, const int32_t *d_rows, const void *d_grads, int64_t n) {
  const int rc = h->train.mark_active(h, 256, d_rows, n);
  if (rc != DM_OK) return rc;
  return h->dtype == DM_F64 ? LAUNCH(h, dm_add_rows_kernel<double>, dim3(1024), dim3(256), 0, (double *)h->train.grad, d_rows, (const double *)d_grads, n, h->embed, h->num_index)
                            : LAUNCH(h, dm_add_rows_kernel<float>, dim3(1024), dim3(256), 0, (float *)h->train.grad, d_rows, (const float *)d_grads, n, h->embed, h->num_index);
}

int dm_train_export_rows(dm_handle_t h, int32_t *d_rows, void *d_grads, int64_t cap, int64_t *n) {
  if (!h || !n) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_export_rows");
  if (rc != DM_OK) return rc;
  if (h->embed_log != h->embed) return fail(h, DM_ERR_UNSUPPORTED, "dm_train_export_rows: the model's embed size is zero-padded on the device; use dm_train_sync_gradients");
  HIPCHK(h, hipSetDevice(h->device));
  unsigned long long cnt = 0;
  HIPCHK(h, hipMemcpyAsync(&cnt, h->d_touch_cnt, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *n = (int64_t)cnt;
  if (!d_rows || !d_grads) return DM_OK;                 // size query
  if ((int64_t)cnt > cap) return fail(h, DM_ERR_INVALID, "dm_train_export_rows: buffer too small");
  if (cnt > 0) {
    if ((rc = launch_gather_rows(h, (int64_t)cnt, d_rows, d_grads)) != DM_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return DM_OK;
}

int dm_train_add_rows(dm_handle_t h, const int32_t *d_rows, const void *d_grads, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_add_rows");
  if (rc != DM_OK) return rc;
  if (h->embed_log != h->embed) return fail(h, DM_ERR_UNSUPPORTED, "dm_train_add_rows: the model's embed size is zero-padded on the device; use dm_train_sync_gradients");
  if (n < 0 || (n > 0 && (!d_rows || !d_grads))) return fail(h, DM_ERR_INVALID, "dm_train_add_rows: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  if (n > 0) {
    if ((rc = launch_add_rows(h, d_rows, d_grads, n)) != DM_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return DM_OK;
}

int dm_memcpy_d2d(dm_handle_t h, void *dst, const void *src, size_t bytes) {
  if (!h) return DM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

// training on rows that already live in device memory (row mask instead of a flat mask list)
int dm_train_forward_backward_dev(dm_handle_t h, const int32_t *d_codes, const int32_t *d_seqs, const uint32_t *d_rowmask,
                                  const float *d_labels, int64_t B, int L, float *loss) {
  if (!h) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_forward_backward_dev");
  if (rc != DM_OK) return rc;
  if (!d_codes || !d_seqs || !d_labels || B <= 0 || L <= 0 || L > DM_PIPE_MAXL) return fail(h, DM_ERR_INVALID, "dm_train_forward_backward_dev: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  return train_fb_dev(h, d_codes, d_seqs, d_rowmask, d_labels, B, L, loss);
}
