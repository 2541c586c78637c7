// Deep-Retrieval: the item -> paths mapping and the training set resident on the device (DESIGN.md §25).
//   * the mapping: MappingOp.itemPathMapping as a table [num_item x J x D]; its inverse, the path -> items CSR the rerank search reads
//     (MappingOp.pathItemMapping, what dm_dr_load_path_items takes from the host), is built from it here: path codes, ONE stable sort of
//     (code, item), duplicate and head flags, two compactions, the offsets with the largest bucket.  Integers only;
//   * the training set: histories [N x L] and targets [N] uploaded once, and an order [N] of sample indices.  A step gathers one range of
//     the order into the handle's workspace (histories, and the [J x D] paths of every target out of the table) and runs the device
//     entry points of the layer step / the rerank step on it, unchanged;
//   * the M-step over the resident set: dm_dr_mstep_optimize without the upload, in STORAGE order (the streaming fold depends on the
//     order of the samples); the new codes are decoded into the table and the CSR is rebuilt from it.
// The shuffle: LocalDataSet.scala shuffles with an unseeded scala.util.Random, so there is no stream to reproduce; the order here is the
// library's own, a function of (seed, epoch) alone, as the rerank sampler's negatives are: the sample indices sorted (stable) by
// key(i) = splitmix(splitmix(seed ^ splitmix(epoch)) + i).

// entry i = (item i / J, slot i % J): key = the path code sum_d node_d K^(D-1-d), value = the item
__global__ __launch_bounds__(256) void dts_codes_kernel(const int32_t *tab, int64_t m, int J, int D, int K, unsigned long long *keys, int32_t *vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long code = 0;
    for (int d = 0; d < D; d++) code = code * (unsigned long long)K + (unsigned long long)tab[i * D + d];
    keys[i] = code;
    vals[i] = (int32_t)(i / J);
  }
}
// sorted by code, items ascending inside a code (the sort is stable and the entries come in item order): an item that lists a path twice
// has its entries next to each other, and the later ones are dropped (a Map has one entry per key)
__global__ __launch_bounds__(256) void dts_keep_kernel(const unsigned long long *ks, const int32_t *vs, int64_t m, uint8_t *keep) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x)
    keep[j] = (j > 0 && ks[j - 1] == ks[j] && vs[j - 1] == vs[j]) ? 0 : 1;
}
// path p holds the kept entries [head[p], head[p + 1]) (the last one ends at n_kept): the offsets, and the largest bucket
__global__ __launch_bounds__(256) void dts_offsets_kernel(const int32_t *head, int64_t P, int64_t n_kept, int64_t *item_off, int *max_len) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < P; base += stride) {      // whole waves stay together: the maximum is wave-wide
    const int64_t p = base + threadIdx.x;
    int len = 0;
    if (p < P) {
      const int64_t a = head[p], e = p + 1 < P ? (int64_t)head[p + 1] : n_kept;
      item_off[p] = a;
      if (p == P - 1) item_off[P] = n_kept;
      len = (int)(e - a);
    }
    for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o));
    if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(max_len, len);
  }
}
// the M-step's codes [num_item x J] back into nodes [num_item x J x D]
__global__ __launch_bounds__(256) void dts_decode_kernel(const long long *codes, int64_t m, int D, int K, int32_t *tab) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long c = (unsigned long long)codes[i];
    for (int d = D - 1; d >= 0; d--) {
      const unsigned long long q = c / (unsigned long long)K;
      tab[i * D + d] = (int32_t)(c - q * (unsigned long long)K);
      c = q;
    }
  }
}
__global__ __launch_bounds__(256) void dts_iota_kernel(int32_t *out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (int32_t)i;
}
__global__ __launch_bounds__(256) void dts_shuffle_keys_kernel(unsigned long long seed, unsigned long long epoch, int64_t n, unsigned long long *keys, int32_t *vals) {
  const unsigned long long base = dm_dev_splitmix(seed ^ dm_dev_splitmix(epoch));
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    keys[i] = dm_dev_splitmix(base + (unsigned long long)i);
    vals[i] = (int32_t)i;
  }
}

// Samples order[offset .. offset + S) of the resident set, one element per thread over three consecutive index ranges:
//   o_seq   [S rep x L]   the history of sample r / rep (rep = 1, or J: transformLayerData's repeated rows)
//   o_paths [S x J x D]   the paths of the sample's target out of the table (tab == nullptr: none); the same bytes as [S J x D]
//   o_tgt   [S]           the targets (o_tgt == nullptr: none)
struct DtsGatherParams {
  const int32_t *seq, *tgt, *order, *tab;
  int64_t offset, S;
  int L, J, D, rep;
  int32_t *o_seq, *o_paths, *o_tgt;
};
__global__ __launch_bounds__(256) void dts_gather_kernel(DtsGatherParams p) {
  const int64_t n_seq = p.S * p.rep * p.L, JD = (int64_t)p.J * p.D, n_pa = p.tab ? p.S * JD : 0, n_t = p.o_tgt ? p.S : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_seq + n_pa + n_t; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_seq) {
      const int64_t r = i / p.L;
      const int64_t smp = p.order[p.offset + r / p.rep];
      p.o_seq[i] = p.seq[smp * p.L + (i - r * p.L)];
    } else if (i < n_seq + n_pa) {
      const int64_t q = i - n_seq, r = q / JD;
      const int64_t smp = p.order[p.offset + r];
      p.o_paths[q] = p.tab[(int64_t)p.tgt[smp] * JD + (q - r * JD)];
    } else {
      const int64_t q = i - n_seq - n_pa;
      p.o_tgt[q] = p.tgt[p.order[p.offset + q]];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int dts_check_model(dm_ctx *h, const char *who) {
  dm_dr_state *s = h->dr;
  if (!s || !s->loaded) return fail(h, DM_ERR_STATE, std::string(who) + ": Deep-Retrieval model not loaded");
  return DM_OK;
}
static int dts_check_set(dm_ctx *h, const char *who, bool need_set, bool need_map) {
  const int rc = dts_check_model(h, who);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if (need_set && !s->d_ts_seq) return fail(h, DM_ERR_STATE, std::string(who) + ": no resident training set (dm_dr_train_set_load)");
  if (need_map && !s->d_item_paths) return fail(h, DM_ERR_STATE, std::string(who) + ": no resident item -> paths table (dm_dr_set_item_paths)");
  return DM_OK;
}

// The path -> items CSR of the table tab [num_item x J x D] (device, nodes in [0, K)), exactly what dm_dr_load_path_items leaves behind
// for the host inversion of the same table.  The handle's CSR is replaced only when everything has succeeded.
static int dts_build_csr(dm_ctx *h, dm_dr_state *s, const int32_t *tab, int J) {
  const int K = s->K, D = s->D;
  const int64_t m = s->num_item * J;
  const bool detail = dr_time_launches();
  int64_t space = 1;
  for (int d = 0; d < D; d++) space *= K;
  int rc;
  DevArena ar(s->ts_ws, 8);
  size_t o_k[2], o_v[2];
  for (int i = 0; i < 2; i++) { o_k[i] = ar.add((size_t)m * 8); o_v[i] = ar.add((size_t)m * 4); }
  const size_t o_flag = ar.add((size_t)m), o_tmp = ar.add(dev_sort_scratch_bytes(m)), o_st = ar.add(64);
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  unsigned long long *kb[2] = {ar.ptr<unsigned long long>(o_k[0]), ar.ptr<unsigned long long>(o_k[1])};
  int32_t *vb[2] = {ar.ptr<int32_t>(o_v[0]), ar.ptr<int32_t>(o_v[1])};
  uint8_t *flag = ar.ptr<uint8_t>(o_flag);
  uint32_t *tmp = ar.ptr<uint32_t>(o_tmp);
  unsigned long long *st = ar.ptr<unsigned long long>(o_st);      // [0] kept entries, [1] paths, [2] (as int) the largest bucket
  HIPCHK(h, hipMemsetAsync(st, 0, 64, h->stream));
  // ---- (code, item) sorted by code; the duplicates dropped into the other pair of buffers
  int where = 0;
  rc = timed(h, EV_DTS_CSR, detail, [&]() -> int {
    int r;
    if ((r = LAUNCH(h, dts_codes_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, tab, m, J, D, K, kb[0], vb[0])) != DM_OK) return r;
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[0], vb[0], kb[1], vb[1], m, 0, std::max(1, drm_ceil_log2(space)), tmp, &where));
    if ((r = LAUNCH(h, dts_keep_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, kb[where], vb[where], m, flag)) != DM_OK) return r;
    HIPCHK(h, (dev_select_flagged<int32_t, unsigned long long>(h->stream, vb[where], kb[where], flag, vb[where ^ 1], kb[where ^ 1], st, m, tmp)));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  unsigned long long cnt[3] = {};
  HIPCHK(h, hipMemcpyAsync(cnt, st, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int64_t n_kept = (int64_t)cnt[0];
  const int32_t *items = vb[where ^ 1];
  const unsigned long long *kcodes = kb[where ^ 1];
  int32_t *head = vb[where];                                      // (the sorted pairs are no longer read)
  unsigned long long *pcodes = kb[where];
  // ---- the distinct codes and where each starts among the kept entries
  rc = timed(h, EV_DTS_CSR, detail, [&]() -> int {
    const int r = LAUNCH(h, drm_heads_kernel, dim3(drt_blocks(h, n_kept, 256)), dim3(256), 0, kcodes, n_kept, ~0ull, flag);
    if (r != DM_OK) return r;
    HIPCHK(h, (dev_select_flagged<int32_t, unsigned long long>(h->stream, (const int32_t *)nullptr, kcodes, flag, head, pcodes, st + 1, n_kept, tmp)));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(cnt + 1, st + 1, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int64_t P = (int64_t)cnt[1];
  void *n_codes = nullptr, *n_off = nullptr, *n_items = nullptr;
  if ((rc = dm_alloc(h, &n_codes, (size_t)P * 8)) != DM_OK || (rc = dm_alloc(h, &n_off, ((size_t)P + 1) * 8)) != DM_OK ||
      (rc = dm_alloc(h, &n_items, (size_t)n_kept * 4)) != DM_OK) {
    dm_release(n_codes, n_off, n_items);
    return rc;
  }
  rc = timed(h, EV_DTS_CSR, detail, [&]() -> int {
    const int r = LAUNCH(h, dts_offsets_kernel, dim3(drt_blocks(h, P, 256)), dim3(256), 0, head, P, n_kept, (int64_t *)n_off, (int *)(st + 2));
    if (r != DM_OK) return r;
    HIPCHK(h, hipMemcpyAsync(n_codes, pcodes, (size_t)P * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(n_items, items, (size_t)n_kept * 4, hipMemcpyDeviceToDevice, h->stream));
    return DM_OK;
  });
  hipError_t e = hipSuccess;
  if (rc == DM_OK && (e = hipMemcpyAsync(cnt + 2, st + 2, 8, hipMemcpyDeviceToHost, h->stream)) == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (rc != DM_OK || e != hipSuccess) {
    dm_release(n_codes, n_off, n_items);
    return rc != DM_OK ? rc : fail(h, DM_ERR_HIP, std::string("dm_dr_set_item_paths: ") + hipGetErrorString(e));
  }
  dm_release(s->d_codes, s->d_item_off, s->d_items);
  s->d_codes = (long long *)n_codes; s->d_item_off = (int64_t *)n_off; s->d_items = (int32_t *)n_items;
  s->P = P; s->n_path_items = n_kept; s->max_bucket = (int)(uint32_t)cnt[2]; s->paths_loaded = true;
  return DM_OK;
}

int dm_dr_set_item_paths(dm_handle_t h, const int32_t *item_paths, int J) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_set_item_paths";
  DM_OWNER_ONLY(h, "dm_dr_set_item_paths");
  int rc = dts_check_model(h, who);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if (!item_paths) return fail(h, DM_ERR_INVALID, std::string(who) + ": null argument");
  if (J < 1) return fail(h, DM_ERR_INVALID, std::string(who) + ": the number of paths per item must be at least 1");
  if (s->num_item >= ((int64_t)1 << 31) / J) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": num_item * J must be below 2^31 (items are the sort's 32-bit values)");
  {
    long long sp = 1;
    for (int d = 0; d < s->D; d++) {
      if (sp > (((long long)1 << 62) - 1) / s->K) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": num_node^num_layer must be below 2^62");
      sp *= s->K;
    }
  }
  const int64_t n = s->num_item * J * s->D;
  for (int64_t i = 0; i < n; i++)
    if (item_paths[i] < 0 || item_paths[i] >= s->K) return fail(h, DM_ERR_INDEX, std::string(who) + ": path node outside [0, num_node)");
  HIPCHK(h, hipSetDevice(h->device));
  void *tab = nullptr;
  if ((rc = dm_alloc(h, &tab, (size_t)n * 4)) != DM_OK) return rc;
  const hipError_t e = hipMemcpyAsync(tab, item_paths, (size_t)n * 4, hipMemcpyHostToDevice, h->stream);
  if (e != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (rc == DM_OK) rc = dts_build_csr(h, s, (const int32_t *)tab, J);
  if (rc != DM_OK) {
    (void)hipStreamSynchronize(h->stream);
    dm_release(tab);
    return rc;
  }
  dm_release(s->d_item_paths);
  s->d_item_paths = (int32_t *)tab; s->J = J;
  return DM_OK;
}

int dm_dr_path_items_size(dm_handle_t h, int64_t *n_paths, int64_t *n_items) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_path_items_size");
  int rc = dts_check_model(h, "dm_dr_path_items_size");
  if (rc != DM_OK) return rc;
  if (!n_paths || !n_items) return fail(h, DM_ERR_INVALID, "dm_dr_path_items_size: null argument");
  if (!h->dr->paths_loaded) return fail(h, DM_ERR_STATE, "dm_dr_path_items_size: path -> items table not loaded");
  *n_paths = h->dr->P; *n_items = h->dr->n_path_items;
  return DM_OK;
}

int dm_dr_path_items_download(dm_handle_t h, int64_t *codes, int64_t *item_off, int32_t *items) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_path_items_download");
  int rc = dts_check_model(h, "dm_dr_path_items_download");
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if (!s->paths_loaded) return fail(h, DM_ERR_STATE, "dm_dr_path_items_download: path -> items table not loaded");
  if (!item_off || (s->P > 0 && !codes) || (s->n_path_items > 0 && !items)) return fail(h, DM_ERR_INVALID, "dm_dr_path_items_download: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (s->P > 0) HIPCHK(h, hipMemcpy(codes, s->d_codes, (size_t)s->P * 8, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(item_off, s->d_item_off, ((size_t)s->P + 1) * 8, hipMemcpyDeviceToHost));
  if (s->n_path_items > 0) HIPCHK(h, hipMemcpy(items, s->d_items, (size_t)s->n_path_items * 4, hipMemcpyDeviceToHost));
  return DM_OK;
}

int dm_dr_item_paths_download(dm_handle_t h, int32_t *out, int64_t n) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_item_paths_download");
  int rc = dts_check_set(h, "dm_dr_item_paths_download", false, true);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if (!out || n != s->num_item * s->J * s->D) return fail(h, DM_ERR_INVALID, "dm_dr_item_paths_download: out must hold num_item * J * D values");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, s->d_item_paths, (size_t)n * 4, hipMemcpyDeviceToHost));
  return DM_OK;
}

int dm_dr_train_set_load(dm_handle_t h, const int32_t *seq_ids, const int32_t *targets, int64_t N) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_train_set_load";
  DM_OWNER_ONLY(h, "dm_dr_train_set_load");
  int rc = dts_check_model(h, who);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  if (N < 1 || !seq_ids || !targets) return fail(h, DM_ERR_INVALID, std::string(who) + ": N must be positive and the arrays non-null");
  if (N >= ((int64_t)1 << 31)) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": N must be below 2^31 (the order holds 32-bit sample indices)");
  if ((rc = dr_check_ids(h, seq_ids, N * s->L)) != DM_OK) return rc;
  for (int64_t i = 0; i < N; i++)
    if (targets[i] < 0 || targets[i] >= s->num_item) return fail(h, DM_ERR_INDEX, std::string(who) + ": target outside [0, num_item)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  void *n_seq = nullptr, *n_tgt = nullptr, *n_ord = nullptr;
  if ((rc = dm_alloc(h, &n_seq, (size_t)N * s->L * 4)) != DM_OK || (rc = dm_alloc(h, &n_tgt, (size_t)N * 4)) != DM_OK || (rc = dm_alloc(h, &n_ord, (size_t)N * 4)) != DM_OK) {
    dm_release(n_seq, n_tgt, n_ord);
    return rc;
  }
  hipError_t e = hipMemcpyAsync(n_seq, seq_ids, (size_t)N * s->L * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(n_tgt, targets, (size_t)N * 4, hipMemcpyHostToDevice, h->stream);
  rc = e == hipSuccess ? LAUNCH(h, dts_iota_kernel, dim3(drt_blocks(h, N, 256)), dim3(256), 0, (int32_t *)n_ord, N) : fail(h, DM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (rc == DM_OK && (e = hipStreamSynchronize(h->stream)) != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (rc != DM_OK) {
    dm_release(n_seq, n_tgt, n_ord);
    return rc;
  }
  dm_release(s->d_ts_seq, s->d_ts_tgt, s->d_ts_order);
  s->d_ts_seq = (int32_t *)n_seq; s->d_ts_tgt = (int32_t *)n_tgt; s->d_ts_order = (int32_t *)n_ord; s->ts_N = N;
  return DM_OK;
}

int dm_dr_train_set_free(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_set_free");
  dm_dr_state *s = h->dr;
  if (!s) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dm_release(s->d_ts_seq, s->d_ts_tgt, s->d_ts_order);
  s->ts_N = 0;
  return DM_OK;
}

int dm_dr_train_set_size(dm_handle_t h, int64_t *n_samples, int32_t *n_paths_per_item) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_set_size");
  int rc = dts_check_model(h, "dm_dr_train_set_size");
  if (rc != DM_OK) return rc;
  if (!n_samples || !n_paths_per_item) return fail(h, DM_ERR_INVALID, "dm_dr_train_set_size: null argument");
  *n_samples = h->dr->d_ts_seq ? h->dr->ts_N : 0;
  *n_paths_per_item = h->dr->d_item_paths ? h->dr->J : 0;
  return DM_OK;
}

int dm_dr_train_set_shuffle(dm_handle_t h, uint64_t seed, int64_t epoch) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_set_shuffle");
  int rc = dts_check_set(h, "dm_dr_train_set_shuffle", true, false);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  const int64_t N = s->ts_N;
  HIPCHK(h, hipSetDevice(h->device));
  DevArena ar(s->ts_ws, 8);
  size_t o_k[2], o_v[2];
  for (int i = 0; i < 2; i++) { o_k[i] = ar.add((size_t)N * 8); o_v[i] = ar.add((size_t)N * 4); }
  const size_t o_tmp = ar.add(dev_sort_scratch_bytes(N));
  if ((rc = ar.commit(h)) != DM_OK) return rc;
  unsigned long long *kb[2] = {ar.ptr<unsigned long long>(o_k[0]), ar.ptr<unsigned long long>(o_k[1])};
  int32_t *vb[2] = {ar.ptr<int32_t>(o_v[0]), ar.ptr<int32_t>(o_v[1])};
  rc = timed(h, EV_DTS_SHUFFLE, dr_time_launches(), [&]() -> int {
    int where = 0;
    const int r = LAUNCH(h, dts_shuffle_keys_kernel, dim3(drt_blocks(h, N, 256)), dim3(256), 0, (unsigned long long)seed, (unsigned long long)epoch, N, kb[0], vb[0]);
    if (r != DM_OK) return r;
    HIPCHK(h, dev_radix_sort_pairs(h->stream, kb[0], vb[0], kb[1], vb[1], N, 0, 64, ar.ptr<uint32_t>(o_tmp), &where));
    HIPCHK(h, hipMemcpyAsync(s->d_ts_order, vb[where], (size_t)N * 4, hipMemcpyDeviceToDevice, h->stream));
    return DM_OK;
  });
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

int dm_dr_train_set_order_download(dm_handle_t h, int32_t *out) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_set_order_download");
  int rc = dts_check_set(h, "dm_dr_train_set_order_download", true, false);
  if (rc != DM_OK) return rc;
  if (!out) return fail(h, DM_ERR_INVALID, "dm_dr_train_set_order_download: null argument");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->dr->d_ts_order, (size_t)h->dr->ts_N * 4, hipMemcpyDeviceToHost));
  return DM_OK;
}

static int dts_check_range(dm_ctx *h, const char *who, int64_t offset, int64_t length) {
  const int64_t N = h->dr->ts_N;
  if (length < 1 || offset < 0 || offset > N || length > N - offset)
    return fail(h, DM_ERR_INVALID, std::string(who) + ": [offset, offset + length) must be a non-empty range inside [0, N]");
  return DM_OK;
}
// rows x L histories, then (paths != 0) S x J x D nodes, then (tgt != 0) S targets, in the handle's workspace
static int dts_gather(dm_ctx *h, int64_t offset, int64_t S, int rep, bool paths, bool tgt, int32_t **o_seq, int32_t **o_paths, int32_t **o_tgt) {
  dm_dr_state *s = h->dr;
  const size_t b_seq = DevArena::up((size_t)S * rep * s->L * 4), b_pa = paths ? DevArena::up((size_t)S * s->J * s->D * 4) : 0, b_t = tgt ? DevArena::up((size_t)S * 4) : 0;
  int rc = ensure_ws(h, b_seq + b_pa + b_t);
  if (rc != DM_OK) return rc;
  DtsGatherParams p{};
  p.seq = s->d_ts_seq; p.tgt = s->d_ts_tgt; p.order = s->d_ts_order; p.tab = paths ? s->d_item_paths : nullptr;
  p.offset = offset; p.S = S; p.L = s->L; p.J = paths ? s->J : 1; p.D = s->D; p.rep = rep;
  p.o_seq = (int32_t *)h->ws.p; p.o_paths = paths ? (int32_t *)((char *)h->ws.p + b_seq) : nullptr; p.o_tgt = tgt ? (int32_t *)((char *)h->ws.p + b_seq + b_pa) : nullptr;
  *o_seq = p.o_seq; *o_paths = p.o_paths; *o_tgt = p.o_tgt;
  const int64_t n = S * rep * s->L + (paths ? S * s->J * s->D : 0) + (tgt ? S : 0);
  return timed(h, EV_DTS_GATHER, dr_time_launches(), [&] { return LAUNCH(h, dts_gather_kernel, dim3(drt_blocks(h, n, 256)), dim3(256), 0, p); });
}

int dm_dr_train_set_forward_backward(dm_handle_t h, int64_t offset, int64_t length, int grouped, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_train_set_forward_backward";
  DM_OWNER_ONLY(h, "dm_dr_train_set_forward_backward");
  int rc = dts_check_set(h, who, true, true);
  if (rc != DM_OK) return rc;
  if ((rc = dr_train_check(h, who, true)) != DM_OK) return rc;
  if ((rc = dts_check_range(h, who, offset, length)) != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  const int64_t S = length, J = s->J;
  // the row limits of the step that follows, ahead of the workspace
  if (grouped) {
    // (shape only: the two array arguments of the check are tested for null and nothing else, the arrays do not exist yet; `s` stands in)
    if ((rc = drtg_check_shape(h, who, S, J, s, s, true)) != DM_OK) return rc;
  } else if (S > (int64_t)DRT_MAX_ROWS / J || S * J * (s->L + s->D - 1) >= ((int64_t)1 << 31)) {
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": range too large (at most 4 194 240 rows length * J, and length * J (L + D - 1) below 2^31): split it");
  }
  HIPCHK(h, hipSetDevice(h->device));
  int32_t *d_seq, *d_pa, *d_t;
  if ((rc = dts_gather(h, offset, S, grouped ? 1 : (int)J, true, false, &d_seq, &d_pa, &d_t)) != DM_OK) return rc;
  return grouped ? dm_dr_train_forward_backward_grouped_dev(h, d_seq, d_pa, S, J, out_loss) : dm_dr_train_forward_backward_dev(h, d_seq, d_pa, S * J, out_loss);
}

int dm_dr_train_set_rerank_forward_backward(dm_handle_t h, int64_t offset, int64_t length, double *out_loss) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_train_set_rerank_forward_backward";
  DM_OWNER_ONLY(h, "dm_dr_train_set_rerank_forward_backward");
  int rc = dts_check_set(h, who, true, false);
  if (rc != DM_OK) return rc;
  if ((rc = drr_check(h, who, true)) != DM_OK) return rc;
  if ((rc = dts_check_range(h, who, offset, length)) != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  const int64_t B = length, NS = s->rt->S;
  if (B > (int64_t)DRT_MAX_ROWS || B * std::max<int64_t>(s->L, NS + 1) >= ((int64_t)1 << 31))
    return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": range too large (at most 4 194 240 rows, and length max(L, S + 1) below 2^31): split it");
  if (2 * NS > s->num_item) return fail(h, DM_ERR_UNSUPPORTED, std::string(who) + ": the device draws negatives for 2 num_sampled <= num_item only");
  HIPCHK(h, hipSetDevice(h->device));
  int32_t *d_seq, *d_pa, *d_t;
  if ((rc = dts_gather(h, offset, B, 1, false, true, &d_seq, &d_pa, &d_t)) != DM_OK) return rc;
  return dm_dr_rerank_forward_backward_dev(h, d_seq, d_t, nullptr, B, out_loss);
}

// dm_dr_mstep_optimize over the resident set in storage order; J is the table's.  The codes are decoded into the table and the CSR follows.
int dm_dr_train_set_mstep(dm_handle_t h, int num_candidate_path, int mode, double decay_factor, int num_iteration, double penalty_factor, int penalty_poly_order,
                          uint64_t seed, int64_t *out_codes) {
  if (!h) return DM_ERR_INVALID;
  const char *who = "dm_dr_train_set_mstep";
  DM_OWNER_ONLY(h, "dm_dr_train_set_mstep");
  int rc = dts_check_set(h, who, true, true);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  const int C = num_candidate_path;
  const int64_t N = s->ts_N;
  if ((rc = drm_check(h, true, N, C, nullptr, nullptr, nullptr, who)) != DM_OK) return rc;
  if (mode != 0 && mode != 1) return fail(h, DM_ERR_INVALID, std::string(who) + ": mode must be 0 (batch) or 1 (streaming)");
  if (mode == 1 && (rc = dms_check_decay(h, who, &decay_factor)) != DM_OK) return rc;
  const int64_t num_item = s->num_item, total = 0;
  const int num_node = s->K, num_layer = s->D, num_path_per_item = s->J;
  DRA_ARGS(a);
  long long space = 0;
  if ((rc = dra_check_args(h, who, a, true, 0, 0, &space)) != DM_OK) return rc;
  if ((rc = dr_check_search(h, who, N, C, false)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const int J = s->J;
  DevArena io(h->dra_io, 8);
  const size_t o_out = io.add((size_t)num_item * J * 8);
  if ((rc = io.commit(h)) != DM_OK) return rc;
  long long *d_out = io.ptr<long long>(o_out);
  DrmResult r;
  if ((rc = mode == 0 ? drm_run_any(h, s->d_ts_seq, s->d_ts_tgt, N, C, nullptr, &r) : dms_run(h, s->d_ts_seq, s->d_ts_tgt, N, C, decay_factor, nullptr, &r)) != DM_OK) return rc;
  a.total = r.total;
  DraResult q;
  if ((rc = dra_run(h, who, a, space, r.item_off, r.codes, r.scores, (const long long *)r.occ, std::min<int64_t>(N, num_item), d_out, nullptr, nullptr, &q)) != DM_OK) return rc;
  s->paths_loaded = false;                                // (until the CSR of the new table stands)
  if ((rc = LAUNCH(h, dts_decode_kernel, dim3(drt_blocks(h, num_item * J, 256)), dim3(256), 0, d_out, num_item * J, s->D, s->K, s->d_item_paths)) != DM_OK) return rc;
  if (out_codes) HIPCHK(h, hipMemcpyAsync(out_codes, d_out, (size_t)num_item * J * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return dts_build_csr(h, s, s->d_item_paths, J);
}
