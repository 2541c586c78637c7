// From "a compact vector in device memory" to a loaded model (DESIGN.md §2): the one place that states how the derived copies of a
// DIN model [emb ; att.W ; l1.W ; l1.b ; l2.W ; l2.b] are made.  Every fragment order and transpose is written by
// dm_refresh_fragments_kernel (train_kernel.hip.inc) on the handle's stream; no host code restates a layout.

// What derive_small rebuilds.  An f32 model has one side and always gets all of it.  An f64 model has two: the copies in its own type
// (plain transposes, d_tr64) follow every weight change; its f32 mirror (d_tail32 -> the fragment orders, b1 / w2 / b2 the throughput
// kernels read) is rebuilt lazily by ensure_f32_mirror.
enum { DERIVE_OWN = 1, DERIVE_F32_MIRROR = 2, DERIVE_ALL = 3 };

// Everything derived from the tail of h->d_compact, on the device, on h->stream.  Buffers the handle does not hold (d_tr64 and the
// transposed fragments exist with training state or after the first matrix-pipe forward) are skipped by the kernel's null guards.
// The f32 side ends with the stream drained: h->b2 is a host value.
static int derive_small(dm_ctx *h, int what) {
  const int E = h->embed;
  const int64_t n2 = (int64_t)E * E;
  const float *tail32 = (const float *)h->d_compact + h->num_index * E;
  const bool f64 = h->dtype == DM_F64;
  if (f64) {
    const double *tail = (const double *)h->d_compact + h->num_index * E;
    if (what & DERIVE_OWN) {
      double *const f = (double *)h->d_tr64, *const no = nullptr;      // six E x E blocks: A fragments of att.W, W1a, W1b, then of their transposes
      auto blk = [&](int i) { return f ? f + i * n2 : no; };
      const int rc = dispatch_E(h, E, "unsupported embed size", [&](auto e) {
        return LAUNCH(h, (dm_refresh_fragments_kernel<double, decltype(e)::value>), dim3(64), dim3(256), 0, tail, tail + n2, no, no, no, blk(0), blk(1), blk(2), blk(3), blk(4),
                      blk(5), (double *)h->d_att_wT_t, (double *)h->d_l1T_t);
      });
      if (rc != DM_OK) return rc;
    }
    if (!(what & DERIVE_F32_MIRROR)) return DM_OK;
    LAUNCHCHK(h, dm_f64_to_f32_kernel, dim3(64), dim3(256), 0, tail, (float *)h->d_tail32, 3 * n2 + 2 * E + 1);
    tail32 = (const float *)h->d_tail32;
  }
  // the transposed fragments and the plain transposes are in the model's own type: not part of an f64 model's f32 mirror
  float *const no = nullptr;
  const int rc = dispatch_E(h, E, "unsupported embed size", [&](auto e) {
    return LAUNCH(h, (dm_refresh_fragments_kernel<float, decltype(e)::value>), dim3(64), dim3(256), 0, tail32, tail32 + n2, (float *)h->d_wfrag, (float *)h->d_afrag,
                  (float *)h->d_bfrag, (float *)h->d_attA, (float *)h->d_w1aA, (float *)h->d_w1bA, f64 ? no : (float *)h->d_attTA, f64 ? no : (float *)h->d_w1aTA,
                  f64 ? no : (float *)h->d_w1bTA, f64 ? no : (float *)h->d_att_wT_t, f64 ? no : (float *)h->d_l1T_t);
  });
  if (rc != DM_OK) return rc;
  const float *b = tail32 + 3 * n2;      // l1.b ; l2.W ; l2.b
  HIPCHK(h, hipMemcpyAsync(h->d_b1, b, E * 4, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_w2, b + E, E * 4, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(&h->b2, b + 2 * E, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DM_OK;
}

// f64 model: the f32 table the throughput beam kernels read
static int mirror_table32(dm_ctx *h) {
  return LAUNCH(h, dm_f64_to_f32_kernel, dim3(4096), dim3(256), 0, (const double *)h->d_compact, h->d_emb32, h->num_index * (int64_t)h->embed);
}

// The handle takes ownership of a device-resident compact vector of `dtype` with the kernels' embed size E (E_model: the model's own,
// smaller when the loader zero-padded it) and becomes a loaded model.  The callers have validated everything: from the first line on
// the previous model is gone and d_compact belongs to the handle, also when a later step fails (the next load or dm_destroy frees it).
// All device work is on h->stream, so a vector the caller filled on that stream (dm_fill_normal) is read in order.
static int install_weights(dm_ctx *h, int dtype, int E, int E_model, int64_t num_index, void *d_compact) {
  free_weights(h);
  h->d_compact = d_compact; h->dtype = dtype; h->embed = E; h->embed_log = E_model; h->num_index = num_index;
  const size_t n2 = (size_t)E * E, es = dtype == DM_F64 ? 8 : 4;
  ALLOC(h, h->d_wfrag, n2 * 4); ALLOC(h, h->d_afrag, n2 * 4); ALLOC(h, h->d_bfrag, n2 * 4);
  ALLOC(h, h->d_attA, n2 * 4); ALLOC(h, h->d_w1aA, n2 * 4); ALLOC(h, h->d_w1bA, n2 * 4);
  ALLOC(h, h->d_b1, E * 4); ALLOC(h, h->d_w2, E * 4);
  ALLOC(h, h->d_att_wT_t, n2 * es); ALLOC(h, h->d_l1T_t, 2 * n2 * es);
  if (dtype == DM_F64) {      // the f32 mirror is made eagerly: the first search after a load pays nothing for it
    ALLOC(h, h->d_emb32, (size_t)num_index * E * 4);
    h->emb32_owned = true;
    ALLOC(h, h->d_tail32, (3 * n2 + 2 * E + 1) * 4);
    const int rc = mirror_table32(h);
    if (rc != DM_OK) return rc;
  } else h->d_emb32 = (float *)d_compact;
  const int rc = derive_small(h, DERIVE_ALL);      // (ends with the stream drained)
  if (rc != DM_OK) return rc;
  h->w_loaded = true;
  h->lazy.loaded();
  return DM_OK;
}

template <typename T>
static int load_weights_host(dm_ctx *h, int dtype, int E, int64_t num_index, const T *w, int64_t n_elems) {
  if (n_elems != compact_len_for(num_index, E)) return fail(h, DM_ERR_INVALID, "dm_load_weights_din: n_elems does not match the DIN layout for (E, num_index)");
  const int Ep = native_embed(E);
  std::vector<T> padded;
  if (Ep != E) {
    padded.resize((size_t)compact_len_for(num_index, Ep));
    pad_compact<T>(w, E, Ep, num_index, padded.data());
    w = padded.data();
  }
  const size_t bytes = (size_t)compact_len_for(num_index, Ep) * sizeof(T);
  free_weights(h);      // before the new vector is allocated: a reload never holds two models on the device
  void *d = nullptr;
  ALLOC(h, d, bytes);
  if (hipMemcpy(d, w, bytes, hipMemcpyHostToDevice) != hipSuccess) { dm_release(d); return fail(h, DM_ERR_HIP, "dm_load_weights_din: upload failed"); }
  return install_weights(h, dtype, Ep, E, num_index, d);
}

int dm_load_weights_din(dm_handle_t h, int dtype, int E, int64_t num_index, const void *compact, int64_t n_elems) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_weights_din");
  if (!compact || num_index <= 0) return fail(h, DM_ERR_INVALID, "dm_load_weights_din: bad arguments");
  if (E < 1 || E > 128)
    return fail(h, DM_ERR_UNSUPPORTED, "dm_load_weights_din: embed size must be 1 .. 128 (sizes other than 16 / 32 / 64 / 128 are zero-padded to the next of them; at E = 256 the "
                "fp16 hi / lo planes of W1a are 256 KB against 64 KB of AccVGPRs per wave and 160 KB of LDS per CU: the weights would have to stream "
                "per 128-column slab, ~4.3 x the E = 128 time per scored row — DESIGN.md, not built)");
  if (dtype != DM_F32 && dtype != DM_F64) return fail(h, DM_ERR_INVALID, "dm_load_weights_din: dtype");
  HIPCHK(h, hipSetDevice(h->device));
  return dtype == DM_F32 ? load_weights_host<float>(h, dtype, E, num_index, (const float *)compact, n_elems)
                         : load_weights_host<double>(h, dtype, E, num_index, (const double *)compact, n_elems);
}

// A compact vector already in device memory (dm_load_model, synthetic models filled in place): ownership passes to the handle once the
// arguments are accepted; a call that fails validation leaves the handle untouched and the buffer with the caller.
static int load_weights_dev(dm_ctx *h, const std::string &who, int dtype, int E, int64_t num_index, void *d_compact, int64_t n_elems) {
  if (!d_compact || num_index <= 0) return fail(h, DM_ERR_INVALID, who + ": bad arguments");
  if (E != 16 && E != 32 && E != 64 && E != 128) return fail(h, DM_ERR_UNSUPPORTED, who + ": embed size must be 16, 32, 64 or 128");
  if (n_elems != compact_len_for(num_index, E)) return fail(h, DM_ERR_INVALID, who + ": n_elems does not match the DIN layout for (E, num_index)");
  HIPCHK(h, hipSetDevice(h->device));
  return install_weights(h, dtype, E, E, num_index, d_compact);
}

int dm_load_weights_din_dev(dm_handle_t h, int E, int64_t num_index, float *d_compact, int64_t n_elems) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_weights_din_dev");
  return load_weights_dev(h, "dm_load_weights_din_dev", DM_F32, E, num_index, d_compact, n_elems);
}

// the fp64 counterpart (the reference's OTM model is DIN[Double]): same ownership rule
int dm_load_weights_din_dev_f64(dm_handle_t h, int E, int64_t num_index, double *d_compact, int64_t n_elems) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_weights_din_dev_f64");
  return load_weights_dev(h, "dm_load_weights_din_dev_f64", DM_F64, E, num_index, d_compact, n_elems);
}
