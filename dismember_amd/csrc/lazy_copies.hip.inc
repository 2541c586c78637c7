// The copies of a loaded model that are rebuilt on first use after the weights change (the eager ones are model_weights.hip.inc's),
// their stale flags and the rules that set them.  DESIGN.md §2 has the table: event -> what goes stale, and when the refresh is
// row-wise.  The state has to precede dm_ctx (it is a member) and the rebuilds need dm_ctx, so dm_hip.hip includes this file once per
// part and names the part: DM_LAZY_COPIES_PART 1 = struct LazyCopies, 2 = predicates, build kernels and the ensure_* rebuilds.
#if DM_LAZY_COPIES_PART == 1

// One state machine.  Its events are the methods below: the only code outside the rebuilds that writes a flag.
struct LazyCopies {
  // split-fp16 scorer (dm_set_scorer_mode): power-of-two scales, fp16 hi / lo planes of W1a, the pre-split table of the W kernel
  int sh_e = 0, sh_w = 0;
  unsigned *d_maxabs = nullptr;
  void *d_wsplit = nullptr, *d_emb_split = nullptr;
  size_t emb_split_bytes = 0;
  bool split_dirty = true, emb_split_dirty = true;      // the scales lag the weights; the pre-split table lags the scales
  // incremental refresh inside a training loop: the table changed only in the ACTIVE rows of the Adam step
  bool table_dense_change = true;   // ... unless something rewrote it wholesale since the last full scan
  bool sh_e_valid = false;          // sh_e comes from a full scan of the current table lineage
  bool emb_split_need_full = true;  // d_emb_split is not (scale sh_e, stale in active rows only)
  bool emb_split_patch = false;     // the last scale refresh was row-wise: so is the table's
  unsigned long long active_rows_host = 0;   // length of the active-row list at the last Adam step
  // general-rows split kernel: fp16 hi / lo planes of W1a and M = W1b att.W, then M in fp32
  int sh_r = 0; void *d_rows_split = nullptr; bool rows_split_dirty = true;
  // fp64 beam kernel: A / B fragments of att.W, W1a, W1b; l2.b read back with them
  void *d_frag64 = nullptr; double b2_64 = 0.0; bool frag64_dirty = true;
  // one-wave-per-SIMD beam kernel: the per-row setup table, row c = W1b (att.W emb32[c]) in fp32 (ensure_g_table)
  float *d_g_table = nullptr; size_t g_table_bytes = 0; bool g_table_dirty = true;
  bool g_table_declined = false;    // DM_G_TABLE unset: the table was too large for the free memory; not asked again before the next load
  // f64 model whose weights moved: the f32 copies the throughput beam kernels read are stale (the buffers are install_weights')
  bool f32_mirror_dirty = false;

  void loaded() { split_dirty = true; table_dense_change = true; g_table_dirty = true; g_table_declined = false; }
  void released() {
    dm_release(d_wsplit, d_maxabs, d_emb_split, d_rows_split, d_frag64);
    dm_release(d_g_table); g_table_bytes = 0; g_table_dirty = true; g_table_declined = false;
    emb_split_bytes = 0; table_dense_change = true; sh_e_valid = false; emb_split_need_full = true;
    split_dirty = true; rows_split_dirty = true; frag64_dirty = true; f32_mirror_dirty = false;
  }
  // dm_train_init: the weights did not move (the mirror flag stays), but changes of an earlier training run that are not yet in the
  // split copies can no longer be found from the new run's active rows.  The setup table stays as it is: it has no row-wise refresh
  void training_started() {
    if (split_dirty || emb_split_dirty) table_dense_change = true;
    active_rows_host = 0; split_dirty = true; frag64_dirty = true;
  }
  void adam_stepped(bool sparse, unsigned long long n_active, bool f64_model) {
    active_rows_host = n_active;
    if (!sparse) table_dense_change = true;         // the split scorer's copies can no longer be refreshed row by row
    split_dirty = true; frag64_dirty = true; f32_mirror_dirty = f32_mirror_dirty || f64_model;
    g_table_dirty = true;                           // att.W and W1b move in every step: every row of the setup table is stale
  }
  void mirror_rebuilt() { f32_mirror_dirty = false; split_dirty = true; table_dense_change = true; g_table_dirty = true; }
  // a clone's copy of its parent's state, taken after the parent brought its copies up to date.  The setup table is not among them: a
  // clone's search asks the owner for it, call by call (g_table_for_search), and never reads its own copy of these fields
  void clone_view() {
    split_dirty = false; emb_split_dirty = false; rows_split_dirty = false; frag64_dirty = false; f32_mirror_dirty = false;
    table_dense_change = false; emb_split_need_full = false; emb_split_patch = false; active_rows_host = 0;
  }
};

#elif DM_LAZY_COPIES_PART == 2

// ---- which copies a handle's searches read: the scorer arithmetic the beam kernels will use for this handle's model (dm_set_scorer_mode)
static bool use_split(const dm_ctx *h) {
  return (h->scorer_mode == DM_SCORER_SPLIT_F16 || h->scorer_mode == DM_SCORER_AUTO) && h->embed % 32 == 0;
}
// fp64 parity mode of the OTM search (otm64.hip.inc): in effect when f64 weights are loaded and the scorer mode is AUTO or F64
static bool use_f64_beam(const dm_ctx *h) {
  return h->dtype == DM_F64 && (h->scorer_mode == DM_SCORER_AUTO || h->scorer_mode == DM_SCORER_F64);
}

// AUTO mode inside a training loop: the split scorer's scales / fp16 copies are stale after every Adam step, and refreshing them is a
// pass (or three) over the whole table.  A request that is small next to that takes the fp32-input kernels, which read the fp32
// table as it is; both arithmetics meet the same tolerance (DESIGN.md §5).  An explicit DM_SCORER_SPLIT_F16 is always honoured.
static bool weights_in_motion(const dm_ctx *h) {
  return h->scorer_mode == DM_SCORER_AUTO && h->train_ready && (h->lazy.split_dirty || h->lazy.f32_mirror_dirty);
}
// ... the same question for a beam search, which reads the pre-split table as well
static bool split_refresh_pending(const dm_ctx *h) {
  return weights_in_motion(h) || (h->scorer_mode == DM_SCORER_AUTO && h->train_ready && h->lazy.emb_split_dirty);
}
// The refresh may touch the Adam step's active rows only: nothing else of the table has moved since the last full scan, whose scale
// 2^sh_e (a power of two: exact) stays as long as the active rows still fit it
static bool split_patchable(const dm_ctx *h) {
  return h->lazy.sh_e_valid && !h->lazy.table_dense_change && h->dtype == DM_F32;
}
static int64_t split_refresh_rows(const dm_ctx *h) { return split_patchable(h) ? (int64_t)h->lazy.active_rows_host : h->num_index; }

// ---- build kernels.  LIST = false: every row of the table (rows unused); LIST = true: the rows of a list (the rows an Adam step can
// have moved).  n counts elements of x.
template <bool LIST>
__global__ void dm_maxabs_kernel(const float *x, const int32_t *rows, int64_t n, int E, unsigned *out) {
  unsigned m = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = LIST ? (int64_t)rows[t / E] * E + (t % E) : t;
    const unsigned b = __float_as_uint(x[i]) & 0x7fffffffu;      // |x| as an ordered integer (NaN / inf sort highest)
    m = b > m ? b : m;
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = t > m ? t : m; }
  if ((threadIdx.x & 63) == 0 && (!LIST || m)) atomicMax(out, m);
}

// planes[p][s][nt][lane][i], lane = (g, m): W1a[16nt + m][32s + 16(i>>2) + 4g + (i&3)] * 2^sh_w split into fp16 hi (p=0) and
// lo (p=1); the column order is the one the beam kernel's gathered rows have inside a lane (two float4 per k-step)
__global__ void dm_build_wsplit_kernel(const float *wfrag, int E, float scale, _Float16 *planes) {
  const int NT = E / 16, NS = E / 32;
  const int n = NS * NT * 64 * 8;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int i = t & 7, lane = (t >> 3) & 63, nt = (t >> 9) % NT, s = (t >> 9) / NT;
    const int jc = 2 * s + (i >> 2);
    const float x = wfrag[(((size_t)jc * NT + nt) * 64 + lane) * 4 + (i & 3)] * scale;
    const _Float16 hi = (_Float16)x;
    const _Float16 lo = (_Float16)(x - (float)hi);
    planes[t] = hi;
    planes[(size_t)n + t] = lo;
  }
}

// The table as the one-wave-per-SIMD kernel gathers it: every fp32 value x already split into hi = RNE16(x 2^s) and
// lo = RNE16(x 2^s - hi), laid out so that the lane group g of a tile finds, per row and k-step, its two MFMA B operands as 32
// contiguous bytes: out[row][s][g][0..7] = hi of columns 32s + 16(i>>2) + 4g + (i&3), out[row][s][g][8..15] = lo of the same.
// Same bytes per row as the fp32 table (E * 4); identical values to the split the LDS-fed kernel does per tile.
template <bool LIST>
__global__ void dm_build_emb_split_kernel(const float *emb, const int32_t *rows, int64_t n_rows, int E, float scale, _Float16 *out) {
  const int64_t n8 = n_rows * (int64_t)(E / 8);        // groups of 8 values = one (row, s, g)
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n8; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = LIST ? (int64_t)rows[t / (E / 8)] : t / (E / 8);
    const int sg = (int)(t % (E / 8)), s_ = sg >> 2, g = sg & 3;
    const float *src = emb + row * E + 32 * s_ + 4 * g;
    _Float16 *dst = out + row * (int64_t)(2 * E) + (int64_t)sg * 16;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const float x = src[16 * (i >> 2) + (i & 3)] * scale;
      const _Float16 hi = (_Float16)x;
      dst[i] = hi;
      dst[8 + i] = (_Float16)(x - (float)hi);
    }
  }
}

// power-of-two shift that puts max|x| into [2^13, 2^14): every scaled value and every rounding of it stays below the fp16
// maximum, and fp16 subnormals only start 2^27 below the largest element
static int split_shift(unsigned maxbits) {
  if (maxbits == 0 || maxbits >= 0x7f800000u) return 0;
  float m;
  int e;
  memcpy(&m, &maxbits, 4);
  frexpf(m, &e);               // m = f * 2^e, f in [0.5, 1)
  return std::clamp(14 - e, -40, 40);
}

// ---- the rebuilds: no-ops while their copy is current; each holds h->mu (an owner thread and clone threads may search concurrently)

// f64 model whose weights moved (dm_adam_step): bring the f32 copies the throughput-mode beam kernels read up to date
// (table, fragment-ordered small matrices, b1 / w2 / b2).  No-op for f32 models and while nothing changed.
static int ensure_f32_mirror(dm_ctx *h) {
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  if (h->dtype != DM_F64 || !h->lazy.f32_mirror_dirty) return DM_OK;
  model_changed(h);
  int rc = mirror_table32(h);
  if (rc == DM_OK) rc = derive_small(h, DERIVE_F32_MIRROR);
  if (rc != DM_OK) return rc;
  h->lazy.mirror_rebuilt();
  return DM_OK;
}

// scales (2^sh_e from max|emb|: one read of the table; 2^sh_w from max|W1a|) and the fp16 planes of W1a: what every split kernel
// needs.  The pre-split copy of the table (ensure_split) is a second, larger step only the beam kernels take.
static int ensure_split_scales(dm_ctx *h) {
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  LazyCopies &z = h->lazy;
  if (!z.split_dirty && z.d_wsplit) return DM_OK;
  model_changed(h);
  const int E = h->embed;
  if (E % 32 != 0) return fail(h, DM_ERR_UNSUPPORTED, "the split-fp16 scorer needs an embedding size that is a multiple of 32");
  if (!z.d_wsplit) ALLOC(h, z.d_wsplit, (size_t)E * E * 4);
  if (!z.d_maxabs) ALLOC(h, z.d_maxabs, 8);
  // a training loop whose Adam steps visit the active rows only: the last full scan's scale stays, only those rows are re-split
  bool patch = h->train_ready && split_patchable(h) && h->train.active_list;
  unsigned mb[2];
  for (;;) {
    HIPCHK(h, hipMemsetAsync(z.d_maxabs, 0, 8, h->stream));
    if (patch) {
      if (z.active_rows_host) LAUNCHCHK(h, dm_maxabs_kernel<true>, dim3(1024), dim3(256), 0, h->d_emb32, h->train.active_list, (int64_t)z.active_rows_host * E, E, z.d_maxabs);
    } else
      LAUNCHCHK(h, dm_maxabs_kernel<false>, dim3(4096), dim3(256), 0, h->d_emb32, nullptr, h->num_index * (int64_t)E, E, z.d_maxabs);
    LAUNCHCHK(h, dm_maxabs_kernel<false>, dim3(16), dim3(256), 0, (const float *)h->d_wfrag, nullptr, (int64_t)E * E, E, z.d_maxabs + 1);
    HIPCHK(h, hipMemcpyAsync(mb, z.d_maxabs, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (patch && mb[0] != 0 && split_shift(mb[0]) < z.sh_e) { patch = false; continue; }    // an active row outgrew the scale: full scan
    break;
  }
  if (!patch) {
    z.sh_e = split_shift(mb[0]);
    z.sh_e_valid = true; z.table_dense_change = false; z.emb_split_need_full = true;
  }
  z.emb_split_patch = patch;
  z.sh_w = split_shift(mb[1]);
  LAUNCHCHK(h, dm_build_wsplit_kernel, dim3(64), dim3(256), 0, (const float *)h->d_wfrag, E, ldexpf(1.0f, z.sh_w), (_Float16 *)z.d_wsplit);
  z.split_dirty = false; z.emb_split_dirty = true; z.rows_split_dirty = true;      // the table's and the rows planes' turn
  return DM_OK;
}

static int ensure_split(dm_ctx *h) {
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  int rc = ensure_split_scales(h);
  if (rc != DM_OK) return rc;
  LazyCopies &z = h->lazy;
  if (!z.emb_split_dirty && z.d_emb_split) return DM_OK;
  model_changed(h);
  const int E = h->embed;
  // the beam kernels gather pre-split rows: a second copy of the table (same size), refreshed whenever the weights change — as a whole,
  // or in the active rows only when nothing else can have moved
  const size_t bytes = (size_t)h->num_index * E * 4;
  if (z.emb_split_bytes != bytes) {
    dm_release(z.d_emb_split); z.emb_split_bytes = 0;
    ALLOC(h, z.d_emb_split, bytes);
    z.emb_split_bytes = bytes;
    z.emb_split_need_full = true;
  }
  if (z.emb_split_need_full || !z.emb_split_patch) {
    LAUNCHCHK(h, dm_build_emb_split_kernel<false>, dim3(8192), dim3(256), 0, h->d_emb32, nullptr, h->num_index, E, ldexpf(1.0f, z.sh_e), (_Float16 *)z.d_emb_split);
    z.emb_split_need_full = false;
  } else if (z.active_rows_host) {
    LAUNCHCHK(h, dm_build_emb_split_kernel<true>, dim3(1024), dim3(256), 0, h->d_emb32, h->train.active_list, (int64_t)z.active_rows_host, E, ldexpf(1.0f, z.sh_e),
              (_Float16 *)z.d_emb_split);
  }
  z.emb_split_dirty = false;
  return DM_OK;
}

// The setup table of the one-wave-per-SIMD kernel: row c = W1b (att.W emb32[c]), built by the kernel's own two-stage product
// (dm_build_g_table_kernel, beam_kernel_w.hip.inc) from the f32 table and the fragment orders the kernel's setup reads.  There is no
// row-wise refresh: att.W and W1b move in every Adam step, and with them every row.
static int ensure_g_table(dm_ctx *h) {
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  int rc = ensure_f32_mirror(h);          // an f64 model builds from its f32 mirror
  if (rc != DM_OK) return rc;
  LazyCopies &z = h->lazy;
  if (!z.g_table_dirty && z.d_g_table) return DM_OK;
  const int E = h->embed;
  const size_t bytes = (size_t)h->num_index * E * 4;
  if (z.g_table_bytes != bytes || !z.d_g_table) {
    dm_release(z.d_g_table); z.g_table_bytes = 0;
    ALLOC(h, z.d_g_table, bytes);
    z.g_table_bytes = bytes;
  }
  const int64_t waves = (h->num_index + 15) / 16, blocks = (waves + DMW_NWAVES - 1) / DMW_NWAVES;
  const int grid = (int)std::min<int64_t>(blocks, (int64_t)h->n_cu * 8);
  rc = dispatch_E<32>(h, E, "the setup table needs an embedding size of 32, 64 or 128", [&](auto e) {
    return LAUNCH(h, dm_build_g_table_kernel<decltype(e)::value>, dim3(grid), dim3(DMW_BLOCK), 0, h->d_emb32, (const f32x4 *)h->d_afrag, (const f32x4 *)h->d_bfrag, h->num_index,
                  z.d_g_table);
  });
  if (rc != DM_OK) return rc;
  z.g_table_dirty = false;
  return DM_OK;
}

// The table a search on the one-wave-per-SIMD kernel reads, or null: the kernel then runs the two products per user.  DM_G_TABLE
// (read per call: the tests run both routes in one process) = 0 never, 1 always (a table that cannot be allocated fails the search),
// unset: unless the table is stale inside a training session (every Adam step would pay the whole rebuild) or its bytes exceed a
// quarter of the free device memory (remembered until the next load).  A clone reads its owner's table, built on the owner's stream.
static int g_table_for_search(dm_ctx *h, const float **table) {
  *table = nullptr;
  const int knob = env_off("DM_G_TABLE") ? 0 : env_on("DM_G_TABLE") ? 1 : -1;
  if (knob == 0) return DM_OK;
  dm_ctx *o = h->parent ? h->parent : h;
  std::lock_guard<std::recursive_mutex> lk_(o->mu);
  LazyCopies &z = o->lazy;
  const bool stale = z.g_table_dirty || !z.d_g_table;
  if (stale && knob < 0) {
    if (o->train_ready || z.g_table_declined) return DM_OK;
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    if ((size_t)o->num_index * o->embed * 4 > free_b / 4) { z.g_table_declined = true; return DM_OK; }
  }
  if (stale) {
    const int rc = ensure_g_table(o);
    if (rc != DM_OK) { if (o != h) h->err = o->err; return rc; }
    if (o != h) HIPCHK(h, hipStreamSynchronize(o->stream));
  }
  *table = z.d_g_table;
  return DM_OK;
}

// the split scorer's four scale parameters of a beam launch: 2^sh_e, 2^(-2 sh_e), 2^(sh_e + sh_w), 2^-(sh_e + sh_w)
static void fill_split_scales(const dm_ctx *h, BeamParams &p) {
  const int e = h->lazy.sh_e, ew = e + h->lazy.sh_w;
  p.emb_scale = ldexpf(1.0f, e); p.score_unscale = ldexpf(1.0f, -2 * e); p.acc_scale = ldexpf(1.0f, ew); p.out_unscale = ldexpf(1.0f, -ew);
}

// fp16 planes of the general-rows split kernel (rows_kernel.hip.inc): follow the weights like the beam kernels' planes
static int ensure_rows_split(dm_ctx *h) {
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  int rc = ensure_split_scales(h);     // sh_e = the table's scale: one read of the table per weight change, shared with the beam kernels
  if (rc != DM_OK) return rc;
  LazyCopies &z = h->lazy;
  if (!z.rows_split_dirty && z.d_rows_split) return DM_OK;
  const int E = h->embed;
  const size_t plane_bytes = (size_t)4 * E * E * 2;
  if (!z.d_rows_split) ALLOC(h, z.d_rows_split, plane_bytes + (size_t)E * E * 4);
  float *Mbuf = (float *)((char *)z.d_rows_split + plane_bytes);
  HIPCHK(h, hipMemsetAsync(z.d_maxabs, 0, 8, h->stream));
  LAUNCHCHK(h, dm_rows_m_kernel, dim3(64), dim3(256), 0, h->d_attA, h->d_w1aA, h->d_w1bA, E, Mbuf, z.d_maxabs);
  unsigned mb[2];
  HIPCHK(h, hipMemcpyAsync(mb, z.d_maxabs, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  model_changed(h);
  z.sh_r = split_shift(mb[0] > mb[1] ? mb[0] : mb[1]);
  LAUNCHCHK(h, dm_build_rows_planes_kernel, dim3(64), dim3(256), 0, h->d_w1aA, Mbuf, E, ldexpf(1.0f, z.sh_r), (_Float16 *)z.d_rows_split);
  z.rows_split_dirty = false;
  return DM_OK;
}

// A / B fragments of the fused fp64 beam kernel (beam_kernel_f64.hip.inc) and of the grouped training step, and l2.b
static int ensure_frags64(dm_ctx *h) {
  std::lock_guard<std::recursive_mutex> lk_(h->mu);
  LazyCopies &z = h->lazy;
  const int E = h->embed;
  const size_t n = (size_t)E * E;
  if (!z.d_frag64) { ALLOC(h, z.d_frag64, 3 * n * 8); z.frag64_dirty = true; }
  if (!z.frag64_dirty) return DM_OK;
  model_changed(h);
  const double *base = (const double *)h->d_compact;
  const double *att_w = base + h->num_index * E, *l1_w = att_w + n;
  double *f = (double *)z.d_frag64;
  LAUNCHCHK(h, dm_build_frags64_kernel, dim3(64), dim3(256), 0, att_w, l1_w, E, f, f + n, f + 2 * n);
  HIPCHK(h, hipMemcpyAsync(&z.b2_64, l1_w + 2 * n + 2 * E, 8, hipMemcpyDeviceToHost, h->stream));      // l2.b: a kernel argument
  HIPCHK(h, hipStreamSynchronize(h->stream));
  z.frag64_dirty = false;
  return DM_OK;
}

#else
#error "define DM_LAZY_COPIES_PART as 1 or 2 before including lazy_copies.hip.inc"
#endif
#undef DM_LAZY_COPIES_PART
