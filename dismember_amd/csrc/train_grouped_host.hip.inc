// Host side of the user-grouped training step (train_grouped_f64.hip.inc): a batch in which every user contributes `n` candidate rows
// that share the user's history — the OTM trainer's level batch (O/dataset/MiniBatch.scala:17-40) and TDM's
// MiniBatch.transformWithMask (T/dataset/MiniBatch.scala:129-147).

static bool tg_enabled() {
  return !env_off("DM_TRAIN_GROUPED");       // DM_TRAIN_GROUPED=0: the grouped entry point expands to plain rows (A/B, tests)
}

static size_t tg_up(size_t v) { return (v + 255) & ~(size_t)255; }

template <int E>
static int tg_launch_E(dm_ctx *h, const int32_t *d_seq, const unsigned *d_umask, const int32_t *d_codes, const float *d_labels, int64_t U,
                       int n, int L) {
  const int64_t B = U * (int64_t)n;
  const size_t ue = (size_t)U * 16 * E;      // doubles per per-user array
  // workspace: Z [B][E], P [B][16], DS [B][16], GL [B], logits [B], eight per-user arrays, the work counter
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o_ = off; off += tg_up(bytes); return o_; };
  const size_t Bs = (size_t)B + 16;           // + 16 slack rows (the dead rows of a user's last tile store there)
  const size_t o_Z = take(Bs * E * 8), o_P = take(Bs * 16 * 8), o_DS = take(Bs * 16 * 8), o_GL = take(Bs * 8),
               o_lg = take(Bs * 8), o_ub = take(8 * ue * 8), o_cnt = take(64);
  int rc = ensure_ws(h, off);
  if (rc != DM_OK) return rc;
  if ((rc = ensure_frags64(h)) != DM_OK) return rc;       // att.W / W1b fragments of the fp64 beam kernel's orders + l2.b
  char *ws = (char *)h->ws.p;
  TgBufs bufs;
  {
    double *ubase = (double *)(ws + o_ub);
    bufs.Kf = ubase; bufs.Gbf = ubase + ue; bufs.Krows = ubase + 2 * ue; bufs.Grows = ubase + 3 * ue; bufs.T1rows = ubase + 4 * ue;
    bufs.dGrows = ubase + 5 * ue; bufs.dKrows = ubase + 6 * ue; bufs.dTrows = ubase + 7 * ue;
  }
  const size_t n2 = (size_t)E * E;
  const double *base = (const double *)h->d_compact;
  const double *att_w = base + h->num_index * E, *l1_w = att_w + n2, *b1 = l1_w + 2 * n2, *w2 = b1 + E;
  const double *f64f = (const double *)h->lazy.d_frag64;          // w1aA, attA, w1bB
  const double *tr = (const double *)h->d_tr64;              // attA, w1aA, w1bA, attTA, w1aTA, w1bTA (training fragment order)
  double *grad = (double *)h->train.grad;
  // every launch gets an event pair (dm_kernel_timing_get_kind: EV_TG_SETUP = per-user setup, EV_TG_ROWS = the row kernel, EV_TG_WGRAD_A = dW1a +
  // per-user sums, EV_TG_USER_BWD = per-user backward, EV_TG_WGRAD_B = dW1b / datt.W): bench.py prices the row kernel against the fp64 matrix peak from these
  // ---- per-user setup
  TgSetupParams sp{};
  sp.emb = base; sp.num_index = h->num_index; sp.attA = f64f + n2; sp.w1bB = f64f + 2 * n2; sp.b1 = b1; sp.seq = d_seq; sp.U = U; sp.L = L; sp.b = bufs;
  if ((rc = timed(h, EV_TG_SETUP, true, [&] { return LAUNCH(h, tg_setup_kernel<E>, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, sp); })) != DM_OK) return rc;
  // ---- rows: forward + backward
  TgRowsParams rp{};
  rp.emb = base; rp.num_index = h->num_index; rp.l1_w = l1_w; rp.w2 = w2; rp.b2 = h->lazy.b2_64;
  rp.codes = d_codes; rp.labels = d_labels; rp.umask = d_umask; rp.U = U; rp.n = n; rp.L = L;
  rp.tiles_per_user = (n + 15) / 16;
  {
    // work items of about five tiles: a wave's last item ends within a few percent of the launch's end, and consecutive items of a user
    // run close in time (their fragments come from L2)
    const int64_t waves = (int64_t)h->n_cu * TG_NWAVES;
    int ct = 5;
    while (ct > 1 && U * ((rp.tiles_per_user + ct - 1) / ct) < 8 * waves) ct--;
    rp.chunk_tiles = ct; rp.chunks_per_user = (rp.tiles_per_user + ct - 1) / ct;
  }
  rp.inv_B = 1.0 / (double)B; rp.sm_scale = sm_scale64(h); rp.b = bufs;
  rp.Z = (double *)(ws + o_Z); rp.P = (double *)(ws + o_P); rp.DS = (double *)(ws + o_DS); rp.GL = (double *)(ws + o_GL); rp.logits = (double *)(ws + o_lg);
  rp.grad = grad; rp.next_item = (unsigned long long *)(ws + o_cnt);
  HIPCHK(h, hipMemsetAsync(ws + o_cnt, 0, 64, h->stream));
  const int lds = E * E * 8 + E * 8;
  {
    const int64_t items = U * rp.chunks_per_user;
    int64_t blocks = (items + TG_NWAVES - 1) / TG_NWAVES;
    if (blocks > h->n_cu) blocks = h->n_cu;
    auto go = [&](void (*tg_rows_kernel_E_KQ)(TgRowsParams)) -> int {      // (the parameter's name is what LAUNCH puts into an error message)
      HIPCHK(h, lds_opt_in(tg_rows_kernel_E_KQ, lds));
      return timed(h, EV_TG_ROWS, true, [&] { return LAUNCH(h, tg_rows_kernel_E_KQ, dim3((unsigned)blocks), dim3(TG_BLOCK), lds, rp); });
    };
    switch ((L + 3) / 4) {
      case 1: rc = go(tg_rows_kernel<E, 1>); break;
      case 2: rc = go(tg_rows_kernel<E, 2>); break;
      case 3: rc = go(tg_rows_kernel<E, 3>); break;
      default: rc = go(tg_rows_kernel<E, 4>); break;
    }
    if (rc != DM_OK) return rc;
  }
  double *g_l2b = grad + h->num_index * E + 3 * (int64_t)n2 + 2 * E;
  if ((rc = LAUNCH(h, tg_loss_kernel, dim3((unsigned)std::min<int64_t>((B + 255) / 256, 1024)), dim3(256), 0, rp.logits, rp.GL, d_labels, B, (double *)h->d_loss, g_l2b)) != DM_OK)
    return rc;
  // ---- dW1a + the per-user sums dG, dK + l1.b / l2.W gradients
  TgWgradParams wp{};
  wp.emb = base; wp.num_index = h->num_index; wp.codes = d_codes; wp.Z = rp.Z; wp.P = rp.P; wp.DS = rp.DS; wp.GL = rp.GL; wp.w2 = w2;
  wp.U = U; wp.n = n; wp.b = bufs; wp.grad = grad;
  constexpr int NT = E / 16, RT = NT < 4 ? NT : 4, NBq = (NT / RT) * (NT / RT);
  {
    const int64_t want = std::max<int64_t>(1, (int64_t)h->n_cu * 8 / NBq);     // two waves per SIMD, a few chunks per slot
    wp.users_per_chunk = (int)std::max<int64_t>(1, (U + 4 * want - 1) / (4 * want));
    const unsigned chunks = (unsigned)((U + wp.users_per_chunk - 1) / wp.users_per_chunk);
    if ((rc = timed(h, EV_TG_WGRAD_A, true, [&] { return LAUNCH(h, tg_wgrad_kernel<E>, dim3(1, chunks), dim3(64 * NBq), 0, wp); })) != DM_OK) return rc;
  }
  // ---- per-user backward, then dW1b / datt.W over the U x 16 per-user rows
  TgUserBwdParams up{};
  up.attTA = (const f64x4 *)(tr + 3 * n2); up.w1bTA = (const f64x4 *)(tr + 5 * n2); up.seq = d_seq; up.U = U; up.L = L; up.num_index = h->num_index;
  up.b = bufs; up.grad = grad;
  if ((rc = timed(h, EV_TG_USER_BWD, true, [&] { return LAUNCH(h, tg_user_bwd_kernel<E>, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, up); })) != DM_OK) return rc;
  WGradParamsT<double> wg{};
  wg.emb = base; wg.codes = nullptr; wg.DZ = bufs.dGrows; wg.AT = bufs.T1rows; wg.DA = bufs.dTrows; wg.CB = bufs.Krows;
  wg.B = U * 16; wg.num_index = h->num_index; wg.grad = grad; wg.mat_base = 1;
  {
    const int64_t want = std::max<int64_t>(1, (int64_t)h->n_cu * 16 / (2 * NBq));
    wg.chunk = std::max<int64_t>(128, (((wg.B + want - 1) / want) + 7) / 8 * 8);
    const int chunks = (int)((wg.B + wg.chunk - 1) / wg.chunk);
    if ((rc = timed(h, EV_TG_WGRAD_B, true, [&] { return LAUNCH(h, (dm_wgrad_kernel<double, E>), dim3(2 * NBq, chunks), dim3(64), 0, wg); })) != DM_OK) return rc;
  }
  return DM_OK;
}

// all pointers device.  d_seq [U][L] node codes (-1 = padding), d_umask [U] (may be null: nothing masked), d_codes / d_labels [U * n]
// user-major.  Accumulates the batch's gradients (mean BCE over the U * n rows) into the handle's gradient, like train_fb_dev.
static int train_fb_grouped_dev(dm_ctx *h, const int32_t *d_seq, const unsigned *d_umask, const int32_t *d_codes, const float *d_labels,
                                int64_t U, int n, int L, float *loss) {
  const int64_t B = U * (int64_t)n;
  if (h->dtype != DM_F64 || L > DM_MAXL || !tg_enabled()) {
    // f32 models and long histories: the same batch as plain rows
    int32_t *rseq = nullptr; unsigned *rmask = nullptr;
    DevTemps t(h);
    int rc = t.alloc(rseq, (size_t)B * L * 4);
    if (rc == DM_OK) rc = t.alloc(rmask, (size_t)B * 4);
    if (rc == DM_OK) {
      rc = LAUNCH(h, tg_expand_rows_kernel, dim3((unsigned)std::min<int64_t>((B + 255) / 256, 8192)), dim3(256), 0, d_seq, d_umask, U, n, L, rseq, rmask);
      float lf = 0.f;
      if (rc == DM_OK) rc = train_fb_dev(h, d_codes, rseq, rmask, d_labels, B, L, &lf);      // (synchronises: the loss is read back)
      if (loss) *loss = lf;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == DM_OK) rc = fail(h, DM_ERR_HIP, "train_fb_grouped_dev: kernel failed");
    return rc;
  }
  {
    // touched-row list capacity (see train_fb_dev): at most B candidate rows + U * L history rows are new
    h->touch_ub += (size_t)B + (size_t)U * L;
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
  }
  HIPCHK(h, hipMemsetAsync(h->d_loss, 0, 16, h->stream));
  int rc = dispatch_E(h, h->embed, "unsupported embed size",
                      [&](auto e) { return tg_launch_E<decltype(e)::value>(h, d_seq, d_umask, d_codes, d_labels, U, n, L); });
  if (rc != DM_OK) return rc;
  // rows the gradient reached: the candidates and the users' histories (each history once, not once per row)
  if ((rc = LAUNCH(h, dm_mark_touched_kernel, dim3(256), dim3(256), 0, d_codes, nullptr, B, 0, h->d_touch_bits, h->d_touch_list, h->d_touch_cnt, h->touch_cap, h->num_index)) != DM_OK ||
      (rc = LAUNCH(h, dm_mark_touched_kernel, dim3(64), dim3(256), 0, d_seq, nullptr, U * L, 0, h->d_touch_bits, h->d_touch_list, h->d_touch_cnt, h->touch_cap, h->num_index)) != DM_OK)
    return rc;
  if ((rc = h->train.mark_active(h, 256, d_codes, B, d_seq, U * L)) != DM_OK) return rc;
  if (loss) {
    double acc[2];
    HIPCHK(h, hipMemcpyAsync(acc, h->d_loss, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->last_loss = (acc[0] - acc[1]) / (double)B;         // BCECriterionWithLogits.scala:52-58, sizeAverage
    *loss = (float)h->last_loss;
  }
  return DM_OK;
}

int dm_train_forward_backward_grouped_dev(dm_handle_t h, const int32_t *d_seq_codes, const uint32_t *d_user_mask, const int32_t *d_codes,
                                          const float *d_labels, int64_t U, int rows_per_user, int L, float *loss) {
  if (!h) return DM_ERR_INVALID;
  int rc = train_check(h, "dm_train_forward_backward_grouped_dev");
  if (rc != DM_OK) return rc;
  if (!d_seq_codes || !d_codes || !d_labels || U <= 0 || rows_per_user <= 0 || L <= 0 || L > DM_PIPE_MAXL)
    return fail(h, DM_ERR_INVALID, "dm_train_forward_backward_grouped_dev: bad arguments (L must be 1..32)");
  HIPCHK(h, hipSetDevice(h->device));
  try { return train_fb_grouped_dev(h, d_seq_codes, d_user_mask, d_codes, d_labels, U, rows_per_user, L, loss); }
  catch (const std::exception &e) { return fail(h, DM_ERR_INVALID, std::string("dm_train_forward_backward_grouped_dev: ") + e.what()); }
}
