// DeepFM training, data-parallel: LocalOptimizer.syncGradients (tdm/src/main/scala/com/mass/tdm/optim/LocalOptimizer.scala:164-187) minus the
// division, which dm_deepfm_adam_step(1 / N) folds in — dm_deepfm_train_sync_gradients (DESIGN.md §19).  One worker per rank ran one of the
// three steps (row, grouped, CSR) on its slice; afterwards every replica holds, for every table row any rank reached,
// ((0 + g_0) + g_1) + ... in RANK order (ranks that did not reach the row are skipped) and the same rank-ordered sum of the dense tail
// [l1.W ; l1.b ; l2.W ; l2.b], on either transport: the fp32 sum of the ranks' local gradients bit for bit, so the replicas stay identical
// with no parameter broadcast and the table never moves.  fp32 only, as the step.
//
// A rank's block, 4-byte words:  [ids: n int32, ascending, unique | rows: n x Ep float | tail: nd float],  nd = T T Ep + 2 T + 1.
// The blocks' shapes travel ahead of them as one 48-byte record per rank {ok, n, NI, Ep, T, 0} through the host all-gather that also
// sizes dm_comm_all_gather_dev: every rank sees every record, so a rank whose pack failed (ok = 0) or that trains another shape fails ALL
// ranks with DM_ERR_STATE before a payload byte moves.
//
// Kernels:
//   dfm_sync_heads_kernel   flag[i] = the sorted destination key i of the last batch (TrainVec::prev) is a table row and differs from key i - 1;
//                           dev_select_flagged compacts the flagged keys into the rank's ascending unique row list
//   dfm_sync_pack_kernel    the block: ids, the rows gathered from the gradient, a copy of the tail
//   dm_sum_blocks_kernel    (comm.hip.inc) the W tails, copied side by side, added in rank order
//   dm_zero_rows_kernel     (comm.hip.inc) this rank's own rows := 0 (every other row of the table's gradient already is: the next step's
//                           zeroGradParameters and the Adam step see to that)
//   dfm_sync_add_rows_kernel  one launch per rank, in rank order: grad[id] += row, and the rank's ids appended to the new `prev` key list.
//                           Rows are unique inside a rank, so a launch is race-free without atomics; ids outside the table are skipped
// Launch kinds under DM_DFM_TIME_LAUNCHES=1: EV_DFT_SYNC_PACK (heads, compaction, pack), EV_DFT_SYNC_SUM (everything after the exchange).

__global__ void dfm_sync_heads_kernel(const unsigned long long *keys, int64_t m, int64_t NI, uint8_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    flag[i] = (key < (unsigned long long)NI && (i == 0 || keys[i - 1] != key)) ? 1 : 0;
  }
}

// block = [n ids | n x Ep rows | nd tail]; grad = [NI x Ep table | nd tail]
__global__ void dfm_sync_pack_kernel(const float *grad, const unsigned long long *uniq, int64_t n, int Ep, int64_t NI, int64_t nd, int32_t *block) {
  int32_t *ids = block;
  float *rows = (float *)(block + n), *tail = rows + n * Ep;
  const float *gtail = grad + NI * Ep;
  const int64_t nrow = n * Ep, total = n + nrow + nd;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    if (t < nrow) rows[t] = grad[(int64_t)uniq[t / Ep] * Ep + (t % Ep)];
    else if (t < nrow + n) ids[t - nrow] = (int32_t)uniq[t - nrow];
    else tail[t - nrow - n] = gtail[t - nrow - n];
  }
}

__global__ void dfm_sync_add_rows_kernel(float *grad, const int32_t *ids, const float *rows, int64_t n, int Ep, int64_t NI, unsigned long long *keys_out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * Ep; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / Ep;
    const int e = (int)(t % Ep);
    const int32_t id = ids[i];
    const bool in = id >= 0 && id < NI;
    if (e == 0) keys_out[i] = in ? (unsigned long long)id : (unsigned long long)NI;      // a padding key to the next step's clear
    if (in) grad[(int64_t)id * Ep + e] += rows[t];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// heads + compaction on the stream: the rank's unique rows in `uniq` (capacity m), their number in *d_cnt
static int dfm_sync_unique_rows(dm_ctx *h, dm_dfm_train *t, int64_t m, uint8_t *flag, unsigned long long *uniq, unsigned long long *d_cnt, uint32_t *tmp, bool detail) {
  return timed(h, EV_DFT_SYNC_PACK, detail, [&]() -> int {
    if (m > 0) LAUNCHCHK(h, dfm_sync_heads_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, (const unsigned long long *)t->vec.prev.p, m, h->num_index, flag);
    const hipError_t e = dev_select_flagged<unsigned long long>(h->stream, (const unsigned long long *)t->vec.prev.p, (const char *)nullptr, flag, uniq, (char *)nullptr, d_cnt, m, tmp);
    return e == hipSuccess ? DM_OK : fail(h, DM_ERR_HIP, std::string("dm_deepfm_train_sync_gradients: compaction failed: ") + hipGetErrorString(e));
  });
}

int dm_deepfm_train_sync_gradients(dm_handle_t h) {
  static const char *who = "dm_deepfm_train_sync_gradients";
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_sync_gradients");
  int rc = dfm_train_check(h, who, true);
  if (rc != DM_OK) return rc;
  dm_comm *c = h->comm;
  if (!c) return fail(h, DM_ERR_STATE, std::string(who) + ": no communicator attached (dm_comm_attach)");
  dm_dfm_train *t = h->dfm_tr;
  if (t->exchanged)
    return fail(h, DM_ERR_STATE, std::string(who) + ": already exchanged - the gradient holds the sum of all ranks until the next forward/backward or Adam step (a second exchange would sum a sum)");
  const int W = c->nranks;
  dm_sync_stats &S = h->sync_stats;
  S = dm_sync_stats{};
  S.nranks = W; S.transport = c->kind;
  if (W == 1) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const bool detail = dfm_time_launches();
  const int Ep = h->embed, T = h->dfm_L + 1;
  const int64_t NI = h->num_index, nd = (int64_t)T * T * Ep + 2 * T + 1, m = t->vec.prev_m;
  float *grad = (float *)t->vec.grad;
  // ---- (1) this rank's unique rows and their number: the one host read that sizes the exchange.  A failure up to here is carried into
  // the record exchange (ok = 0): returning at once would leave the peers waiting in it
  DevArena wa(t->ws, 8);
  const size_t o_flag = wa.add((size_t)m), o_uniq = wa.add((size_t)m * 8), o_cnt = wa.add(8), o_tmp = wa.add(dev_sort_scratch_bytes(m));
  unsigned long long n_mine = 0;
  rc = wa.commit(h);
  const unsigned long long *uniq = wa.ptr<unsigned long long>(o_uniq);
  if (rc == DM_OK) rc = dfm_sync_unique_rows(h, t, m, wa.ptr<uint8_t>(o_flag), wa.ptr<unsigned long long>(o_uniq), wa.ptr<unsigned long long>(o_cnt), wa.ptr<uint32_t>(o_tmp), detail);
  if (rc == DM_OK) {
    hipError_t e = hipMemcpyAsync(&n_mine, wa.ptr<unsigned long long>(o_cnt), 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    S.host_syncs++;
    if (e != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string(who) + ": reading the row count failed: " + hipGetErrorString(e));
  }
  // ---- (2) the records: every rank's shape and row count
  const uint64_t rec[6] = {rc == DM_OK ? 1ull : 0ull, n_mine, (uint64_t)NI, (uint64_t)Ep, (uint64_t)T, 0};
  std::vector<char> rbuf; std::vector<uint64_t> rsz;
  const int rc_r = comm_all_gather_v_host(c, rec, sizeof rec, rbuf, rsz);
  if (rc != DM_OK) return rc;
  if (rc_r != DM_OK) return fail(h, rc_r, c->err);
  std::vector<uint64_t> cnt(W), bytes(W);
  uint64_t rows_total = 0, total = 0;
  for (int r = 0; r < W; r++) {
    uint64_t v[6];
    if (rsz[r] != sizeof rec) return fail(h, DM_ERR_STATE, std::string(who) + ": peers disagree on the record size (rank " + std::to_string(r) + ")");
    memcpy(v, rbuf.data() + sizeof rec * (size_t)r, sizeof rec);
    if (!v[0]) return fail(h, DM_ERR_STATE, std::string(who) + ": rank " + std::to_string(r) + " failed before the exchange; every rank leaves it");
    if (v[2] != (uint64_t)NI || v[3] != (uint64_t)Ep || v[4] != (uint64_t)T || v[1] > (uint64_t)NI) {
      char msg[320];
      snprintf(msg, sizeof msg, "%s: rank %d trains another shape (num_index %llu, padded embed %llu, seq_len + 1 = %llu, %llu rows; here %lld, %d, %d): every rank fails the exchange",
               who, r, (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4], (unsigned long long)v[1], (long long)NI, Ep, T);
      return fail(h, DM_ERR_STATE, msg);
    }
    cnt[r] = v[1];
    bytes[r] = 4 * (cnt[r] + cnt[r] * (uint64_t)Ep + (uint64_t)nd);
    rows_total += cnt[r]; total += bytes[r];
  }
  S.rows_mine = n_mine; S.rows_total = rows_total;
  // ---- (3) staging [W blocks in rank order | W tails side by side], the new key list, this rank's block packed in its place.  A rank
  // that cannot allocate says so before anybody enters the payload exchange
  size_t my_off = 0;
  for (int r = 0; r < c->rank; r++) my_off += bytes[r];
  DevArena sa(t->sync, 4);
  const size_t o_blocks = sa.add((size_t)total), o_tails = sa.add((size_t)W * nd * 4);
  rc = sa.commit(h);
  // (a key list that has to grow is allocated here and swapped in after the agreement: a rank that leaves the exchange keeps the keys
  //  its next step has to clear)
  DevGrow keys;
  if (rc == DM_OK && t->vec.prev.bytes < (size_t)rows_total * 8) rc = keys.reserve(h, (size_t)rows_total * 8, (size_t)rows_total);
  char *blocks = sa.ptr<char>(o_blocks);
  float *tails = sa.ptr<float>(o_tails);
  if (rc == DM_OK)
    rc = timed(h, EV_DFT_SYNC_PACK, detail, [&]() -> int {
      return LAUNCH(h, dfm_sync_pack_kernel, dim3(drt_blocks(h, (int64_t)(bytes[c->rank] / 4), 256)), dim3(256), 0, grad, uniq, (int64_t)n_mine, Ep, NI, nd, (int32_t *)(blocks + my_off));
    });
  if ((rc = comm_agree(h, c, rc, who)) != DM_OK) { keys.release(); return rc; }
  if (keys.p) {      // cold path: the old keys move over (they stay this rank's list until the rebuild replaces them)
    if (m > 0) HIPCHK(h, hipMemcpyAsync(keys.p, t->vec.prev.p, (size_t)m * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    S.host_syncs++;
    t->vec.prev.release();
    t->vec.prev = keys;
  }
  // ---- (4) ONE var-size all-gather of the blocks, this rank's in place: the payload half of dm_comm_all_gather_dev
  int syncs = 0;
  rc = comm_all_gather_dev_payload(h, c, blocks + my_off, (size_t)bytes[c->rank], blocks, bytes, (size_t)total, &syncs);
  S.host_syncs += syncs;
  if (rc != DM_OK) return rc;
  S.bytes_sent = bytes[c->rank]; S.bytes_recv = total;
  // ---- (5) rebuild: tails in rank order, own rows := 0, every rank's rows in rank order; received rows are marked active (Adam visits
  // them) and `prev` becomes the concatenation of all ranks' rows (the next step's zeroGradParameters clears foreign rows too)
  t->exchanged = true;      // from the first write on: a failure below leaves a gradient that must not be exchanged again
  rc = timed(h, EV_DFT_SYNC_SUM, detail, [&]() -> int {
    size_t off = 0;
    for (int r = 0; r < W; r++) {
      const hipError_t e = hipMemcpyAsync(tails + (int64_t)r * nd, blocks + off + 4 * (size_t)(cnt[r] + cnt[r] * Ep), (size_t)nd * 4, hipMemcpyDeviceToDevice, h->stream);
      if (e != hipSuccess) return fail(h, DM_ERR_HIP, std::string(who) + ": tail copy failed: " + hipGetErrorString(e));
      off += bytes[r];
    }
    LAUNCHCHK(h, dm_sum_blocks_kernel<float>, dim3(64), dim3(256), 0, grad + NI * Ep, (const float *)tails, nd, W);
    const int32_t *my_ids = (const int32_t *)(blocks + my_off);
    if (n_mine) LAUNCHCHK(h, dm_zero_rows_kernel<float>, dim3(drt_blocks(h, (int64_t)n_mine * Ep, 256)), dim3(256), 0, grad, my_ids, (int64_t)n_mine, Ep);
    off = 0;
    uint64_t ro = 0;
    for (int r = 0; r < W; r++) {
      if (cnt[r]) {
        const int32_t *ids = (const int32_t *)(blocks + off);
        const int64_t n = (int64_t)cnt[r];
        LAUNCHCHK(h, dfm_sync_add_rows_kernel, dim3(drt_blocks(h, n * Ep, 256)), dim3(256), 0, grad, ids, (const float *)(ids + n), n, Ep, NI, (unsigned long long *)t->vec.prev.p + ro);
        if (r != c->rank) { const int rc_m = t->vec.mark_active(h, drt_blocks(h, n, 256), ids, n); if (rc_m != DM_OK) return rc_m; }
      }
      off += bytes[r]; ro += cnt[r];
    }
    return DM_OK;
  });
  t->vec.prev_m = (int64_t)rows_total;
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.host_syncs++;
  return DM_OK;
}
