// The gradient of a TrainVec ([rows x E table | tail]) whose last step left its sorted destination keys in TrainVec::prev, exchanged across
// ranks: rows_sync<T>, LocalOptimizer.syncGradients minus the division for the two models whose step works that way — the DeepFM scorer
// (dfm_train_sync.hip.inc, DESIGN.md §19: T = float) and the Deep-Retrieval layer model (dr_train_sync.hip.inc, §22: float or double).  After
// the call every replica holds, for every table row any rank reached, ((0 + g_0) + g_1) + ... in RANK order (ranks that did not reach the
// row are skipped) and the same rank-ordered sum of the dense tail, on either transport: the sum in T of the ranks' local gradients bit for
// bit, no floating-point atomics, so the replicas stay identical with no parameter broadcast and the table never moves.  The callers
// differ in T, the row width, the row count, the tail length, the record's shape words and the block's padding: a RowsSync says which.
//
// A rank's block:  [ids: n int32, ascending, unique | rows: n x E of T | tail: nd of T].  With RowsSync::align8 the id list is padded to an
// even count (padding id = the row count, which no kernel takes for a row) and the block to a multiple of 8 bytes, so that every rows
// section and every tail of doubles starts 8-byte aligned in the receive buffer whatever the ranks' counts are.
// The blocks' shapes travel ahead of them as one 48-byte record per rank {ok, n, shape[0..4)} through the host all-gather that also sizes
// dm_comm_all_gather_dev: every rank sees every record, so a rank whose pack failed (ok = 0) or that trains another shape fails ALL ranks
// with DM_ERR_STATE before a payload byte moves.
//
// Kernels:
//   rows_sync_heads_kernel  flag[i] = the sorted destination key i of the last batch (TrainVec::prev) is a table row and differs from key i - 1;
//                           dev_select_flagged compacts the flagged keys into the rank's ascending unique row list
//   rows_sync_pack_kernel   the block: ids, the rows gathered from the gradient, a copy of the tail
//   dm_sum_blocks_kernel    (comm.hip.inc) the W tails, copied side by side, added in rank order
//   dm_zero_rows_kernel     (comm.hip.inc) this rank's own rows := 0 (every other row of the table's gradient already is: the next step's
//                           zeroGradParameters and the Adam step see to that)
//   rows_sync_add_rows_kernel  one launch per rank, in rank order: grad[id] += row, and the rank's ids appended to the new `prev` key list.
//                           Rows are unique inside a rank, so a launch is race-free without atomics; ids outside the table are skipped
// Two launch kinds, the caller's, under the caller's switch: pack (heads, compaction, pack) and sum (everything after the exchange).

__global__ void rows_sync_heads_kernel(const unsigned long long *keys, int64_t m, int64_t NR, uint8_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    flag[i] = (key < (unsigned long long)NR && (i == 0 || keys[i - 1] != key)) ? 1 : 0;
  }
}

// block = [n_ids ids (the last n_ids - n: padding, = NR) | n x E rows | nd tail | `trail` zero words]; grad = [NR x E table | nd tail]
template <typename T>
__global__ void rows_sync_pack_kernel(const T *grad, const unsigned long long *uniq, int64_t n, int64_t n_ids, int E, int64_t NR, int64_t nd, int trail, int32_t *block) {
  int32_t *ids = block;
  T *rows = (T *)(block + n_ids), *tail = rows + n * E;
  const T *gtail = grad + NR * E;
  const int64_t nrow = n * E, total = nrow + n_ids + nd + trail;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    if (t < nrow) rows[t] = grad[(int64_t)uniq[t / E] * E + (t % E)];
    else if (t < nrow + n_ids) ids[t - nrow] = t - nrow < n ? (int32_t)uniq[t - nrow] : (int32_t)NR;
    else if (t < nrow + n_ids + nd) tail[t - nrow - n_ids] = gtail[t - nrow - n_ids];
    else ((int32_t *)(tail + nd))[t - nrow - n_ids - nd] = 0;
  }
}

template <typename T>
__global__ void rows_sync_add_rows_kernel(T *grad, const int32_t *ids, const T *rows, int64_t n, int E, int64_t NR, unsigned long long *keys_out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * E; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / E;
    const int e = (int)(t % E);
    const int32_t id = ids[i];
    const bool in = id >= 0 && id < NR;
    if (e == 0) keys_out[i] = in ? (unsigned long long)id : (unsigned long long)NR;      // a padding key to the next step's clear
    if (in) grad[(int64_t)id * E + e] += rows[t];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// what an exchange is made of: the vector, its owner's buffers and flag, the shape, the names its messages and event pairs carry
struct RowsSync {
  const char *who;
  TrainVec *vec;
  DevGrow *ws, *staging;          // the step's workspace (the unique-row scratch) and the grow-only staging of the blocks
  bool *exchanged;
  int64_t NR; int E; int64_t nd;  // table rows, row width, tail length (elements)
  uint64_t shape[4];              // the record's words after {ok, n}: every rank's must equal this rank's
  bool align8;
  int ev_pack, ev_sum; bool detail;
  std::string (*mismatch)(const RowsSync &x, int r, const uint64_t *rec);      // the message for rank r's record (6 words) that differs
};

// heads + compaction on the stream: the rank's unique rows in `uniq` (capacity m), their number in *d_cnt
static int rows_sync_unique_rows(dm_ctx *h, const RowsSync &x, int64_t m, uint8_t *flag, unsigned long long *uniq, unsigned long long *d_cnt, uint32_t *tmp) {
  return timed(h, x.ev_pack, x.detail, [&]() -> int {
    if (m > 0) LAUNCHCHK(h, rows_sync_heads_kernel, dim3(drt_blocks(h, m, 256)), dim3(256), 0, (const unsigned long long *)x.vec->prev.p, m, x.NR, flag);
    const hipError_t e = dev_select_flagged<unsigned long long>(h->stream, (const unsigned long long *)x.vec->prev.p, (const char *)nullptr, flag, uniq, (char *)nullptr, d_cnt, m, tmp);
    return e == hipSuccess ? DM_OK : fail(h, DM_ERR_HIP, std::string(x.who) + ": compaction failed: " + hipGetErrorString(e));
  });
}

// The caller has made its own checks (model, training state); everything from the communicator on happens here.
template <typename T>
static int rows_sync(dm_ctx *h, const RowsSync &x) {
  const char *who = x.who;
  dm_comm *c = h->comm;
  if (!c) return fail(h, DM_ERR_STATE, std::string(who) + ": no communicator attached (dm_comm_attach)");
  if (*x.exchanged)
    return fail(h, DM_ERR_STATE, std::string(who) + ": already exchanged - the gradient holds the sum of all ranks until the next forward/backward or Adam step (a second exchange would sum a sum)");
  const int W = c->nranks;
  dm_sync_stats &S = h->sync_stats;
  S = dm_sync_stats{};
  S.nranks = W; S.transport = c->kind;
  if (W == 1) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  TrainVec &vec = *x.vec;
  const int E = x.E;
  const int64_t NR = x.NR, nd = x.nd, m = vec.prev_m;
  T *grad = (T *)vec.grad;
  const auto ids_of = [&](uint64_t n) { return x.align8 ? (n + 1) & ~(uint64_t)1 : n; };
  const auto bytes_of = [&](uint64_t n) {
    const uint64_t b = 4 * ids_of(n) + sizeof(T) * (n * (uint64_t)E + (uint64_t)nd);
    return x.align8 ? (b + 7) & ~(uint64_t)7 : b;
  };
  int rc;
  // ---- (1) this rank's unique rows and their number: the one host read that sizes the exchange.  A failure up to here is carried into
  // the record exchange (ok = 0): returning at once would leave the peers waiting in it
  DevArena wa(*x.ws, 8);
  const size_t o_flag = wa.add((size_t)m), o_uniq = wa.add((size_t)m * 8), o_cnt = wa.add(8), o_tmp = wa.add(dev_sort_scratch_bytes(m));
  unsigned long long n_mine = 0;
  rc = wa.commit(h);
  const unsigned long long *uniq = wa.ptr<unsigned long long>(o_uniq);
  if (rc == DM_OK) rc = rows_sync_unique_rows(h, x, m, wa.ptr<uint8_t>(o_flag), wa.ptr<unsigned long long>(o_uniq), wa.ptr<unsigned long long>(o_cnt), wa.ptr<uint32_t>(o_tmp));
  if (rc == DM_OK) {
    hipError_t e = hipMemcpyAsync(&n_mine, wa.ptr<unsigned long long>(o_cnt), 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    S.host_syncs++;
    if (e != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string(who) + ": reading the row count failed: " + hipGetErrorString(e));
  }
  // ---- (2) the records: every rank's shape and row count
  const uint64_t rec[6] = {rc == DM_OK ? 1ull : 0ull, n_mine, x.shape[0], x.shape[1], x.shape[2], x.shape[3]};
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
    if (memcmp(v + 2, x.shape, sizeof x.shape) != 0 || v[1] > (uint64_t)NR) return fail(h, DM_ERR_STATE, x.mismatch(x, r, v));
    cnt[r] = v[1];
    bytes[r] = bytes_of(cnt[r]);
    rows_total += cnt[r]; total += bytes[r];
  }
  S.rows_mine = n_mine; S.rows_total = rows_total;
  // ---- (3) staging [W blocks in rank order | W tails side by side], the new key list, this rank's block packed in its place.  A rank
  // that cannot allocate says so before anybody enters the payload exchange
  size_t my_off = 0;
  for (int r = 0; r < c->rank; r++) my_off += bytes[r];
  DevArena sa(*x.staging, 4);
  const size_t o_blocks = sa.add((size_t)total), o_tails = sa.add((size_t)W * nd * sizeof(T));
  rc = sa.commit(h);
  // (a key list that has to grow is allocated here and swapped in after the agreement: a rank that leaves the exchange keeps the keys
  //  its next step has to clear)
  DevGrow keys;
  if (rc == DM_OK && vec.prev.bytes < (size_t)rows_total * 8) rc = keys.reserve(h, (size_t)rows_total * 8, (size_t)rows_total);
  char *blocks = sa.ptr<char>(o_blocks);
  T *tails = sa.ptr<T>(o_tails);
  if (rc == DM_OK)
    rc = timed(h, x.ev_pack, x.detail, [&]() -> int {
      const int64_t n_ids = (int64_t)ids_of(n_mine);
      const int trail = (int)((bytes[c->rank] - 4 * (uint64_t)n_ids - sizeof(T) * (n_mine * (uint64_t)E + (uint64_t)nd)) / 4);
      return LAUNCH(h, rows_sync_pack_kernel<T>, dim3(drt_blocks(h, (int64_t)n_mine * E + n_ids + nd + trail, 256)), dim3(256), 0, grad, uniq, (int64_t)n_mine, n_ids, E, NR, nd,
                    trail, (int32_t *)(blocks + my_off));
    });
  if ((rc = comm_agree(h, c, rc, who)) != DM_OK) { keys.release(); return rc; }
  if (keys.p) {      // cold path: the old keys move over (they stay this rank's list until the rebuild replaces them)
    if (m > 0) HIPCHK(h, hipMemcpyAsync(keys.p, vec.prev.p, (size_t)m * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    S.host_syncs++;
    vec.prev.release();
    vec.prev = keys;
  }
  // ---- (4) ONE var-size all-gather of the blocks, this rank's in place: the payload half of dm_comm_all_gather_dev
  int syncs = 0;
  rc = comm_all_gather_dev_payload(h, c, blocks + my_off, (size_t)bytes[c->rank], blocks, bytes, (size_t)total, &syncs);
  S.host_syncs += syncs;
  if (rc != DM_OK) return rc;
  S.bytes_sent = bytes[c->rank]; S.bytes_recv = total;
  // ---- (5) rebuild: tails in rank order, own rows := 0, every rank's rows in rank order; received rows are marked active (Adam visits
  // them) and `prev` becomes the concatenation of all ranks' rows (the next step's zeroGradParameters clears foreign rows too)
  *x.exchanged = true;      // from the first write on: a failure below leaves a gradient that must not be exchanged again
  rc = timed(h, x.ev_sum, x.detail, [&]() -> int {
    size_t off = 0;
    for (int r = 0; r < W; r++) {
      const hipError_t e = hipMemcpyAsync(tails + (int64_t)r * nd, blocks + off + 4 * (size_t)ids_of(cnt[r]) + sizeof(T) * (size_t)(cnt[r] * E), (size_t)nd * sizeof(T),
                                          hipMemcpyDeviceToDevice, h->stream);
      if (e != hipSuccess) return fail(h, DM_ERR_HIP, std::string(who) + ": tail copy failed: " + hipGetErrorString(e));
      off += bytes[r];
    }
    LAUNCHCHK(h, dm_sum_blocks_kernel<T>, dim3(std::max(64u, drt_blocks(h, nd, 256))), dim3(256), 0, grad + NR * E, (const T *)tails, nd, W);
    const int32_t *my_ids = (const int32_t *)(blocks + my_off);
    if (n_mine) LAUNCHCHK(h, dm_zero_rows_kernel<T>, dim3(drt_blocks(h, (int64_t)n_mine * E, 256)), dim3(256), 0, grad, my_ids, (int64_t)n_mine, E);
    off = 0;
    uint64_t ro = 0;
    for (int r = 0; r < W; r++) {
      if (cnt[r]) {
        const int32_t *ids = (const int32_t *)(blocks + off);
        const int64_t n = (int64_t)cnt[r];
        LAUNCHCHK(h, rows_sync_add_rows_kernel<T>, dim3(drt_blocks(h, n * E, 256)), dim3(256), 0, grad, ids, (const T *)(ids + ids_of(cnt[r])), n, E, NR,
                  (unsigned long long *)vec.prev.p + ro);
        if (r != c->rank) { const int rc_m = vec.mark_active(h, drt_blocks(h, n, 256), ids, n); if (rc_m != DM_OK) return rc_m; }
      }
      off += bytes[r]; ro += cnt[r];
    }
    return DM_OK;
  });
  vec.prev_m = (int64_t)rows_total;
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.host_syncs++;
  return DM_OK;
}
