// DeepFM training, data-parallel: LocalOptimizer.syncGradients (tdm/src/main/scala/com/mass/tdm/optim/LocalOptimizer.scala:164-187) minus the
// division, which dm_deepfm_adam_step(1 / N) folds in — dm_deepfm_train_sync_gradients (DESIGN.md §19).  One worker per rank ran one of the
// three steps (row, grouped, CSR) on its slice; afterwards every replica holds the rank-ordered fp32 sum of the ranks' table rows and of
// the dense tail [l1.W ; l1.b ; l2.W ; l2.b].  fp32 only, as the step.
//
// The pipeline, its kernels and the block layout are rows_sync<float> (rows_sync.hip.inc), here with
//   rows    num_index rows of Ep (the padded embed size) values
//   tail    nd = T T Ep + 2 T + 1 values, T = seq_len + 1
//   record  {ok, n, NI, Ep, T, 0}
//   block   4-byte words throughout, unpadded
// Launch kinds under DM_DFM_TIME_LAUNCHES=1: EV_DFT_SYNC_PACK (heads, compaction, pack), EV_DFT_SYNC_SUM (everything after the exchange).

static std::string dfm_sync_mismatch(const RowsSync &x, int r, const uint64_t *v) {
  char msg[320];
  snprintf(msg, sizeof msg, "%s: rank %d trains another shape (num_index %llu, padded embed %llu, seq_len + 1 = %llu, %llu rows; here %lld, %d, %d): every rank fails the exchange",
           x.who, r, (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4], (unsigned long long)v[1], (long long)x.NR, x.E, (int)x.shape[2]);
  return msg;
}

int dm_deepfm_train_sync_gradients(dm_handle_t h) {
  static const char *who = "dm_deepfm_train_sync_gradients";
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_train_sync_gradients");
  int rc = dfm_train_check(h, who, true);
  if (rc != DM_OK) return rc;
  dm_dfm_train *t = h->dfm_tr;
  const int Ep = h->embed, T = h->dfm_L + 1;
  RowsSync x{};
  x.who = who; x.vec = &t->vec; x.ws = &t->ws; x.staging = &t->sync; x.exchanged = &t->exchanged;
  x.NR = h->num_index; x.E = Ep; x.nd = (int64_t)T * T * Ep + 2 * T + 1;
  x.shape[0] = (uint64_t)h->num_index; x.shape[1] = (uint64_t)Ep; x.shape[2] = (uint64_t)T; x.shape[3] = 0;
  x.align8 = false;
  x.ev_pack = EV_DFT_SYNC_PACK; x.ev_sum = EV_DFT_SYNC_SUM; x.detail = dfm_time_launches();
  x.mismatch = dfm_sync_mismatch;
  return rows_sync<float>(h, x);
}
