// Deep-Retrieval layer model, data-parallel: LocalOptimizer.syncGradients (deep-retrieval/src/main/scala/com/mass/dr/optim/LocalOptimizer.scala:
// 167-194) minus the division, which dm_dr_adam_step(1 / P) folds in — dm_dr_train_sync_gradients (DESIGN.md §22).  Every rank ran
// dm_dr_train_forward_backward on its slice of the mini-batch (or nothing: an idle rank); afterwards every replica holds, for every
// embedding row any rank reached, ((0 + g_0) + g_1) + ... in RANK order in the model's dtype (ranks that did not reach the row are
// skipped), and the same rank-ordered sum of the dense tail [W_0 ; b_0 ; ... ; W_{D-1} ; b_{D-1}], on either transport.
//
// The pipeline, its kernels and the block layout are rows_sync<T> (rows_sync.hip.inc), here with
//   T       float or double, the model's
//   rows    NR = num_item + K (D - 1): the item rows and the node rows (which every rank reaches on every batch)
//   tail    nd = n_par - NR E = sum_d (K (L + d) E + K) values — the bulk of the block at the shipped shapes
//   record  {ok, n, NR, E, n_par, dtype}
//   block   align8: ids padded to an even count with NR, the block a multiple of 8 bytes (doubles stay 8-byte aligned in the receive buffer)
// A rank that ran no step since dm_dr_train_init or its last Adam step sends no rows and a zero tail: TrainVec::init clears the whole
// gradient, the Adam step (dm_adam_kernel / dm_adam_rows_kernel without KEEP) zeroes every element it visits, and it always visits the tail.
// Launch kinds under DM_DR_TIME_LAUNCHES=1: EV_DRT_SYNC_PACK (heads, compaction, pack), EV_DRT_SYNC_SUM (everything after the exchange).

static std::string dr_sync_mismatch(const RowsSync &x, int r, const uint64_t *v) {
  char msg[360];
  snprintf(msg, sizeof msg, "%s: rank %d trains another shape (%llu embedding rows of %llu, %llu parameters, %s, %llu rows sent; here %lld rows of %d, %llu parameters, %s): every rank fails the exchange",
           x.who, r, (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4], v[5] == (uint64_t)DM_F64 ? "fp64" : "fp32", (unsigned long long)v[1],
           (long long)x.NR, x.E, (unsigned long long)x.shape[2], x.shape[3] == (uint64_t)DM_F64 ? "fp64" : "fp32");
  return msg;
}

int dm_dr_train_sync_gradients(dm_handle_t h) {
  static const char *who = "dm_dr_train_sync_gradients";
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_dr_train_sync_gradients");
  int rc = dr_train_check(h, who, true);
  if (rc != DM_OK) return rc;
  dm_dr_state *s = h->dr;
  dm_dr_train *t = s->tr;
  RowsSync x{};
  x.who = who; x.vec = &t->vec; x.ws = &t->ws; x.staging = &t->sync; x.exchanged = &t->exchanged;
  x.NR = s->num_item + (int64_t)s->K * (s->D - 1); x.E = s->E; x.nd = s->n_par - x.NR * s->E;
  x.shape[0] = (uint64_t)x.NR; x.shape[1] = (uint64_t)s->E; x.shape[2] = (uint64_t)s->n_par; x.shape[3] = (uint64_t)s->dtype;
  x.align8 = true;
  x.ev_pack = EV_DRT_SYNC_PACK; x.ev_sum = EV_DRT_SYNC_SUM; x.detail = dr_time_launches();
  x.mismatch = dr_sync_mismatch;
  return s->dtype == DM_F64 ? rows_sync<double>(h, x) : rows_sync<float>(h, x);
}
