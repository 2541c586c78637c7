// The optimizer state of ONE trained parameter vector and its Adam step: the DIN compact vector (dm_ctx::train), the Deep-Retrieval
// layer model (dm_dr_train), the rerank graph and the rerank criterion (dm_dr_rr_train).  A vector is `rows` table rows of E values
// followed by a tail of n - rows E values; the weights themselves belong to the model and are an argument of the step.
// The state has to precede dm_ctx (it is a member) and its methods need dm_ctx, so dm_hip.hip includes this file once per part and
// names the part: DM_ADAM_VEC_PART 1 = struct TrainVec, 2 = its methods and the step.
#if DM_ADAM_VEC_PART == 1

struct AdamPlan { double step; int64_t act; bool rows_path; };      // one step, decided: TrainVec::plan_step

struct TrainVec {
  int64_t rows = 0, n = 0;
  int E = 0;
  void *grad = nullptr, *s = nullptr, *r = nullptr;      // [n] in the model's type: gradient and the two moments
  unsigned *active_bits = nullptr;                       // table rows a gradient has ever reached since init (what the step has to visit)
  int32_t *active_list = nullptr;
  unsigned long long *active_cnt = nullptr;
  dm_adam_opts opts{};
  int t = 0;
  DevGrow prev;                                          // the sorted destination rows of the last batch (zeroed by the next); DIN: unused.
                                                         // After a gradient exchange (rows_sync): every rank's unique rows, rank after rank (a
                                                         // union with repeats, sorted only inside a rank) - enough for drt_seg_rows_kernel<T, true>,
                                                         // which clears at every change of key, and clearing a row twice changes nothing
  int64_t prev_m = 0;

  int init(dm_ctx *h, int64_t rows_, int E_, int64_t n_, size_t elem_size, const dm_adam_opts &o);
  void release() { dm_release(grad, s, r, active_bits, active_list, active_cnt); prev.release(); prev_m = 0; t = 0; }
  const void *buffer(int what) const { return what == 1 ? grad : what == 2 ? s : r; }      // the download entry points' 1..3
  int mark_active(dm_ctx *h, unsigned grid, const int32_t *a, int64_t na, const int32_t *b = nullptr, int64_t nb = 0);
  int remember(dm_ctx *h, const unsigned long long *sorted_keys, int64_t m);
  void forget() { prev_m = 0; }
  AdamPlan plan_step(unsigned long long active);
};

#elif DM_ADAM_VEC_PART == 2

// All buffers zeroed on the handle's stream (the caller synchronises if it has to).  A failure releases everything: a handle that is
// not training, not one that trains on null buffers.
int TrainVec::init(dm_ctx *h, int64_t rows_, int E_, int64_t n_, size_t elem_size, const dm_adam_opts &o) {
  release();
  const size_t nb = (size_t)n_ * elem_size, words = (size_t)((rows_ + 31) / 32 + 1) * 4;
  int rc = DM_OK;
  for (void **p : {&grad, &s, &r})
    if (rc == DM_OK) rc = dm_alloc(h, p, nb);
  if (rc == DM_OK) rc = dm_alloc(h, (void **)&active_bits, words);
  if (rc == DM_OK) rc = dm_alloc(h, (void **)&active_list, (size_t)rows_ * 4);
  if (rc == DM_OK) rc = dm_alloc(h, (void **)&active_cnt, 8);
  hipError_t e = hipSuccess;
  for (void *p : {grad, s, r})
    if (rc == DM_OK && e == hipSuccess) e = hipMemsetAsync(p, 0, nb, h->stream);
  if (rc == DM_OK && e == hipSuccess) e = hipMemsetAsync(active_bits, 0, words, h->stream);
  if (rc == DM_OK && e == hipSuccess) e = hipMemsetAsync(active_cnt, 0, 8, h->stream);
  if (rc == DM_OK && e != hipSuccess) rc = fail(h, DM_ERR_HIP, std::string("training state: hipMemsetAsync failed: ") + hipGetErrorString(e));
  if (rc != DM_OK) { release(); return rc; }
  rows = rows_; E = E_; n = n_; opts = o; t = 0; prev_m = 0;
  return DM_OK;
}

// rows that have ever received a gradient (the Adam step visits these and the tail only: dm_adam_rows_kernel)
__global__ void dm_mark_active_kernel(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, unsigned *bits, int32_t *list,
                                      unsigned long long *cnt, int64_t num_index) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < na + nb; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t idx = t < na ? a[t] : b[t - na];
    if (idx < 0 || idx >= num_index) continue;
    const unsigned bit = 1u << (idx & 31);
    if (bits[idx >> 5] & bit) continue;
    const unsigned old = atomicOr(bits + (idx >> 5), bit);
    if (!(old & bit)) list[atomicAdd(cnt, 1ull)] = idx;        // at most num_index entries: the list has that capacity
  }
}
int TrainVec::mark_active(dm_ctx *h, unsigned grid, const int32_t *a, int64_t na, const int32_t *b, int64_t nb) {
  return LAUNCH(h, dm_mark_active_kernel, dim3(grid), dim3(256), 0, a, na, b, nb, active_bits, active_list, active_cnt, rows);
}

int TrainVec::remember(dm_ctx *h, const unsigned long long *sorted_keys, int64_t m) {
  const int rc = prev.reserve(h, (size_t)m * 8, (size_t)m);
  if (rc != DM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(prev.p, sorted_keys, (size_t)m * 8, hipMemcpyDeviceToDevice, h->stream));
  prev_m = m;
  return DM_OK;
}

// The next step's size (Adam.scala:19-73: decayed rate, both bias corrections) and its path, given the active count the caller read.
// Rows no gradient has ever reached keep g = s = r = 0 and the dense update leaves their weights bit-identical (see
// dm_adam_rows_kernel): visit the active rows and the tail only, unless eps == 0 or a quarter of the table is active anyway.
// DM_ADAM_DENSE=1 forces the dense stream (tests compare the two).
AdamPlan TrainVec::plan_step(unsigned long long active) {
  const double clr = opts.lr / (1 + t * opts.lr_decay);
  t += 1;
  const double bc1 = 1 - pow(opts.beta1, t), bc2 = 1 - pow(opts.beta2, t);
  const bool force_dense = env_on("DM_ADAM_DENSE");
  return AdamPlan{clr * sqrt(bc2) / bc1, (int64_t)active, !force_dense && opts.eps > 0 && (int64_t)active * 4 < rows};
}

// The launches of one planned step.  Rows path: the listed rows, then the tail — dense, or one value per table row (the criterion's
// softmax_b: tail_by_row, the same list with E = 1).  KEEP puts the gradient back (the accumulating criterion never clears it).
template <typename T, bool KEEP>
static int adam_step_vec(dm_ctx *h, const TrainVec &v, const AdamPlan &p, void *weights, float grad_scale, bool tail_by_row, unsigned tail_grid) {
  const dm_adam_opts &o = v.opts;
  const T gs = (T)grad_scale, b1 = (T)o.beta1, c1 = (T)(1 - o.beta1), b2 = (T)o.beta2, c2 = (T)(1 - o.beta2), eps = (T)o.eps, ns = (T)(-p.step);
  T *w = (T *)weights, *g = (T *)v.grad, *s_ = (T *)v.s, *r_ = (T *)v.r;
  const int64_t table = v.rows * v.E;
  if (!p.rows_path) return LAUNCH(h, (dm_adam_kernel<T, KEEP>), dim3(8192), dim3(256), 0, w, g, s_, r_, v.n, gs, b1, c1, b2, c2, eps, ns);
  int rc = DM_OK;
  if (p.act) rc = LAUNCH(h, (dm_adam_rows_kernel<T, KEEP>), dim3(4096), dim3(256), 0, w, g, s_, r_, v.active_list, p.act, v.E, gs, b1, c1, b2, c2, eps, ns);
  if (rc != DM_OK) return rc;
  if (!tail_by_row)
    return LAUNCH(h, (dm_adam_kernel<T, KEEP>), dim3(tail_grid), dim3(256), 0, w + table, g + table, s_ + table, r_ + table, v.n - table, gs, b1, c1, b2, c2, eps, ns);
  if (p.act)
    return LAUNCH(h, (dm_adam_rows_kernel<T, KEEP>), dim3(tail_grid), dim3(256), 0, w + table, g + table, s_ + table, r_ + table, v.active_list, p.act, 1, gs, b1, c1, b2, c2,
                  eps, ns);
  return DM_OK;
}
static int adam_step(dm_ctx *h, const TrainVec &v, const AdamPlan &p, void *weights, bool f64, bool keep, float grad_scale, bool tail_by_row, unsigned tail_grid) {
  if (f64) return keep ? adam_step_vec<double, true>(h, v, p, weights, grad_scale, tail_by_row, tail_grid) : adam_step_vec<double, false>(h, v, p, weights, grad_scale, tail_by_row, tail_grid);
  return keep ? adam_step_vec<float, true>(h, v, p, weights, grad_scale, tail_by_row, tail_grid) : adam_step_vec<float, false>(h, v, p, weights, grad_scale, tail_by_row, tail_grid);
}

#else
#error "define DM_ADAM_VEC_PART as 1 or 2 before including adam_vec.hip.inc"
#endif
#undef DM_ADAM_VEC_PART
