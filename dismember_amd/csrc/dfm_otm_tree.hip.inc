// OTM tree construction with a DeepFM model: the child weights of TreeConstruction.aggregateWeights (otm/.../tree/TreeConstruction.scala:
// 194-232, useMask = false: Table(nodes, seq) is the DeepFM graph's input) on the device.  fp32 model, double sums, no atomics.
// The DIN twin (dm_otm_child_weights, jtm_host.hip.inc) expands every (row, chain node) pair on the host; here nothing is expanded:
//   per history, once per construction (dfm_jtm_rows_kernel, dfm_jtm.hip.inc):  s, c, a = W1s vec(K) + l1.b      -> S [R][E], aux [R][NCT 16]
//   per (item, 16 chain nodes), once (dfm_otm_tree_score_kernel):                W1a e by MFMA, kept in the accumulator registers
//   per (row, chain node):                                                       e.s (VALU), sum_t w2[t] relu(acc[t] + a[t]) + c, one double add
// Chain order is the DIN twin's: depth d = 1 .. gap, left to right; the node at (d, c) has code (item_node << d) + (1 << d) - 1 + c and chain
// index x = (1 << d) - 2 + c; nchain = (2 << gap) - 2 nodes in ceil(nchain / 16) tiles.  Chain slots at or past nchain are neither gathered nor
// summed.
//
// One wave takes a unit = (segment of an item's rows, chain tile).  The per-pair logit is dfm_jtm_pairs_kernel's byte for byte: the product
// starts from zero and depends on the chain node only, so keeping it over the rows changes no bit, and e.s and the epilogue below restate
// that kernel's orders (tests/test_gpu_deepfm_otm_tree.py holds the weights to the sums of dm_deepfm_pairs_forward's logits):
//   W1a[t].e    v_mfma_f32_16x16x4_f32 over k = 0 .. E-1 in steps of 4
//   e.s         fma chain over the lane's features in (jc, t) order, then xor 16, xor 32
//   logit       per column w2 relu(. + a) (column 0: c), column tiles added in order, the xor tree over the 16 lanes that hold a pair's
//               columns, + e.s last
// Summation order of the weights (fixed):
//   segment     an item's rows are cut into segments of DFM_OTM_TREE_SEG rows (the last one shorter); within a segment the logits of a
//               chain node are added left to right in double, from 0.0, by the wave that owns the unit
//   score[x]    the item's segment sums added left to right in double, from 0.0 (dfm_otm_tree_sum_kernel); with no more rows than a segment
//               this is the DIN twin's strict row order
//   weight[c]   sum over d = gap .. 1 of score[(1 << d) - 2 + idx], idx = c, idx >>= 1 per step, in double, no contraction
// The segments exist so that an item with 10^5 rows is not one wave's serial loop.  Nothing depends on the grid, on the slice of histories
// a one-shot call sets up at a time, or on which other items a call holds.

#define DFM_OTM_TREE_SEG 256
// DM_DFM_OTM_TREE_SEG=<1 .. 256>: rows per segment, read per call like DM_JTM_MAX_PAIRS (tests: segment edges at sizes a test can afford);
// unset or invalid: DFM_OTM_TREE_SEG
static int dfm_otm_tree_seg() {
  const char *e = env_str("DM_DFM_OTM_TREE_SEG");
  if (!e || !*e) return DFM_OTM_TREE_SEG;
  char *end = nullptr;
  const long long v = strtoll(e, &end, 10);
  return (*end == 0 && v >= 1 && v <= DFM_OTM_TREE_SEG) ? (int)v : DFM_OTM_TREE_SEG;
}

struct DfmOtmSeg { int64_t row0; int32_t item, nrows; };      // rows [row0, row0 + nrows) of the call's histories belong to `item`

struct DfmOtmTreeScore {
  const float *emb;
  const f32x4 *frag;                   // [NCT][E / 16][64] (d_dfm_frag: column 0 zero, columns 1 .. T = W1a)
  const float *w2p;                    // [NCT * 16]
  const float *S, *aux;                // [rows][E], [rows][NCT * 16]: row 0 here is row `row_base` of the segments' numbering
  const int32_t *item_node;            // [items]
  const DfmOtmSeg *segs;               // the launch's segments
  double *part;                        // [segments][nchain]
  int64_t n_units, row_base, num_index;
  int gap;
};

template <int E, int NCT>
__global__ __launch_bounds__(256) void dfm_otm_tree_score_kernel(DfmOtmTreeScore p) {
  constexpr int NJ = E / 16, NC = NCT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem_dot[];
  f32x4 *wl = (f32x4 *)smem_dot;
  dfm_stage_frag<E, NCT>(p.frag, wl, nullptr, nullptr, 256);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int nchain = (2 << p.gap) - 2, ntiles = (nchain + 15) / 16;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < p.n_units; u += (int64_t)gridDim.x * 4) {
    const int64_t sg = u / ntiles;
    const int tile = (int)(u - sg * ntiles);
    const DfmOtmSeg seg = p.segs[sg];
    const int x = 16 * tile + r;
    int32_t code = -1;                   // chain slots at or past nchain are neither gathered nor summed
    if (x < nchain) {
      const int d = 31 - __clz(x + 2);
      code = (int32_t)(((int64_t)p.item_node[seg.item] << d) + (1 << d) - 1 + (x - ((1 << d) - 2)));
    }
    f32x4 qa[NJ], acc[NCT];
    dfm_tile_gather<E>(p.emb, code, p.num_index, g, qa);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {   // W1a e of the 16 chain nodes: once per unit
      acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
        const f32x4 b = wl[(ct * NJ + jc) * 64 + lane];
#pragma unroll
        for (int t = 0; t < 4; t++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[jc][t], b[t], acc[ct], 0, 0, 0);
      }
    }
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    const float *Sr = p.S + (seg.row0 - p.row_base) * E + 4 * g, *ar = p.aux + (seg.row0 - p.row_base) * NC + r;
    // the next row's S and aux are in flight while this row is scored (a segment is one wave's serial loop: its rows' latencies must overlap)
    f32x4 sv[NJ], sn[NJ];
    float av[NCT], an[NCT];
#pragma unroll
    for (int jc = 0; jc < NJ; jc++) sn[jc] = *(const f32x4 *)(Sr + 16 * jc);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) an[ct] = ar[16 * ct];
    for (int n = 0; n < seg.nrows; n++) {
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) sv[jc] = sn[jc];
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) av[ct] = an[ct];
      if (n + 1 < seg.nrows) {             // (rows past the segment are not read)
        Sr += E; ar += NC;
#pragma unroll
        for (int jc = 0; jc < NJ; jc++) sn[jc] = *(const f32x4 *)(Sr + 16 * jc);
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) an[ct] = ar[16 * ct];
      }
      float es = 0.0f;
#pragma unroll
      for (int jc = 0; jc < NJ; jc++) {
#pragma unroll
        for (int t = 0; t < 4; t++) es = fmaf(qa[jc][t], sv[jc][t], es);
      }
      es += __shfl_xor(es, 16);
      es += __shfl_xor(es, 32);            // e.s of chain node r, in all four lane groups
      float tot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
        const int col = 16 * ct + r;
        const float wv = p.w2p[col];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const float xv = acc[ct][rr] + av[ct];      // (one history for the whole tile)
          tot[rr] += col == 0 ? xv : wv * fmaxf(xv, 0.0f);
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) tot[rr] += __shfl_xor(tot[rr], o);
        tot[rr] += __shfl(es, 4 * g + rr);         // lane 4 g + rr (group 0) holds e.s of chain node 4 g + rr
        sum[rr] += (double)tot[rr];
      }
    }
    if (r == 0) {
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int xo = 16 * tile + 4 * g + rr;
        if (xo < nchain) p.part[sg * nchain + xo] = sum[rr];
      }
    }
  }
}

// one thread per (item, child): the items [i0, i0 + n) of a launch whose segments start at seg_base
__global__ void dfm_otm_tree_sum_kernel(const int64_t *seg_off, int64_t seg_base, int64_t i0, int64_t n, int gap, const double *part, double *weights) {
#pragma clang fp contract(off)
  const int nchild = 1 << gap, nchain = (2 << gap) - 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * nchild) return;
  const int64_t i = i0 + t / nchild;
  const int c = (int)(t % nchild);
  const int64_t s0 = seg_off[i] - seg_base, s1 = seg_off[i + 1] - seg_base;
  if (s0 == s1) { weights[i * nchild + c] = -1e6; return; }      // never appeared as a target (TreeConstruction.scala:201)
  double w = 0.0;
  int idx = c;
  for (int d = gap; d >= 1; d--) {
    const double *sc = part + ((1 << d) - 2 + idx);
    double s = 0.0;
    for (int64_t sg = s0; sg < s1; sg++) s = s + sc[sg * nchain];
    w = w + s;
    idx >>= 1;
  }
  weights[i * nchild + c] = w;
}

// ------------------------------------------------------------------------------------------------ host
// the segments of a catalogue: depends on row_off and the segment length only
struct DfmOtmSegList {
  DfmOtmSeg *d_seg = nullptr;
  int64_t *d_seg_off = nullptr;        // [items + 1]
  std::vector<int64_t> seg_off;        // its host copy
  int seg = 0;
  void release() { dm_release(d_seg, d_seg_off); seg_off.clear(); seg = 0; }
};

// what dm_deepfm_otm_tree_prepare keeps: the owner's, dropped with the weights
struct dm_dfm_otm_tree {
  float *S = nullptr, *aux = nullptr;
  std::vector<int64_t> row_off;        // from 0
  DfmOtmSegList segs;
  DevGrow part;
  uint64_t epoch = 0;
};

static void dfm_otm_tree_release(dm_ctx *h) {
  dm_dfm_otm_tree *t = h->dfm_otree;
  if (!t) return;
  dm_release(t->S, t->aux);
  t->segs.release();
  t->part.release();
  delete t;
  h->dfm_otree = nullptr;
}

static int dfm_otm_seg_list(dm_ctx *h, const int64_t *row_off, int64_t n_items, int seg, DfmOtmSegList &out) {
  out.release();
  out.seg_off.assign((size_t)n_items + 1, 0);
  for (int64_t i = 0; i < n_items; i++) out.seg_off[i + 1] = out.seg_off[i] + (row_off[i + 1] - row_off[i] + seg - 1) / seg;
  std::vector<DfmOtmSeg> sl((size_t)out.seg_off[n_items]);
  size_t q = 0;
  for (int64_t i = 0; i < n_items; i++)
    for (int64_t r0 = row_off[i]; r0 < row_off[i + 1]; r0 += seg) sl[q++] = {r0 - row_off[0], (int32_t)i, (int32_t)std::min<int64_t>(seg, row_off[i + 1] - r0)};
  int rc;
  if ((rc = dm_alloc(h, (void **)&out.d_seg, sl.size() * sizeof(DfmOtmSeg))) != DM_OK ||
      (rc = dm_alloc(h, (void **)&out.d_seg_off, out.seg_off.size() * 8)) != DM_OK) { out.release(); return rc; }
  hipError_t e = sl.empty() ? hipSuccess : hipMemcpyAsync(out.d_seg, sl.data(), sl.size() * sizeof(DfmOtmSeg), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out.d_seg_off, out.seg_off.data(), out.seg_off.size() * 8, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);        // (sl is pageable and dies here)
  if (e != hipSuccess) { out.release(); return fail(h, DM_ERR_HIP, std::string("dfm_otm_seg_list: upload failed: ") + hipGetErrorString(e)); }
  out.seg = seg;
  return DM_OK;
}

template <int E, int NCT>
static int dfm_otm_tree_launch_score(dm_ctx *h, const DfmOtmTreeScore &p) {
  int64_t blocks = (p.n_units + 3) / 4;
  if (blocks > (int64_t)h->n_cu * 16) blocks = (int64_t)h->n_cu * 16;
  if (const long long g_ = env_int("DM_DFM_OTM_TREE_GRID")) blocks = std::min<int64_t>(g_, 65535);      // (tests: several rounds of the unit loop)
  return timed(h, EV_DFM_OTM_TREE_SCORE, true, [&] {
    return LAUNCH(h, (dfm_otm_tree_score_kernel<E, NCT>), dim3((unsigned)blocks), dim3(256), dfm_frag_bytes(E, NCT), p);
  });
}

// the set-up of H histories (codes on the device) into S / aux
static int dfm_otm_tree_setup(dm_ctx *h, const int32_t *d_hcode, int64_t H, float *S, float *aux) {
  if (H <= 0) return DM_OK;
  const DfmBlocks b = dfm_blocks(h);
  DfmJtmRows r;
  r.emb = h->d_emb32; r.fragS = (const f32x4 *)h->d_dfm_fragS; r.l1_b = b.l1_b; r.b2 = h->b2; r.L = h->dfm_L; r.num_index = h->num_index;
  r.hcode = d_hcode; r.H = H; r.S = S; r.aux = aux;
  return dispatch_E_NCT(h, h->embed, dfm_col_tiles(h->dfm_L), "unsupported embed size", [&](auto e, auto n) { return dfm_jtm_launch_rows<decltype(e)::value, decltype(n)::value>(h, r); });
}

// The gap step on device arrays, asynchronous on the handle's stream: weights [n_items][1 << gap] double.  Items go in chunks of whole
// items that hold at most dfm_jtm_slice() histories (at least one item).  d_hcode != null (one-shot): the chunk's histories are set up into
// S / aux (room for the largest chunk) first; null (prepared): S / aux hold every history of the call.
static int64_t dfm_otm_tree_chunk_end(const int64_t *row_off, int64_t n_items, int64_t i0, int64_t slice) {
  int64_t i1 = i0, rows = 0;
  while (i1 < n_items) {
    const int64_t add = row_off[i1 + 1] - row_off[i1];
    if (i1 > i0 && rows + add > slice) break;
    rows += add; i1++;
  }
  return i1;
}

static int dfm_otm_tree_steps(dm_ctx *h, const int64_t *row_off, const DfmOtmSegList &sl, const int32_t *d_item_node, int64_t n_items, int gap,
                              const int32_t *d_hcode, float *S, float *aux, DevGrow &part, double *d_w) {
  const int E = h->embed, L = h->dfm_L, NCT = dfm_col_tiles(L), nchild = 1 << gap, nchain = (2 << gap) - 2, ntiles = (nchain + 15) / 16;
  const int64_t slice = dfm_jtm_slice();
  int64_t max_segs = 0;
  for (int64_t i0 = 0; i0 < n_items;) {
    const int64_t i1 = dfm_otm_tree_chunk_end(row_off, n_items, i0, slice);
    max_segs = std::max(max_segs, sl.seg_off[i1] - sl.seg_off[i0]);
    i0 = i1;
  }
  int rc = part.reserve(h, (size_t)std::max<int64_t>(max_segs, 1) * nchain * 8);
  if (rc != DM_OK) return rc;
  DfmOtmTreeScore p;
  p.emb = h->d_emb32; p.frag = (const f32x4 *)h->d_dfm_frag; p.w2p = h->d_dfm_w2p; p.S = S; p.aux = aux; p.item_node = d_item_node;
  p.part = (double *)part.p; p.num_index = h->num_index; p.gap = gap;
  for (int64_t i0 = 0; i0 < n_items;) {
    const int64_t i1 = dfm_otm_tree_chunk_end(row_off, n_items, i0, slice);
    const int64_t r0 = row_off[i0] - row_off[0], H = row_off[i1] - row_off[i0], s0 = sl.seg_off[i0], ns = sl.seg_off[i1] - s0;
    if (d_hcode && (rc = dfm_otm_tree_setup(h, d_hcode + r0 * L, H, S, aux)) != DM_OK) return rc;
    if (ns > 0) {
      p.segs = sl.d_seg + s0; p.n_units = ns * ntiles; p.row_base = d_hcode ? r0 : 0;
      rc = dispatch_E_NCT(h, E, NCT, "unsupported embed size", [&](auto e, auto n) { return dfm_otm_tree_launch_score<decltype(e)::value, decltype(n)::value>(h, p); });
      if (rc != DM_OK) return rc;
    }
    rc = timed(h, EV_DFM_OTM_TREE_SUM, true, [&] {
      return LAUNCH(h, dfm_otm_tree_sum_kernel, dim3((unsigned)(((i1 - i0) * nchild + 255) / 256)), dim3(256), 0, sl.d_seg_off, s0, i0, i1 - i0, gap, (const double *)part.p, d_w);
    });
    if (rc != DM_OK) return rc;
    i0 = i1;
  }
  return DM_OK;
}

// the refusals the two forms share: nothing is allocated or read through before they pass
static int dfm_otm_tree_check_rows(dm_ctx *h, const char *who, const int64_t *row_off, const int32_t *row_codes, int64_t n_items, int L) {
  if (!row_off || n_items < 0 || n_items >= ((int64_t)1 << 31)) return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  for (int64_t i = 0; i < n_items; i++)
    if (row_off[i + 1] < row_off[i]) return fail(h, DM_ERR_INVALID, std::string(who) + ": row_off must be non-decreasing");
  if (row_off[0] < 0) return fail(h, DM_ERR_INVALID, std::string(who) + ": row_off must not be negative");
  const int64_t R = row_off[n_items] - row_off[0];
  if (R > 0 && !row_codes) return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  return R > 0 ? check_lookup_ids(h, row_codes + row_off[0] * L, R * L, L, "history") : DM_OK;
}
static int dfm_otm_tree_check_step(dm_ctx *h, const char *who, const int32_t *item_node, int64_t n_items, int old_level, int level) {
  if (old_level < 0 || level <= old_level || level - old_level > 8 || level > 30) return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  const int64_t lo = ((int64_t)1 << old_level) - 1, hi = ((int64_t)2 << old_level) - 2;
  for (int64_t i = 0; i < n_items; i++)
    if (item_node[i] < lo || item_node[i] > hi)
      return fail(h, DM_ERR_INVALID, std::string(who) + ": item_node " + std::to_string(item_node[i]) + " of item " + std::to_string(i) + " is not a node of level " + std::to_string(old_level));
  if ((((int64_t)1) << (level + 1)) - 1 > h->num_index) return fail(h, DM_ERR_INDEX, std::string(who) + ": level exceeds the embedding table");
  return DM_OK;
}

// d_w -> weights after the steps; nothing is freed under a running kernel
static int dfm_otm_tree_finish(dm_ctx *h, const char *who, int rc, const double *d_w, double *weights, size_t n) {
  hipError_t e = hipSuccess;
  if (rc == DM_OK) e = hipMemcpyAsync(weights, d_w, n * 8, hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);
  if (rc != DM_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess) return fail(h, DM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e != hipSuccess ? e : e2));
  return DM_OK;
}

int dm_deepfm_otm_child_weights(dm_handle_t h, const int64_t *row_off, const int32_t *row_codes, const int32_t *item_node,
                                int64_t n_items, int L, int old_level, int level, int use_mask, double *weights) {
  static const char who[] = "dm_deepfm_otm_child_weights";
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  int rc = dfm_jtm_enter(h, who, use_mask, L);
  if (rc != DM_OK) return rc;
  if (!row_off || !item_node || !weights || n_items < 0) return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  if ((rc = dfm_otm_tree_check_step(h, who, item_node, n_items, old_level, level)) != DM_OK) return rc;
  if ((rc = dfm_otm_tree_check_rows(h, who, row_off, row_codes, n_items, L)) != DM_OK) return rc;
  if (n_items == 0) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const int gap = level - old_level, nchild = 1 << gap, E = h->embed, NC = dfm_col_tiles(L) * 16;
  const int64_t R = row_off[n_items] - row_off[0], slice = dfm_jtm_slice();
  int64_t max_rows = 1;
  for (int64_t i0 = 0; i0 < n_items;) {
    const int64_t i1 = dfm_otm_tree_chunk_end(row_off, n_items, i0, slice);
    max_rows = std::max(max_rows, row_off[i1] - row_off[i0]);
    i0 = i1;
  }
  const size_t o_aux = DevArena::up((size_t)max_rows * E * 4);
  if ((rc = h->dfm_jtm_ws.reserve(h, o_aux + (size_t)max_rows * NC * 4)) != DM_OK) return rc;      // (grows for an item larger than the slice)
  DevTemps t(h);
  DfmOtmSegList sl;
  struct Drop { DfmOtmSegList &s; ~Drop() { s.release(); } } drop{sl};
  DevGrow part;
  struct DropG { DevGrow &g; ~DropG() { g.release(); } } dropg{part};
  int32_t *d_hcode = nullptr, *d_node = nullptr;
  double *d_w = nullptr;
  if ((rc = t.alloc(d_hcode, (size_t)std::max<int64_t>(R, 1) * L * 4)) != DM_OK || (rc = t.alloc(d_node, (size_t)n_items * 4)) != DM_OK ||
      (rc = t.alloc(d_w, (size_t)n_items * nchild * 8)) != DM_OK)
    return rc;
  if ((rc = dfm_otm_seg_list(h, row_off, n_items, dfm_otm_tree_seg(), sl)) != DM_OK) return rc;
  hipError_t e = R > 0 ? hipMemcpyAsync(d_hcode, row_codes + row_off[0] * L, (size_t)R * L * 4, hipMemcpyHostToDevice, h->stream) : hipSuccess;      // once per call
  if (e == hipSuccess) e = hipMemcpyAsync(d_node, item_node, (size_t)n_items * 4, hipMemcpyHostToDevice, h->stream);
  if (e != hipSuccess) { (void)hipStreamSynchronize(h->stream); return fail(h, DM_ERR_HIP, std::string(who) + ": upload failed"); }
  rc = dfm_otm_tree_steps(h, row_off, sl, d_node, n_items, gap, d_hcode, (float *)h->dfm_jtm_ws.p, (float *)((char *)h->dfm_jtm_ws.p + o_aux), part, d_w);
  return dfm_otm_tree_finish(h, who, rc, d_w, weights, (size_t)n_items * nchild);
}

int dm_deepfm_otm_tree_release(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_otm_tree_release");
  if (!h->dfm_otree) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfm_otm_tree_release(h);
  return DM_OK;
}

int dm_deepfm_otm_tree_prepare(dm_handle_t h, const int64_t *row_off, const int32_t *row_codes, int64_t n_items, int L) {
  static const char who[] = "dm_deepfm_otm_tree_prepare";
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_otm_tree_prepare");
  int rc = dfm_jtm_enter(h, who, 0, L);
  if (rc != DM_OK) return rc;
  if ((rc = dfm_otm_tree_check_rows(h, who, row_off, row_codes, n_items, L)) != DM_OK) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dfm_otm_tree_release(h);             // a second prepare replaces the first
  const int E = h->embed, NC = dfm_col_tiles(L) * 16;
  const int64_t R = row_off[n_items] - row_off[0], slice = dfm_jtm_slice();
  dm_dfm_otm_tree *t = new dm_dfm_otm_tree();
  h->dfm_otree = t;
  t->row_off.resize((size_t)n_items + 1);
  for (int64_t i = 0; i <= n_items; i++) t->row_off[i] = row_off[i] - row_off[0];
  {
    DevTemps tmp(h);                   // the codes: dropped after the set-up
    int32_t *d_hcode = nullptr;
    rc = dm_alloc(h, (void **)&t->S, (size_t)std::max<int64_t>(R, 1) * E * 4);
    if (rc == DM_OK) rc = dm_alloc(h, (void **)&t->aux, (size_t)std::max<int64_t>(R, 1) * NC * 4);
    if (rc == DM_OK) rc = tmp.alloc(d_hcode, (size_t)std::max<int64_t>(R, 1) * L * 4);
    if (rc == DM_OK && R > 0 && hipMemcpyAsync(d_hcode, row_codes + row_off[0] * L, (size_t)R * L * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess)
      rc = fail(h, DM_ERR_HIP, std::string(who) + ": upload failed");
    for (int64_t h0 = 0; h0 < R && rc == DM_OK; h0 += slice)
      rc = dfm_otm_tree_setup(h, d_hcode + h0 * L, std::min(slice, R - h0), t->S + h0 * E, t->aux + h0 * NC);
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == DM_OK) rc = fail(h, DM_ERR_HIP, std::string(who) + ": device pass failed");
  }
  if (rc == DM_OK) rc = dfm_otm_seg_list(h, t->row_off.data(), n_items, dfm_otm_tree_seg(), t->segs);
  if (rc != DM_OK) { dfm_otm_tree_release(h); return rc; }      // nothing is kept
  t->epoch = h->model_epoch.load();
  return DM_OK;
}

int dm_deepfm_otm_tree_weights(dm_handle_t h, const int32_t *item_node, int64_t n_items, int old_level, int level, double *weights) {
  static const char who[] = "dm_deepfm_otm_tree_weights";
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_deepfm_otm_tree_weights");
  int rc = dfm_jtm_enter(h, who, 0, -1);
  if (rc != DM_OK) return rc;
  if (!item_node || !weights || n_items < 0) return fail(h, DM_ERR_INVALID, std::string(who) + ": bad arguments");
  dm_dfm_otm_tree *t = h->dfm_otree;
  if (!t) return fail(h, DM_ERR_STATE, std::string(who) + ": call dm_deepfm_otm_tree_prepare first");
  if (n_items != (int64_t)t->row_off.size() - 1)
    return fail(h, DM_ERR_STATE, std::string(who) + ": " + std::to_string(n_items) + " items, but " + std::to_string(t->row_off.size() - 1) + " were prepared");
  if (t->epoch != h->model_epoch.load()) return fail(h, DM_ERR_STATE, std::string(who) + ": the model changed since dm_deepfm_otm_tree_prepare (prepare again)");
  if ((rc = dfm_otm_tree_check_step(h, who, item_node, n_items, old_level, level)) != DM_OK) return rc;
  if (n_items == 0) return DM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const int gap = level - old_level, nchild = 1 << gap, seg = dfm_otm_tree_seg();
  if (t->segs.seg != seg && (rc = dfm_otm_seg_list(h, t->row_off.data(), n_items, seg, t->segs)) != DM_OK) return rc;
  DevTemps tmp(h);
  int32_t *d_node = nullptr;
  double *d_w = nullptr;
  if ((rc = tmp.alloc(d_node, (size_t)n_items * 4)) != DM_OK || (rc = tmp.alloc(d_w, (size_t)n_items * nchild * 8)) != DM_OK) return rc;
  if (hipMemcpyAsync(d_node, item_node, (size_t)n_items * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    return fail(h, DM_ERR_HIP, std::string(who) + ": upload failed");
  }
  rc = dfm_otm_tree_steps(h, t->row_off.data(), t->segs, d_node, n_items, gap, nullptr, t->S, t->aux, t->part, d_w);
  return dfm_otm_tree_finish(h, who, rc, d_w, weights, (size_t)n_items * nchild);
}
