// Model checkpoint: the state TDM.saveModel / loadModel keep (tdm/src/main/scala/com/mass/tdm/utils/Serialization.scala:60-101
// serialises the whole module graph with Java's ObjectOutputStream; tdm/src/test/scala/TdmModelTrainSpec.scala:85-96 pins
// "save -> load -> identical recommendations") as ONE flat little-endian file: header, the compact parameter vector in
// Graph.parameters order (SURVEY.md row A0) in the loaded dtype, and the index arrays (tree nodes, item id -> leaf code).  Like
// the reference's format it holds no optimizer state (Adam.buffer is transient, scalann/.../optim/Adam.scala:85-88).
//
//   char     magic[8] = "DMHIPCK1"
//   int32    version (1), dtype (DM_F32 | DM_F64), embed, max_level, has_tree, has_ids,
//            reserved[0] = scorer kind (0 DIN, 1 DeepFM), reserved[1] = DeepFM's seq_len (0 for DIN): a DIN file has both words 0, as ever
//   int64    num_index, n_elems, n_nodes, n_leaf_ids
//   [has_tree] int32 codes[n_nodes]; int32 node_ids[n_nodes]; uint8 is_leaf[n_nodes] (+ padding to 8 bytes)
//   [has_ids]  int32 leaf_item_ids[n_leaf_ids]; int32 leaf_codes[n_leaf_ids]
//   elem     compact[n_elems]      (DIN: SURVEY.md row A0; DeepFM: deepfm.hip.inc; always the MODEL's embed size, never the padded one)

#include <sys/stat.h>

struct dm_ckpt_header {
  char magic[8];
  int32_t version, dtype, embed, max_level, has_tree, has_ids, reserved[2];
  int64_t num_index, n_elems, n_nodes, n_leaf_ids;
};

static bool ckpt_write(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
static bool ckpt_read(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// Both entry points keep every exception inside (a corrupt header must not abort a JVM through JNI): the bodies run under
// try / catch and report DM_ERR_INVALID.
static int save_model_body(dm_ctx *h, const char *path) {
  if (!path) return fail(h, DM_ERR_INVALID, "dm_save_model: path is NULL");
  if (!h->w_loaded) return fail(h, DM_ERR_STATE, "dm_save_model: weights not loaded");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dm_ckpt_header hd;
  memset(&hd, 0, sizeof hd);
  memcpy(hd.magic, "DMHIPCK1", 8);
  hd.version = 1; hd.dtype = h->dtype; hd.embed = h->embed_log; hd.max_level = h->max_level;      // the MODEL's embed size
  hd.has_tree = h->tree_loaded ? 1 : 0; hd.has_ids = h->ids_loaded ? 1 : 0;
  hd.num_index = h->num_index;
  const int64_t E = h->embed_log;
  const bool dfm = h->scorer_kind == DM_KIND_DEEPFM;
  hd.n_elems = dfm ? deepfm_len_for(h->num_index, E, h->dfm_L) : h->num_index * E + 3 * E * E + 2 * E + 1;
  if (dfm) { hd.reserved[0] = DM_KIND_DEEPFM; hd.reserved[1] = h->dfm_L; }
  std::vector<int32_t> codes, nids, lids, lcodes;
  std::vector<uint8_t> isleaf;
  if (h->tree_loaded) {
    const int64_t words = (h->n_slots + 31) / 32 + 1;
    std::vector<uint32_t> ex((size_t)words), lf((size_t)words);
    std::vector<int32_t> nid((size_t)h->n_slots);
    HIPCHK(h, hipMemcpy(ex.data(), h->d_exists, (size_t)words * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(lf.data(), h->d_leaf, (size_t)words * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(nid.data(), h->d_node_id, (size_t)h->n_slots * 4, hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < h->n_slots; c++)
      if ((ex[(size_t)(c >> 5)] >> (c & 31)) & 1u) {
        codes.push_back((int32_t)c); nids.push_back(nid[(size_t)c]); isleaf.push_back((uint8_t)((lf[(size_t)(c >> 5)] >> (c & 31)) & 1u));
      }
  }
  if (h->ids_loaded)
    for (size_t id = 0; id < h->h_id_to_code.size(); id++)
      if (h->h_id_to_code[id] >= 0) { lids.push_back((int32_t)id); lcodes.push_back(h->h_id_to_code[id]); }
  hd.n_nodes = (int64_t)codes.size(); hd.n_leaf_ids = (int64_t)lids.size();
  // padded models: the file holds the model's own layout (dm_train_download strips the padding); fetched BEFORE the file is touched
  std::vector<char> lv;
  if (h->embed_log != h->embed) {
    lv.resize((size_t)hd.n_elems * (h->dtype == DM_F64 ? 8 : 4));
    int rc_;
    if (dfm) {
      std::vector<float> m;
      if ((rc_ = dfm_download_model(h, m)) == DM_OK) memcpy(lv.data(), m.data(), lv.size());
    } else rc_ = dm_train_download(h, 0, lv.data(), hd.n_elems);
    if (rc_ != DM_OK) return rc_;
  }
  // written next to the target and renamed over it on success: a failed save leaves the previous checkpoint intact (the reference
  // serialises to memory before it opens the file, T/utils/Serialization.scala:60-75)
  // (a unique temporary name: several worker threads, each with its own handle, may save to the same path)
  static std::atomic<unsigned> seq_{0};
  const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid()) + "." + std::to_string(seq_.fetch_add(1));
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return fail(h, DM_ERR_INVALID, std::string("dm_save_model: cannot open ") + tmp + ": " + strerror(errno));
  auto abandon = [&](int rc_) { fclose(f); (void)remove(tmp.c_str()); return rc_; };
  bool ok = ckpt_write(f, &hd, sizeof hd);
  if (h->tree_loaded) {
    const uint8_t pad[8] = {0};
    ok = ok && ckpt_write(f, codes.data(), codes.size() * 4) && ckpt_write(f, nids.data(), nids.size() * 4) &&
         ckpt_write(f, isleaf.data(), isleaf.size()) && ckpt_write(f, pad, (8 - isleaf.size() % 8) % 8);
  }
  if (h->ids_loaded) ok = ok && ckpt_write(f, lids.data(), lids.size() * 4) && ckpt_write(f, lcodes.data(), lcodes.size() * 4);
  if (h->embed_log != h->embed) ok = ok && ckpt_write(f, lv.data(), lv.size());
  else {
    // the compact vector in slices: a 34 GB table does not need a host copy of its own size
    const size_t es = h->dtype == DM_F64 ? 8 : 4, total = (size_t)hd.n_elems * es, slice = (size_t)256 << 20;
    std::vector<char> buf(total < slice ? total : slice);
    for (size_t off = 0; ok && off < total; off += slice) {
      const size_t n = total - off < slice ? total - off : slice;
      if (hipMemcpy(buf.data(), (const char *)h->d_compact + off, n, hipMemcpyDeviceToHost) != hipSuccess) return abandon(fail(h, DM_ERR_HIP, "dm_save_model: download failed"));
      ok = ckpt_write(f, buf.data(), n);
    }
  }
  ok = (fflush(f) == 0) && ok;
  ok = (fsync(fileno(f)) == 0) && ok;          // the data is on the disk before the rename publishes the name (a crash leaves the old file or the new one, never a torn one)
  ok = (fclose(f) == 0) && ok;
  if (!ok) { (void)remove(tmp.c_str()); return fail(h, DM_ERR_INVALID, std::string("dm_save_model: write to ") + tmp + " failed"); }
  if (rename(tmp.c_str(), path) != 0) { (void)remove(tmp.c_str()); return fail(h, DM_ERR_INVALID, std::string("dm_save_model: cannot rename onto ") + path + ": " + strerror(errno)); }
  return DM_OK;
}

int dm_save_model(dm_handle_t h, const char *path) {
  if (!h) return DM_ERR_INVALID;
  DM_CLONE_ENTER(h);
  try { return save_model_body(h, path); }
  catch (const std::exception &e) { return fail(h, DM_ERR_INVALID, std::string("dm_save_model: ") + e.what()); }
}

// The file is validated against its own size before anything is allocated from its header, every section is read into temporaries, the
// weights go to a fresh device buffer — and only when all of that has succeeded does the handle change (weights, then tree, then id
// maps): a corrupt or truncated file leaves the handle exactly as it was.  (Everything dm_load_tree_tdm / dm_load_id_maps validate is
// checked on the temporaries first; what can still fail between the three commits is a device allocation, and then the handle holds the
// new weights with the old tree — the error is returned.)
static int load_model_body(dm_ctx *h, FILE *f) {
  dm_ckpt_header hd;
  struct stat st;
  if (fstat(fileno(f), &st) != 0) return fail(h, DM_ERR_INVALID, "dm_load_model: cannot stat the file");
  const uint64_t fsize = (uint64_t)st.st_size;
  if (!ckpt_read(f, &hd, sizeof hd) || memcmp(hd.magic, "DMHIPCK1", 8) != 0 || hd.version != 1)
    return fail(h, DM_ERR_INVALID, "dm_load_model: not a dismember_hip checkpoint (version 1)");
  const int64_t E = hd.embed;
  if ((hd.dtype != DM_F32 && hd.dtype != DM_F64) || E < 1 || E > 128 || hd.max_level < 0 || hd.max_level > 30 ||
      (hd.has_tree != 0 && hd.has_tree != 1) || (hd.has_ids != 0 && hd.has_ids != 1))
    return fail(h, DM_ERR_INVALID, "dm_load_model: header fields out of range");
  // every count is bounded by the file's size BEFORE it enters a product or an allocation (no overflow: each factor < 2^40)
  const uint64_t es = hd.dtype == DM_F64 ? 8 : 4;
  if (hd.num_index <= 0 || (uint64_t)hd.num_index > fsize / es || hd.n_nodes < 0 || (uint64_t)hd.n_nodes > fsize / 9 ||
      hd.n_leaf_ids < 0 || (uint64_t)hd.n_leaf_ids > fsize / 8 || (!hd.has_tree && hd.n_nodes) || (!hd.has_ids && hd.n_leaf_ids))
    return fail(h, DM_ERR_INVALID, "dm_load_model: header counts exceed the file");
  const int kind = hd.reserved[0], seq_len = hd.reserved[1];
  if ((kind != DM_KIND_DIN && kind != DM_KIND_DEEPFM) || (kind == DM_KIND_DIN && seq_len != 0) ||
      (kind == DM_KIND_DEEPFM && (seq_len < 1 || seq_len > DFM_MAXL || hd.dtype != DM_F32)))
    return fail(h, DM_ERR_INVALID, "dm_load_model: unknown scorer in the header (kind / seq_len words)");
  if (hd.n_elems != (kind == DM_KIND_DEEPFM ? deepfm_len_for(hd.num_index, E, seq_len) : hd.num_index * E + 3 * E * E + 2 * E + 1))
    return fail(h, DM_ERR_INVALID, "dm_load_model: inconsistent header");
  const uint64_t tree_bytes = hd.has_tree ? (uint64_t)hd.n_nodes * 8 + (((uint64_t)hd.n_nodes + 7) & ~(uint64_t)7) : 0;
  const uint64_t ids_bytes = hd.has_ids ? (uint64_t)hd.n_leaf_ids * 8 : 0;
  const uint64_t total = (uint64_t)hd.n_elems * es;
  if (sizeof hd + tree_bytes + ids_bytes + total != fsize) return fail(h, DM_ERR_INVALID, "dm_load_model: truncated file (size does not match the header)");
  std::vector<int32_t> codes, nids, lids, lcodes;
  std::vector<uint8_t> isleaf;
  if (hd.has_tree) {
    codes.resize((size_t)hd.n_nodes); nids.resize((size_t)hd.n_nodes); isleaf.resize((size_t)(((uint64_t)hd.n_nodes + 7) & ~(uint64_t)7));
    if (!ckpt_read(f, codes.data(), codes.size() * 4) || !ckpt_read(f, nids.data(), nids.size() * 4) || !ckpt_read(f, isleaf.data(), isleaf.size()))
      return fail(h, DM_ERR_INVALID, "dm_load_model: truncated file (tree)");
    if (hd.n_nodes == 0) return fail(h, DM_ERR_INVALID, "dm_load_model: empty tree section");
    const int64_t lim = ((int64_t)2 << hd.max_level) - 1;
    for (int64_t i = 0; i < hd.n_nodes; i++)
      if (codes[(size_t)i] < 0 || codes[(size_t)i] >= lim) return fail(h, DM_ERR_INVALID, "dm_load_model: tree code outside the levels of the header");
  }
  if (hd.has_ids) {
    lids.resize((size_t)hd.n_leaf_ids); lcodes.resize((size_t)hd.n_leaf_ids);
    if (!ckpt_read(f, lids.data(), lids.size() * 4) || !ckpt_read(f, lcodes.data(), lcodes.size() * 4))
      return fail(h, DM_ERR_INVALID, "dm_load_model: truncated file (id map)");
    if (hd.n_leaf_ids == 0) return fail(h, DM_ERR_INVALID, "dm_load_model: empty id-map section");
    for (int64_t i = 0; i < hd.n_leaf_ids; i++)
      if (lids[(size_t)i] < 0 || lcodes[(size_t)i] < 0) return fail(h, DM_ERR_INVALID, "dm_load_model: negative entry in the id map");
  }
  int rc = DM_OK;
  if (kind == DM_KIND_DEEPFM || native_embed(hd.embed) != hd.embed) {          // DeepFM, or an embed size the kernels pad: through the host loader
    std::vector<char> lv((size_t)total);
    if (!ckpt_read(f, lv.data(), lv.size())) return fail(h, DM_ERR_INVALID, "dm_load_model: truncated file (weights)");
    rc = kind == DM_KIND_DEEPFM ? dm_load_weights_deepfm(h, hd.dtype, hd.embed, seq_len, hd.num_index, lv.data(), hd.n_elems)
                                : dm_load_weights_din(h, hd.dtype, hd.embed, hd.num_index, lv.data(), hd.n_elems);
  } else {
    // weights: straight into a device buffer the handle then owns (no host copy of the table's size)
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, DM_ERR_HIP, "hipSetDevice failed");
    const size_t slice = (size_t)256 << 20;
    void *d = nullptr;
    if ((rc = dm_alloc(h, &d, (size_t)total)) != DM_OK) return rc;
    std::vector<char> buf((size_t)(total < slice ? total : slice));
    bool ok = true;
    for (size_t off = 0; ok && off < total; off += slice) {
      const size_t n = total - off < slice ? (size_t)(total - off) : slice;
      ok = ckpt_read(f, buf.data(), n) && hipMemcpy((char *)d + off, buf.data(), n, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { dm_release(d); return fail(h, DM_ERR_INVALID, "dm_load_model: truncated file (weights)"); }
    rc = hd.dtype == DM_F64 ? dm_load_weights_din_dev_f64(h, hd.embed, hd.num_index, (double *)d, hd.n_elems)
                            : dm_load_weights_din_dev(h, hd.embed, hd.num_index, (float *)d, hd.n_elems);
    if (rc != DM_OK && h->d_compact != d) dm_release(d);
  }
  if (rc != DM_OK) return rc;
  if (hd.has_tree && (rc = dm_load_tree_tdm(h, codes.data(), nids.data(), isleaf.data(), hd.n_nodes, hd.max_level)) != DM_OK) return rc;
  if (hd.has_ids && (rc = dm_load_id_maps(h, lids.data(), lcodes.data(), hd.n_leaf_ids)) != DM_OK) return rc;
  return DM_OK;
}

int dm_load_model(dm_handle_t h, const char *path) {
  if (!h) return DM_ERR_INVALID;
  DM_OWNER_ONLY(h, "dm_load_model");
  if (!path) return fail(h, DM_ERR_INVALID, "dm_load_model: path is NULL");
  FILE *f = fopen(path, "rb");
  if (!f) return fail(h, DM_ERR_INVALID, std::string("dm_load_model: cannot open ") + path + ": " + strerror(errno));
  int rc;
  try { rc = load_model_body(h, f); }
  catch (const std::exception &e) { rc = fail(h, DM_ERR_INVALID, std::string("dm_load_model: ") + e.what()); }
  fclose(f);
  return rc;
}
