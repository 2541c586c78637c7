// Device memory (host code only): the one place that frees it, and the three shapes every allocation in the library has.
//   dm_release(p, q, ...)  frees and nulls raw pointers (the handle's members stay raw: clones copy them field by field)
//   DevGrow / DevArena     a grow-only buffer, and the 256-byte-aligned layout of one call's arrays inside it
//   DevTemps               the temporaries of one call: what alloc() handed out is freed at scope exit, nothing else is
// Ownership follows registration: a pointer taken from the handle's cache or from the caller was never given to a DevTemps and is
// never freed by one.  dm_alloc (dm_hip.hip) is the only hipMalloc; both ends count the live allocations (dm_debug_live_device_allocs).
// The byte count has to know at free time what an allocation's size was, so next to the two atomics there is a pointer -> size map under
// a process-wide mutex, taken once per dm_alloc and once per free (both next to a hipMalloc / hipFree, never on a request path that
// has seen its largest request).  A pointer dm_alloc never handed out (a foreign one given to dm_dev_free) is freed but not counted.
struct dm_ctx;
static int dm_alloc(dm_ctx *h, void **p, size_t bytes);

static std::atomic<unsigned long long> g_live_count{0}, g_live_bytes{0};
static std::mutex g_live_mu;
static std::unordered_map<const void *, size_t> g_live_size;

static void dm_live_add(const void *p, size_t bytes) {
  { std::lock_guard<std::mutex> lk(g_live_mu); g_live_size[p] = bytes; }
  g_live_count.fetch_add(1); g_live_bytes.fetch_add(bytes);
}
static hipError_t dm_free_one(void *p) {
  if (!p) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    auto it = g_live_size.find(p);
    if (it != g_live_size.end()) { g_live_count.fetch_sub(1); g_live_bytes.fetch_sub(it->second); g_live_size.erase(it); }
  }
  return hipFree(p);
}
template <typename... T>
static void dm_release(T *&...p) { (((void)dm_free_one((void *)p), p = nullptr), ...); }

extern "C" int dm_debug_live_device_allocs(unsigned long long *count, unsigned long long *bytes) {
  if (!count || !bytes) return DM_ERR_INVALID;
  *count = g_live_count.load(); *bytes = g_live_bytes.load();
  return DM_OK;
}

// ---- grow only: a block that is replaced by one of need + slack bytes when it is too small, and otherwise left alone
struct DevGrow {
  void *p = nullptr; size_t bytes = 0;
  int reserve(dm_ctx *h, size_t need, size_t slack = 0) {
    if (bytes >= need) return DM_OK;
    release();
    const int rc = dm_alloc(h, &p, need + slack);
    if (rc != DM_OK) { p = nullptr; return rc; }
    bytes = need + slack;
    return DM_OK;
  }
  void release() { dm_release(p); bytes = 0; }
};

// ---- the arrays of one call laid out in a DevGrow: add() every array, commit(), then ptr<T>(offset).  Offsets are multiples of 256
// bytes; a buffer that has to grow grows to need + need / slack_div (0: no slack).
struct DevArena {
  DevGrow &buf; size_t slack_div; size_t need = 0; char *base = nullptr;
  explicit DevArena(DevGrow &b, size_t slack_div_ = 0) : buf(b), slack_div(slack_div_) {}
  static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }
  size_t add(size_t bytes) { const size_t off = need; need += up(bytes); return off; }
  int commit(dm_ctx *h) {
    const int rc = buf.reserve(h, need, slack_div ? need / slack_div : 0);
    base = (char *)buf.p;
    return rc;
  }
  template <typename T> T *ptr(size_t off) const { return (T *)(base + off); }
};

// ---- the temporaries of one call
struct DevTemps {
  dm_ctx *h; std::vector<void *> owned;
  explicit DevTemps(dm_ctx *h_) : h(h_) {}
  DevTemps(const DevTemps &) = delete;
  DevTemps &operator=(const DevTemps &) = delete;
  ~DevTemps() { for (void *p : owned) (void)dm_free_one(p); }
  template <typename T> int alloc(T *&p, size_t bytes) {
    void *v = nullptr;
    const int rc = dm_alloc(h, &v, bytes);
    if (rc != DM_OK) return rc;
    owned.push_back(v); p = (T *)v;
    return DM_OK;
  }
  template <typename T> void drop(T *&p) {          // early release of one pointer (a buffer regrown inside a loop); not ours: only nulled
    auto it = std::find(owned.begin(), owned.end(), (void *)p);
    if (it != owned.end()) { (void)dm_free_one(*it); owned.erase(it); }
    p = nullptr;
  }
  void drop_from(size_t mark) {                     // ... or of everything allocated since owned.size() was `mark`
    while (owned.size() > mark) { (void)dm_free_one(owned.back()); owned.pop_back(); }
  }
};
