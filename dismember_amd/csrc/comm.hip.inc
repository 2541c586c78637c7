// Multi-GPU exchange behind the C ABI (SURVEY.md §5, §8e): the reference's only "collective" is the in-process average of the
// per-thread gradient buffers, LocalOptimizer.syncGradients (tdm/src/main/scala/com/mass/tdm/optim/LocalOptimizer.scala:164-187;
// OTM: otm/.../optim/LocalOptimizer.scala:217-233).  With one worker per GPU it becomes
//   * ncclAllReduce(sum) of the dense block [att.W ; l1.W ; l1.b ; l2.W ; l2.b] (198 KB at E = 128), and
//   * an all-gather of every worker's touched embedding rows (index, gradient row) — never a ring over the 17 GB table —
//     after which each replica rebuilds every touched row as 0 + g_0 + g_1 + ... in RANK order, so all replicas hold the
//     same bits and stay identical with no parameter broadcast; the 1/N is folded into dm_adam_step.
// Two transports implement the same primitives (var-size all-gather of device or host buffers, all-reduce of the dense block):
//   DM_COMM_RCCL  RCCL over xGMI, one rank per GPU (multi-process via ncclCommInitRank, or one process driving N handles via
//                 ncclCommInitAll + group calls: dm_comm_create_all / dm_allreduce_grads).
//   DM_COMM_HOST  a TCP star through rank 0 with device buffers staged through host memory: several worker processes on ONE
//                 GPU (RCCL refuses two ranks on one device), which is how the protocol is tested on a single-GPU box, and
//                 CPU-only processes for the host-buffer collectives.
#include <rccl/rccl.h>

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <unistd.h>

struct dm_comm {
  int nranks = 1, rank = 0, kind = DM_COMM_HOST, device = -1;
  ncclComm_t nccl = nullptr;
  hipStream_t stream = nullptr;          // RCCL kind: stream of the comm-level (host-buffer) collectives
  void *d_stage = nullptr; size_t stage_bytes = 0;
  std::vector<int> fds;                  // HOST kind: rank 0 holds fds[r] for r >= 1; rank r holds fds[0]
  std::string err;
};
static std::string g_comm_err;

static int comm_fail(dm_comm *c, int code, const std::string &msg) {
  if (c) c->err = msg; else g_comm_err = msg;
  return code;
}
#define NCCLCHK(c, call)                                                                            \
  do {                                                                                              \
    ncclResult_t r_ = (call);                                                                       \
    if (r_ != ncclSuccess) return comm_fail((c), DM_ERR_HIP, std::string(#call " failed: ") + ncclGetErrorString(r_)); \
  } while (0)
#define CHIPCHK(c, call)                                                                            \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) return comm_fail((c), DM_ERR_HIP, std::string(#call " failed: ") + hipGetErrorString(e_)); \
  } while (0)

static bool sock_send(int fd, const void *buf, size_t n) {
  const char *p = (const char *)buf;
  while (n) { ssize_t k = ::send(fd, p, n, MSG_NOSIGNAL); if (k <= 0) return false; p += k; n -= (size_t)k; }
  return true;
}
static bool sock_recv(int fd, void *buf, size_t n) {
  char *p = (char *)buf;
  while (n) { ssize_t k = ::recv(fd, p, n, 0); if (k <= 0) return false; p += k; n -= (size_t)k; }
  return true;
}

static void comm_close_sockets(dm_comm *c) {
  for (int fd : c->fds) if (fd >= 0) ::close(fd);
  c->fds.clear();
}

// rank 0 listens on addr:port, ranks 1..n-1 connect (retrying for up to ~120 s) and announce their rank
static int comm_rendezvous(dm_comm *c, const char *addr, int port) {
  c->fds.assign(c->nranks, -1);
  if (c->nranks == 1) return DM_OK;
  struct addrinfo hints{}, *res = nullptr;
  hints.ai_family = AF_INET; hints.ai_socktype = SOCK_STREAM;
  char ps[16]; snprintf(ps, sizeof ps, "%d", port);
  if (getaddrinfo(addr && *addr ? addr : "127.0.0.1", ps, &hints, &res) != 0 || !res)
    return comm_fail(c, DM_ERR_INVALID, std::string("dm_comm: cannot resolve ") + (addr ? addr : "(null)"));
  const int one = 1;
  int rc = DM_OK;
  const std::string where = std::string(addr && *addr ? addr : "127.0.0.1") + ":" + ps;
  if (c->rank == 0) {
    int ls = ::socket(AF_INET, SOCK_STREAM, 0);
    setsockopt(ls, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
    if (ls < 0 || ::bind(ls, res->ai_addr, res->ai_addrlen) != 0 || ::listen(ls, c->nranks) != 0) {
      rc = comm_fail(c, DM_ERR_INVALID, "dm_comm: rank 0 cannot listen on " + where + " (" + strerror(errno) + ")");
      if (ls >= 0) ::close(ls);
    } else {
      // a peer that never arrives must not hang rank 0: the listening socket gets the same 120 s the connecting side retries for
      struct timeval tv{120, 0};
      setsockopt(ls, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
      for (int k = 1; k < c->nranks && rc == DM_OK; k++) {
        int fd = ::accept(ls, nullptr, nullptr);
        int32_t r = -1;
        if (fd >= 0) { struct timeval t1{30, 0}; setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &t1, sizeof t1); }
        if (fd < 0 || !sock_recv(fd, &r, 4) || r <= 0 || r >= c->nranks || c->fds[r] >= 0) {
          rc = comm_fail(c, DM_ERR_INVALID, fd < 0 ? "dm_comm: rendezvous timed out waiting for a peer at " + where : std::string("dm_comm: bad peer during rendezvous"));
          if (fd >= 0) ::close(fd);
          break;
        }
        { struct timeval t0{0, 0}; setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &t0, sizeof t0); }     // collectives block as long as the slowest rank computes
        setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
        c->fds[r] = fd;
      }
      ::close(ls);
    }
  } else {
    int fd = -1;
    for (int attempt = 0; attempt < 1200; attempt++) {
      fd = ::socket(AF_INET, SOCK_STREAM, 0);
      if (fd >= 0 && ::connect(fd, res->ai_addr, res->ai_addrlen) == 0) break;
      if (fd >= 0) ::close(fd);
      fd = -1;
      usleep(100 * 1000);
    }
    const int32_t r = c->rank;
    if (fd < 0 || !sock_send(fd, &r, 4)) {
      rc = comm_fail(c, DM_ERR_INVALID, "dm_comm: cannot reach rank 0 at " + where);
      if (fd >= 0) ::close(fd);
    } else {
      setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
      c->fds[0] = fd;
    }
  }
  freeaddrinfo(res);
  return rc;
}

// ---- HOST transport: var-size all-gather through rank 0.  recv gets the blocks in rank order, sizes[r] their lengths.
static int host_all_gather_v(dm_comm *c, const void *send, size_t bytes, std::vector<char> &recv, std::vector<uint64_t> &sizes) {
  sizes.assign(c->nranks, 0);
  if (c->nranks == 1) { sizes[0] = bytes; recv.assign((const char *)send, (const char *)send + bytes); return DM_OK; }
  if (c->rank == 0) {
    std::vector<std::vector<char>> blocks(c->nranks);
    sizes[0] = bytes;
    for (int r = 1; r < c->nranks; r++) {
      uint64_t n = 0;
      if (!sock_recv(c->fds[r], &n, 8)) return comm_fail(c, DM_ERR_HIP, "dm_comm: peer closed the connection");
      blocks[r].resize(n);
      if (n && !sock_recv(c->fds[r], blocks[r].data(), n)) return comm_fail(c, DM_ERR_HIP, "dm_comm: peer closed the connection");
      sizes[r] = n;
    }
    size_t total = 0;
    for (auto s : sizes) total += s;
    recv.resize(total);
    size_t o = 0;
    memcpy(recv.data(), send, bytes); o += bytes;
    for (int r = 1; r < c->nranks; r++) { if (sizes[r]) memcpy(recv.data() + o, blocks[r].data(), sizes[r]); o += sizes[r]; }
    for (int r = 1; r < c->nranks; r++)
      if (!sock_send(c->fds[r], sizes.data(), 8 * c->nranks) || (total && !sock_send(c->fds[r], recv.data(), total)))
        return comm_fail(c, DM_ERR_HIP, "dm_comm: peer closed the connection");
  } else {
    const uint64_t n = bytes;
    if (!sock_send(c->fds[0], &n, 8) || (bytes && !sock_send(c->fds[0], send, bytes))) return comm_fail(c, DM_ERR_HIP, "dm_comm: rank 0 closed the connection");
    if (!sock_recv(c->fds[0], sizes.data(), 8 * c->nranks)) return comm_fail(c, DM_ERR_HIP, "dm_comm: rank 0 closed the connection");
    size_t total = 0;
    for (auto s : sizes) total += s;
    recv.resize(total);
    if (total && !sock_recv(c->fds[0], recv.data(), total)) return comm_fail(c, DM_ERR_HIP, "dm_comm: rank 0 closed the connection");
  }
  return DM_OK;
}

static int comm_stage(dm_comm *c, size_t bytes) {
  if (c->stage_bytes >= bytes) return DM_OK;
  dm_release(c->d_stage); c->stage_bytes = 0;
  if (dm_alloc(nullptr, &c->d_stage, bytes + bytes / 2 + 256) != DM_OK) { c->err = g_create_err; return DM_ERR_HIP; }
  c->stage_bytes = bytes + bytes / 2 + 256;
  return DM_OK;
}

// ---- RCCL transport: var-size all-gather of DEVICE buffers = one broadcast per rank inside a group (all 7 xGMI links of a
// GPU carry a different peer's block at once; no ring).  sizes[] are known on every rank.
static int rccl_all_gather_v_dev(dm_comm *c, const void *d_send, void *d_recv, const std::vector<uint64_t> &sizes, hipStream_t st) {
  NCCLCHK(c, ncclGroupStart());
  size_t off = 0;
  for (int r = 0; r < c->nranks; r++) {
    if (sizes[r]) {
      ncclResult_t e = ncclBroadcast(r == c->rank ? d_send : (const void *)((char *)d_recv + off), (char *)d_recv + off, sizes[r], ncclChar, r, c->nccl, st);
      if (e != ncclSuccess) { (void)ncclGroupEnd(); return comm_fail(c, DM_ERR_HIP, std::string("ncclBroadcast failed: ") + ncclGetErrorString(e)); }
    }
    off += sizes[r];
  }
  NCCLCHK(c, ncclGroupEnd());
  return DM_OK;
}

// var-size all-gather of HOST buffers on either transport
static int comm_all_gather_v_host(dm_comm *c, const void *send, size_t bytes, std::vector<char> &recv, std::vector<uint64_t> &sizes) {
  if (c->kind == DM_COMM_HOST) return host_all_gather_v(c, send, bytes, recv, sizes);
  CHIPCHK(c, hipSetDevice(c->device));
  // sizes first (fixed 8 bytes per rank), then the payload
  int rc = comm_stage(c, 8 * (size_t)(c->nranks + 1));
  if (rc != DM_OK) return rc;
  uint64_t n = bytes;
  sizes.assign(c->nranks, 0);
  CHIPCHK(c, hipMemcpyAsync(c->d_stage, &n, 8, hipMemcpyHostToDevice, c->stream));
  NCCLCHK(c, ncclAllGather(c->d_stage, (char *)c->d_stage + 8, 8, ncclChar, c->nccl, c->stream));
  CHIPCHK(c, hipMemcpyAsync(sizes.data(), (char *)c->d_stage + 8, 8 * (size_t)c->nranks, hipMemcpyDeviceToHost, c->stream));
  CHIPCHK(c, hipStreamSynchronize(c->stream));
  size_t total = 0;
  for (auto s : sizes) total += s;
  recv.resize(total);
  if ((rc = comm_stage(c, total + bytes + 16)) != DM_OK) return rc;
  char *d_send = (char *)c->d_stage, *d_recv = d_send + ((bytes + 15) & ~(size_t)15);
  if (bytes) CHIPCHK(c, hipMemcpyAsync(d_send, send, bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = rccl_all_gather_v_dev(c, d_send, d_recv, sizes, c->stream)) != DM_OK) return rc;
  if (total) CHIPCHK(c, hipMemcpyAsync(recv.data(), d_recv, total, hipMemcpyDeviceToHost, c->stream));
  CHIPCHK(c, hipStreamSynchronize(c->stream));
  return DM_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI: communicators
const char *dm_comm_last_error(dm_comm_t c) { return c ? c->err.c_str() : g_comm_err.c_str(); }

int dm_comm_unique_id(void *id128) {
  if (!id128) return DM_ERR_INVALID;
  static_assert(sizeof(ncclUniqueId) <= DM_COMM_ID_BYTES, "ncclUniqueId does not fit DM_COMM_ID_BYTES");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) return comm_fail(nullptr, DM_ERR_HIP, std::string("ncclGetUniqueId failed: ") + ncclGetErrorString(r));
  memset(id128, 0, DM_COMM_ID_BYTES);
  memcpy(id128, &id, sizeof id);
  return DM_OK;
}

static int comm_init_rccl(dm_comm *c, const void *id128, int device_id) {
  c->kind = DM_COMM_RCCL; c->device = device_id;
  CHIPCHK(c, hipSetDevice(device_id));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  NCCLCHK(c, ncclCommInitRank(&c->nccl, c->nranks, id, c->rank));
  CHIPCHK(c, hipStreamCreate(&c->stream));
  return DM_OK;
}

int dm_comm_create_rccl(int nranks, int rank, const void *id128, int device_id, dm_comm_t *out) {
  if (!out || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return comm_fail(nullptr, DM_ERR_INVALID, "dm_comm_create_rccl: bad arguments");
  dm_comm *c = new dm_comm();
  c->nranks = nranks; c->rank = rank;
  int rc = comm_init_rccl(c, id128, device_id);
  if (rc != DM_OK) { g_comm_err = c->err; delete c; return rc; }
  *out = c;
  return DM_OK;
}

int dm_comm_create_tcp(int nranks, int rank, const char *addr, int port, int transport, int device_id, dm_comm_t *out) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks || port <= 0 || (transport != DM_COMM_HOST && transport != DM_COMM_RCCL))
    return comm_fail(nullptr, DM_ERR_INVALID, "dm_comm_create_tcp: bad arguments");
  dm_comm *c = new dm_comm();
  c->nranks = nranks; c->rank = rank; c->kind = DM_COMM_HOST; c->device = device_id;
  int rc = comm_rendezvous(c, addr, port);
  if (rc == DM_OK && transport == DM_COMM_RCCL) {
    // the sockets only carry the ncclUniqueId; all traffic afterwards is RCCL
    char id[DM_COMM_ID_BYTES];
    if (rank == 0) rc = dm_comm_unique_id(id);
    if (rc == DM_OK && nranks > 1) {
      if (rank == 0) { for (int r = 1; r < nranks; r++) if (!sock_send(c->fds[r], id, sizeof id)) rc = comm_fail(c, DM_ERR_HIP, "dm_comm: id broadcast failed"); }
      else if (!sock_recv(c->fds[0], id, sizeof id)) rc = comm_fail(c, DM_ERR_HIP, "dm_comm: id broadcast failed");
    }
    if (rc == DM_OK) rc = comm_init_rccl(c, id, device_id);
    comm_close_sockets(c);
  }
  if (rc != DM_OK) { g_comm_err = c->err.empty() ? g_comm_err : c->err; comm_close_sockets(c); delete c; return rc; }
  *out = c;
  return DM_OK;
}

// one process driving n GPUs (the shape of the reference: ONE JVM, N worker threads): ncclCommInitAll
int dm_comm_destroy(dm_comm_t c);
int dm_comm_create_all(int n, const int *devices, dm_comm_t *out) {
  if (!out || !devices || n < 1) return comm_fail(nullptr, DM_ERR_INVALID, "dm_comm_create_all: bad arguments");
  for (int i = 0; i < n; i++) {
    out[i] = nullptr;
    for (int j = 0; j < i; j++) if (devices[i] == devices[j]) return comm_fail(nullptr, DM_ERR_INVALID, "dm_comm_create_all: a device is listed twice (RCCL takes one rank per device)");
  }
  std::vector<ncclComm_t> comms(n);
  ncclResult_t r = ncclCommInitAll(comms.data(), n, devices);
  if (r != ncclSuccess) return comm_fail(nullptr, DM_ERR_HIP, std::string("ncclCommInitAll failed: ") + ncclGetErrorString(r));
  for (int i = 0; i < n; i++) {
    dm_comm *c = new dm_comm();
    c->nranks = n; c->rank = i; c->kind = DM_COMM_RCCL; c->device = devices[i]; c->nccl = comms[i];
    if (hipSetDevice(devices[i]) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) {
      c->stream = nullptr;
      (void)dm_comm_destroy(c);                                      // this rank's communicator ...
      for (int j = 0; j < i; j++) { (void)dm_comm_destroy(out[j]); out[j] = nullptr; }      // ... the ranks already wrapped ...
      for (int j = i + 1; j < n; j++) (void)ncclCommDestroy(comms[j]);                       // ... and the ones not wrapped yet
      return comm_fail(nullptr, DM_ERR_HIP, "dm_comm_create_all: stream creation failed");
    }
    out[i] = c;
  }
  return DM_OK;
}

int dm_comm_destroy(dm_comm_t c) {
  if (!c) return DM_ERR_INVALID;
  if (c->kind == DM_COMM_RCCL) {
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    dm_release(c->d_stage);
    if (c->nccl) (void)ncclCommDestroy(c->nccl);
  }
  comm_close_sockets(c);
  delete c;
  return DM_OK;
}

int dm_comm_rank(dm_comm_t c, int *rank, int *nranks, int *transport) {
  if (!c) return DM_ERR_INVALID;
  if (rank) *rank = c->rank;
  if (nranks) *nranks = c->nranks;
  if (transport) *transport = c->kind;
  return DM_OK;
}

int dm_comm_all_gather_v(dm_comm_t c, const void *send, size_t bytes, void *recv, size_t recv_cap, uint64_t *sizes) {
  if (!c || (bytes && !send) || !sizes) return DM_ERR_INVALID;
  std::vector<char> buf;
  std::vector<uint64_t> sz;
  int rc = comm_all_gather_v_host(c, send, bytes, buf, sz);
  if (rc != DM_OK) return rc;
  for (int r = 0; r < c->nranks; r++) sizes[r] = sz[r];
  if (!recv) return DM_OK;      // size query (the data is exchanged again by the next call)
  if (buf.size() > recv_cap) return comm_fail(c, DM_ERR_INVALID, "dm_comm_all_gather_v: receive buffer too small");
  if (!buf.empty()) memcpy(recv, buf.data(), buf.size());
  return DM_OK;
}

int dm_comm_allreduce_f64(dm_comm_t c, double *vals, int n, int op) {
  if (!c || !vals || n < 0 || (op != 0 && op != 1)) return DM_ERR_INVALID;
  std::vector<char> buf;
  std::vector<uint64_t> sz;
  int rc = comm_all_gather_v_host(c, vals, (size_t)n * 8, buf, sz);      // every rank reduces the same blocks in rank order
  if (rc != DM_OK) return rc;
  for (int r = 0; r < c->nranks; r++)
    if (sz[r] != (uint64_t)n * 8) return comm_fail(c, DM_ERR_INVALID, "dm_comm_allreduce_f64: ranks disagree on the number of values");
  const double *all = (const double *)buf.data();
  for (int i = 0; i < n; i++) {
    double a = all[i];
    for (int r = 1; r < c->nranks; r++) { const double v = all[(size_t)r * n + i]; a = op == 0 ? a + v : (v > a ? v : a); }
    vals[i] = a;
  }
  return DM_OK;
}

// Every rank enters with its own status; all leave with the same one: DM_OK only if every rank was fine.  Called BEFORE a data-path
// collective so that a rank-local failure (an allocation, a validation error, a refused shape) cannot leave the peers blocked inside
// RCCL / a socket read (round-4 advisor finding).  A rank that fails anywhere between two agreement points calls this once with its
// error and returns; the peers learn it at their next point.
static int comm_agree(dm_ctx *h, dm_comm *c, int rc, const char *who) {
  if (!c || c->nranks <= 1) return rc;
  double bad = rc != DM_OK ? 1.0 : 0.0;
  const int rc2 = dm_comm_allreduce_f64(c, &bad, 1, 0);
  if (rc != DM_OK) return rc;
  if (rc2 != DM_OK) return fail(h, rc2, c->err);
  if (bad > 0) return fail(h, DM_ERR_STATE, std::string(who) + ": a peer rank failed; this rank left the collective step with it");
  return DM_OK;
}

int dm_comm_barrier(dm_comm_t c) {
  double z = 0;
  return dm_comm_allreduce_f64(c, &z, 1, 0);
}

int dm_comm_attach(dm_handle_t h, dm_comm_t c) {
  if (!h) return DM_ERR_INVALID;
  if (c && c->kind == DM_COMM_RCCL && c->device != h->device) return fail(h, DM_ERR_INVALID, "dm_comm_attach: the communicator was created for another device");
  h->comm = c;
  return DM_OK;
}

// ------------------------------------------------------------------------------------------------ gradient exchange
template <typename T>
__global__ void dm_zero_rows_kernel(T *grad, const int32_t *list, int64_t n, int E) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * E; t += (int64_t)gridDim.x * blockDim.x)
    grad[(int64_t)list[t / E] * E + (t % E)] = (T)0;
}
template <typename T>
__global__ void dm_sum_blocks_kernel(T *out, const T *blocks, int64_t n, int nblocks) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    T a = blocks[t];
    for (int r = 1; r < nblocks; r++) a += blocks[(int64_t)r * n + t];      // rank order on every replica
    out[t] = a;
  }
}
// {touched rows, list did not overflow} of this rank: the 16-byte record the ranks all-gather before sizing the exchange
__global__ void dm_sync_record_kernel(const unsigned long long *cnt, unsigned long long cap, unsigned long long *rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { rec[0] = *cnt; rec[1] = *cnt <= cap ? 1ull : 0ull; }
}

static int sync_grow(dm_ctx *h, size_t bytes) {
  return h->sync.reserve(h, bytes, bytes / 4 + 256);
}

// what the last exchange moved (bench.py prints it) lives in the handle (dm_ctx::sync_stats: the reference's shape is N worker threads
// in one process, each driving its own handle — a process-global record would race); the clique call files it under every handle

// syncGradients for the workers hs[0..nh): nh == 1 is the usual one-process-per-GPU case (peers are other processes, reached
// through the attached communicator); nh > 1 drives all ranks of an in-process RCCL clique from one thread with group calls.
//
// RCCL transport, per step: (1) ncclAllGather of the 16-byte {count, ok} records on the stream, ONE read-back + host sync (the
// exchange has to be sized on the host); (2) one ncclAllReduce(sum) of the dense block and ONE ncclAllGather of max-padded
// [row ids | gradient rows] blocks; (3) every rank zeroes the rows it touched and re-adds all ranks' rows in rank order, so the
// touched embedding rows carry the same bits on every replica.  The dense sum is RCCL's (ring / tree order, identical on all
// ranks but not the rank-ordered sum of the host transport).  A rank whose touch list overflowed reports ok = 0 in (1), so all
// ranks fail together instead of one of them leaving the others inside a collective.
static int sync_gradients_impl(dm_ctx **hs, int nh) {
  dm_ctx *h0 = hs[0];
  dm_comm *c0 = h0->comm;
  if (!c0) return fail(h0, DM_ERR_STATE, "dm_train_sync_gradients: no communicator attached (dm_comm_attach)");
  const int W = c0->nranks;
  if (nh > 1) {
    if (nh != W) return fail(h0, DM_ERR_INVALID, "dm_allreduce_grads: the handle list must cover every rank of the communicator");
    for (int i = 0; i < nh; i++) {
      if (!hs[i]->comm || hs[i]->comm->kind != DM_COMM_RCCL || hs[i]->comm->nranks != W || hs[i]->comm->rank != i)
        return fail(h0, DM_ERR_INVALID, "dm_allreduce_grads: handle i must carry rank i of one dm_comm_create_all clique");
      if (hs[i]->embed != h0->embed || hs[i]->num_index != h0->num_index || hs[i]->dtype != h0->dtype)
        return fail(h0, DM_ERR_INVALID, "dm_allreduce_grads: replicas differ in shape");
    }
  }
  for (int i = 0; i < nh; i++) { int rc = train_check(hs[i], "dm_train_sync_gradients"); if (rc != DM_OK) return rc; }
  dm_sync_stats &S = h0->sync_stats;
  S = dm_sync_stats{};
  S.nranks = W; S.transport = c0->kind;
  struct Share { dm_ctx **hs; int nh; ~Share() { for (int i = 1; i < nh; i++) hs[i]->sync_stats = hs[0]->sync_stats; } } share_{hs, nh};
  if (W == 1) return DM_OK;
  const int64_t E = h0->embed;
  const int64_t nd = 3 * E * E + 2 * E + 1;
  const bool f64 = h0->dtype == DM_F64;
  const size_t es = f64 ? 8 : 4;
  const ncclDataType_t nty = f64 ? ncclDouble : ncclFloat;
  // ---- (1) touched-row counts of every rank
  std::vector<uint64_t> cnt(W, 0), okf(W, 1);
  if (c0->kind == DM_COMM_RCCL) {
    std::vector<std::vector<unsigned long long>> rec(nh, std::vector<unsigned long long>(2 * (size_t)W));
    for (int i = 0; i < nh; i++) {
      dm_ctx *h = hs[i];
      HIPCHK(h, hipSetDevice(h->device));
      int rc = sync_grow(h, 16 + 16 * (size_t)W);
      if (rc != DM_OK) return rc;
      if ((rc = LAUNCH(h, dm_sync_record_kernel, dim3(1), dim3(64), 0, h->d_touch_cnt, h->touch_cap, (unsigned long long *)h->sync.p)) != DM_OK) return rc;
    }
    ncclResult_t e = ncclGroupStart();
    for (int i = 0; i < nh && e == ncclSuccess; i++)
      e = ncclAllGather(hs[i]->sync.p, (char *)hs[i]->sync.p + 16, 2, ncclUint64, hs[i]->comm->nccl, hs[i]->stream);
    ncclResult_t e2 = ncclGroupEnd();
    if (e != ncclSuccess || e2 != ncclSuccess)
      return fail(h0, DM_ERR_HIP, std::string("dm_train_sync_gradients: RCCL count exchange failed: ") + ncclGetErrorString(e != ncclSuccess ? e : e2));
    for (int i = 0; i < nh; i++) {
      HIPCHK(hs[i], hipSetDevice(hs[i]->device));
      HIPCHK(hs[i], hipMemcpyAsync(rec[i].data(), (char *)hs[i]->sync.p + 16, 16 * (size_t)W, hipMemcpyDeviceToHost, hs[i]->stream));
    }
    for (int i = 0; i < nh; i++) { HIPCHK(hs[i], hipSetDevice(hs[i]->device)); HIPCHK(hs[i], hipStreamSynchronize(hs[i]->stream)); }
    S.host_syncs++;
    for (int r = 0; r < W; r++) { cnt[r] = rec[0][2 * r]; okf[r] = rec[0][2 * r + 1]; }
  } else {
    dm_ctx *h = h0;
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long k = 0;
    HIPCHK(h, hipMemcpyAsync(&k, h->d_touch_cnt, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    S.host_syncs++;
    const uint64_t mine2[2] = {k, k <= h->touch_cap ? 1ull : 0ull};
    std::vector<char> buf; std::vector<uint64_t> sz;
    int rc = comm_all_gather_v_host(c0, mine2, 16, buf, sz);
    if (rc != DM_OK) return fail(h0, rc, c0->err);
    for (int r = 0; r < W; r++) {
      if (sz[r] != 16) return fail(h0, DM_ERR_STATE, "dm_train_sync_gradients: peers disagree on the record size");
      uint64_t v[2]; memcpy(v, buf.data() + 16 * (size_t)r, 16);
      cnt[r] = v[0]; okf[r] = v[1];
    }
  }
  for (int r = 0; r < W; r++)
    if (!okf[r]) return fail(h0, DM_ERR_STATE, "dm_train_sync_gradients: touched-row list overflow on rank " + std::to_string(r) + " (every rank aborts the exchange)");
  uint64_t total = 0, maxc = 0;
  for (auto k : cnt) { total += k; maxc = k > maxc ? k : maxc; }
  S.rows_total = total;
  // ---- per handle staging.  RCCL: [record area 256 B | own block | W blocks], block = [maxc row ids (padded to 256 B) | maxc x E
  // gradient elements]; HOST: [own rows | own grads | all rows | all grads | W dense blocks]
  const size_t blk_rows = DevArena::up(maxc * 4), blk = blk_rows + DevArena::up(maxc * E * es);
  struct Lay { char *mine; char *all; int32_t *my_rows; void *my_grads; int32_t *all_rows; char *all_grads; char *dense_all; };
  std::vector<Lay> lay(nh);
  for (int i = 0; i < nh; i++) {
    dm_ctx *h = hs[i];
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t mine = cnt[h->comm->rank];
    const size_t need = c0->kind == DM_COMM_RCCL ? 256 + 16 * (size_t)W + (size_t)(W + 1) * blk
                                                 : DevArena::up(mine * 4) + DevArena::up(mine * E * es) + DevArena::up(total * 4) + DevArena::up(total * E * es) + DevArena::up((size_t)W * nd * es);
    int rc = sync_grow(h, need);
    if (rc != DM_OK) return rc;
    char *w = (char *)h->sync.p;
    if (c0->kind == DM_COMM_RCCL) {
      w += DevArena::up(16 + 16 * (size_t)W);
      lay[i].mine = w; lay[i].all = w + blk;
      lay[i].my_rows = (int32_t *)lay[i].mine; lay[i].my_grads = lay[i].mine + blk_rows;
    } else {
      lay[i].my_rows = (int32_t *)w; w += DevArena::up(mine * 4);
      lay[i].my_grads = w; w += DevArena::up(mine * E * es);
      lay[i].all_rows = (int32_t *)w; w += DevArena::up(total * 4);
      lay[i].all_grads = w; w += DevArena::up(total * E * es);
      lay[i].dense_all = w;
    }
    if (mine) { rc = launch_gather_rows(h, (int64_t)mine, lay[i].my_rows, lay[i].my_grads); if (rc != DM_OK) return rc; }
    if (h->comm->rank == c0->rank) S.rows_mine = mine;
  }
  // ---- (2) exchange
  if (c0->kind == DM_COMM_RCCL) {
    ncclResult_t e = ncclGroupStart();
    for (int i = 0; i < nh && e == ncclSuccess; i++) {
      dm_ctx *h = hs[i];
      char *dense = (char *)h->train.grad + (size_t)(h->num_index * E) * es;
      e = ncclAllReduce(dense, dense, (size_t)nd, nty, ncclSum, h->comm->nccl, h->stream);
      if (e == ncclSuccess && maxc) e = ncclAllGather(lay[i].mine, lay[i].all, blk, ncclChar, h->comm->nccl, h->stream);
    }
    ncclResult_t e2 = ncclGroupEnd();
    if (e != ncclSuccess || e2 != ncclSuccess)
      return fail(h0, DM_ERR_HIP, std::string("dm_train_sync_gradients: RCCL exchange failed: ") + ncclGetErrorString(e != ncclSuccess ? e : e2));
    S.bytes_sent = (uint64_t)nd * es + blk; S.bytes_recv = (uint64_t)nd * es + (uint64_t)W * blk;
  } else {
    // HOST transport (nh == 1): stage through host memory; the dense block is summed in rank order by every replica
    dm_ctx *h = h0;
    const uint64_t mine = cnt[c0->rank];
    std::vector<char> sendbuf((size_t)nd * es + mine * 4 + mine * E * es), recv;
    std::vector<uint64_t> sz;
    HIPCHK(h, hipMemcpyAsync(sendbuf.data(), (char *)h->train.grad + (size_t)(h->num_index * E) * es, (size_t)nd * es, hipMemcpyDeviceToHost, h->stream));
    if (mine) {
      HIPCHK(h, hipMemcpyAsync(sendbuf.data() + nd * es, lay[0].my_rows, mine * 4, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(sendbuf.data() + nd * es + mine * 4, lay[0].my_grads, mine * E * es, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    S.host_syncs++;
    int rc = comm_all_gather_v_host(c0, sendbuf.data(), sendbuf.size(), recv, sz);
    if (rc != DM_OK) return fail(h, rc, c0->err);
    size_t off = 0, ro = 0, go = 0;
    for (int r = 0; r < W; r++) {
      if (sz[r] != (uint64_t)nd * es + cnt[r] * 4 + cnt[r] * E * es) return fail(h, DM_ERR_STATE, "dm_train_sync_gradients: peers disagree on the block sizes");
      HIPCHK(h, hipMemcpyAsync(lay[0].dense_all + (size_t)r * nd * es, recv.data() + off, (size_t)nd * es, hipMemcpyHostToDevice, h->stream));
      if (cnt[r]) {
        HIPCHK(h, hipMemcpyAsync(lay[0].all_rows + ro, recv.data() + off + nd * es, cnt[r] * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(lay[0].all_grads + go * es, recv.data() + off + nd * es + cnt[r] * 4, cnt[r] * E * es, hipMemcpyHostToDevice, h->stream));
      }
      off += sz[r]; ro += cnt[r]; go += cnt[r] * E;
    }
    S.bytes_sent = sendbuf.size(); S.bytes_recv = off;
    char *dense = (char *)h->train.grad + (size_t)(h->num_index * E) * es;
    const int rc_s = f64 ? LAUNCH(h, dm_sum_blocks_kernel<double>, dim3(64), dim3(256), 0, (double *)dense, (const double *)lay[0].dense_all, nd, W)
                         : LAUNCH(h, dm_sum_blocks_kernel<float>, dim3(64), dim3(256), 0, (float *)dense, (const float *)lay[0].dense_all, nd, W);
    if (rc_s != DM_OK) return rc_s;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // recv is read by the copies above
    S.host_syncs++;
  }
  // ---- (3) every replica rebuilds each touched row as 0 + g_0 + g_1 + ... in rank order (same bits everywhere)
  for (int i = 0; i < nh; i++) {
    dm_ctx *h = hs[i];
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t mine = cnt[h->comm->rank];
    if (mine) {
      const int rc_z = f64 ? LAUNCH(h, dm_zero_rows_kernel<double>, dim3(1024), dim3(256), 0, (double *)h->train.grad, h->d_touch_list, mine, E)
                           : LAUNCH(h, dm_zero_rows_kernel<float>, dim3(1024), dim3(256), 0, (float *)h->train.grad, h->d_touch_list, mine, E);
      if (rc_z != DM_OK) return rc_z;
    }
    size_t ro = 0, go = 0;
    for (int r = 0; r < W; r++) {
      if (cnt[r]) {
        const int32_t *rows = c0->kind == DM_COMM_RCCL ? (const int32_t *)(lay[i].all + (size_t)r * blk) : lay[i].all_rows + ro;
        const void *grads = c0->kind == DM_COMM_RCCL ? (const void *)(lay[i].all + (size_t)r * blk + blk_rows) : (const void *)(lay[i].all_grads + go * es);
        int rc = launch_add_rows(h, rows, grads, (int64_t)cnt[r]);
        if (rc != DM_OK) return rc;
      }
      ro += cnt[r]; go += cnt[r] * E;
    }
  }
  for (int i = 0; i < nh; i++) { HIPCHK(hs[i], hipSetDevice(hs[i]->device)); HIPCHK(hs[i], hipStreamSynchronize(hs[i]->stream)); }
  S.host_syncs++;
  return DM_OK;
}

// what the last dm_train_sync_gradients / dm_allreduce_grads on this handle moved: out[0..7] = nranks, transport, touched rows of
// this rank, touched rows of all ranks, bytes sent, bytes received, host synchronisations, 0
int dm_train_sync_stats(dm_handle_t h, uint64_t *out8) {
  if (!h || !out8) return DM_ERR_INVALID;
  const dm_sync_stats &S = h->sync_stats;
  out8[0] = (uint64_t)S.nranks; out8[1] = (uint64_t)S.transport; out8[2] = S.rows_mine;
  out8[3] = S.rows_total; out8[4] = S.bytes_sent; out8[5] = S.bytes_recv;
  out8[6] = (uint64_t)S.host_syncs; out8[7] = 0;
  return DM_OK;
}

int dm_train_sync_gradients(dm_handle_t h) {
  if (!h) return DM_ERR_INVALID;
  DM_DIN_ONLY(h, "dm_train_sync_gradients");
  dm_ctx *one[1] = {h};
  return sync_gradients_impl(one, 1);
}

int dm_allreduce_grads(dm_handle_t *hs, int n) {
  if (!hs || n < 1) return DM_ERR_INVALID;
  for (int i = 0; i < n; i++) if (!hs[i]) return DM_ERR_INVALID;
  return sync_gradients_impl(hs, n);
}

// The payload half of dm_comm_all_gather_dev, for a caller that already knows every rank's size (all[r], total = their sum): the only
// transport-specific code of a device all-gather.  Ordered after the work queued on the handle's stream and complete on return; d_send
// may be this rank's place inside d_recv.  *syncs (optional) += the times the host waited for the stream.
static int comm_all_gather_dev_payload(dm_ctx *h, dm_comm *c, const void *d_send, size_t bytes, void *d_recv, const std::vector<uint64_t> &all, size_t total, int *syncs) {
  int rc;
  if (c->kind == DM_COMM_RCCL) {
    rc = rccl_all_gather_v_dev(c, d_send, d_recv, all, h->stream);
    if (rc != DM_OK) return fail(h, rc, c->err);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (syncs) *syncs += 1;
    return DM_OK;
  }
  std::vector<char> sendbuf(bytes), recv;
  std::vector<uint64_t> sz;
  if (bytes) HIPCHK(h, hipMemcpyAsync(sendbuf.data(), d_send, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (syncs) *syncs += 1;
  rc = comm_all_gather_v_host(c, sendbuf.data(), bytes, recv, sz);
  if (rc != DM_OK) return fail(h, rc, c->err);
  if (recv.size() != total) return fail(h, DM_ERR_STATE, "dm_comm_all_gather_dev: the blocks received do not add up to the announced sizes");
  if (total) HIPCHK(h, hipMemcpyAsync(d_recv, recv.data(), total, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));      // recv is read by the copy
  if (syncs) *syncs += 1;
  return DM_OK;
}

// var-size all-gather of DEVICE buffers on the handle's stream (JTM weight blocks, result lists): d_recv receives the blocks
// in rank order; sizes[r] (host) are filled for every rank.  d_recv == NULL: size query only.
int dm_comm_all_gather_dev(dm_handle_t h, const void *d_send, size_t bytes, void *d_recv, size_t recv_cap, uint64_t *sizes) {
  if (!h || !sizes) return DM_ERR_INVALID;
  dm_comm *c = h->comm;
  if (!c) return fail(h, DM_ERR_STATE, "dm_comm_all_gather_dev: no communicator attached");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<char> buf; std::vector<uint64_t> sz;
  const uint64_t mine = bytes;
  int rc = comm_all_gather_v_host(c, &mine, 8, buf, sz);
  if (rc != DM_OK) return fail(h, rc, c->err);
  std::vector<uint64_t> all(c->nranks);
  memcpy(all.data(), buf.data(), 8 * (size_t)c->nranks);
  size_t total = 0;
  for (int r = 0; r < c->nranks; r++) { sizes[r] = all[r]; total += all[r]; }
  if (!d_recv) return DM_OK;
  if (total > recv_cap) return fail(h, DM_ERR_INVALID, "dm_comm_all_gather_dev: receive buffer too small");
  return comm_all_gather_dev_payload(h, c, d_send, bytes, d_recv, all, total, nullptr);
}
