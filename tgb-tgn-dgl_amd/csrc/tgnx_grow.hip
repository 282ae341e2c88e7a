// Node-space growth of the TGN engine on gfx950: move everything sized by num_nodes into larger
// allocations, so that the result is bit for bit the state of an engine built at the larger node count.
//
// Two kernels, both plain copies with a device-side check:
//   grow_rows    ONE launch walks every row-major [N, .] tensor the caller passed (ring nbr / eid / t, assoc, memory,
//                last_update, node_gen): bytes [0, old) are copied, bytes [old, new) take the tensor's reset word
//                (nbr / eid: -1, ring t: -1.0f, the rest 0).  The unit is a 16-byte piece (uint4 load / store); the one
//                piece per tensor that straddles the old end, the tail of a byte count that is no multiple of 16, and a
//                tensor whose pointers are not 16-B aligned go word by word (every element size is a multiple of 4)
//   grow_store   the message store [4 * N node-table words | arena] into [4 * n_new | arena].  Run offsets are
//                arena-relative (tgnx_tgn.hip: c.arena + s.so), so the arena moves as a block, 16 bytes per thread and
//                round, and no run is rewritten.  Every node's two runs {off, cnt} are checked against the arena on
//                the way (cnt < 0, or a non-empty run outside [0, 2 * num_events)): counted into *bad, never followed
//   No workspace, no float arithmetic, no atomics on data: the result does not depend on the launch shape.
#include <algorithm>

#include "tgnx_common.h"

using namespace tgnx;

namespace {

constexpr int GT = 256;              // workgroup size
constexpr int64_t MAX_GRID = 2048;   // grid-stride kernels: 8 workgroups per CU cover the 256 CUs
constexpr int NROW = 7;              // row-major tensors of one engine

struct RowJob {
  const char* src;
  char* dst;
  int64_t old_bytes, new_bytes;   // both multiples of 4
  int64_t piece0;                 // first 16-byte piece of this tensor in the launch's piece numbering
  uint32_t fill;                  // the reset value's 32-bit pattern (every reset element repeats one)
  int vec;                        // both pointers 16-B aligned
};

struct RowJobs {
  RowJob j[NROW];
  int n;
  int64_t pieces;
};

__global__ void __launch_bounds__(GT) grow_rows(RowJobs J) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = tid; p < J.pieces; p += nt) {
#pragma unroll
    for (int i = 0; i < NROW; ++i) {   // (static indices: the jobs stay in the kernel arguments; unused jobs are empty)
      const RowJob& r = J.j[i];
      const int64_t end = i + 1 < NROW ? J.j[i + 1].piece0 : J.pieces;
      if (p < r.piece0 || p >= end) continue;
      const int64_t lo = (p - r.piece0) * 16, hi = lo + 16;
      if (r.vec && hi <= r.old_bytes) {
        *reinterpret_cast<uint4*>(r.dst + lo) = *reinterpret_cast<const uint4*>(r.src + lo);
      } else if (r.vec && lo >= r.old_bytes && hi <= r.new_bytes) {
        *reinterpret_cast<uint4*>(r.dst + lo) = make_uint4(r.fill, r.fill, r.fill, r.fill);
      } else {
        for (int64_t b = lo; b < hi && b < r.new_bytes; b += 4)
          *reinterpret_cast<uint32_t*>(r.dst + b) =
              b < r.old_bytes ? *reinterpret_cast<const uint32_t*>(r.src + b) : r.fill;
      }
    }
  }
}

// node-table rows are 32 bytes and the arena starts at a multiple of 32 bytes in both stores: uint4 throughout when
// both store pointers are 16-B aligned, int64 words otherwise
__global__ void __launch_bounds__(GT) grow_store(const int64_t* __restrict__ st, int64_t N, int64_t n_new, int64_t nev,
                                                 int64_t* __restrict__ nst, int vec,
                                                 unsigned long long* __restrict__ bad) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t lim = 2 * nev;
  unsigned long long nbad = 0;
  for (int64_t v = tid; v < n_new; v += nt) {
    int64_t w[4] = {0, 0, 0, 0};
    if (v < N) {
      if (vec) {
        const uint4 a = reinterpret_cast<const uint4*>(st)[2 * v], b = reinterpret_cast<const uint4*>(st)[2 * v + 1];
        w[0] = (int64_t)(((uint64_t)a.y << 32) | a.x);
        w[1] = (int64_t)(((uint64_t)a.w << 32) | a.z);
        w[2] = (int64_t)(((uint64_t)b.y << 32) | b.x);
        w[3] = (int64_t)(((uint64_t)b.w << 32) | b.z);
      } else {
        for (int i = 0; i < 4; ++i) w[i] = st[4 * v + i];
      }
      for (int dir = 0; dir < 2; ++dir) {
        const int64_t off = w[2 * dir], cnt = w[2 * dir + 1];
        if (cnt < 0 || (cnt > 0 && (off < 0 || cnt > lim || off > lim - cnt))) ++nbad;
      }
    }
    if (vec) {
      reinterpret_cast<uint4*>(nst)[2 * v] =
          make_uint4((uint32_t)w[0], (uint32_t)((uint64_t)w[0] >> 32), (uint32_t)w[1], (uint32_t)((uint64_t)w[1] >> 32));
      reinterpret_cast<uint4*>(nst)[2 * v + 1] =
          make_uint4((uint32_t)w[2], (uint32_t)((uint64_t)w[2] >> 32), (uint32_t)w[3], (uint32_t)((uint64_t)w[3] >> 32));
    } else {
      for (int i = 0; i < 4; ++i) nst[4 * v + i] = w[i];
    }
  }
  const int64_t* arena = st + 4 * N;
  int64_t* narena = nst + 4 * n_new;
  if (vec) {   // 2 * nev int64 = nev pieces of 16 bytes
    for (int64_t p = tid; p < nev; p += nt) reinterpret_cast<uint4*>(narena)[p] = reinterpret_cast<const uint4*>(arena)[p];
  } else {
    for (int64_t p = tid; p < lim; p += nt) narena[p] = arena[p];
  }
  if (nbad) atomicAdd(bad, nbad);
}

unsigned grid_for(int64_t work_items) {
  return (unsigned)std::min<int64_t>(MAX_GRID, std::max<int64_t>(1, (work_items + GT - 1) / GT));
}

bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

int check_common(const char* who, const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* b, int64_t n_new, const void* bad) {
  TGNX_CHECK_ARG(cfg && b && bad, "%s: null config / buffers / bad counter", who);
  TGNX_CHECK_ARG(cfg->num_nodes > 0 && cfg->ring > 0 && cfg->mem_dim > 0 && cfg->num_events > 0,
                 "%s: bad num_nodes / ring / mem_dim / num_events", who);
  TGNX_CHECK_ARG(n_new >= cfg->num_nodes, "%s: n_new = %lld below num_nodes = %lld (nodes are never dropped)", who,
                 (long long)n_new, (long long)cfg->num_nodes);
  if (n_new >= (1ll << 31)) {
    set_error("%s: n_new = %lld: node ids are below 2^31", who, (long long)n_new);
    return TGNX_ETOOBIG;
  }
  TGNX_CHECK_ARG((reinterpret_cast<uintptr_t>(bad) & 7) == 0, "%s: the bad counter must be 8-B aligned", who);
  return TGNX_OK;
}

int check_store(const char* who, const int64_t* st, const int64_t* nst) {
  TGNX_CHECK_ARG(st && nst && st != nst, "%s: null store / new store (or the same one)", who);
  TGNX_CHECK_ARG(((reinterpret_cast<uintptr_t>(st) | reinterpret_cast<uintptr_t>(nst)) & 7) == 0,
                 "%s: stores must be 8-B aligned", who);
  return TGNX_OK;
}

int launch_store(const tgnx_tgn_config* cfg, const int64_t* st, int64_t n_new, int64_t* nst, int64_t* bad,
                 hipStream_t s) {
  const int64_t N = cfg->num_nodes, nev = cfg->num_events;
  grow_store<<<grid_for(std::max(n_new, nev)), GT, 0, s>>>(st, N, n_new, nev, nst, aligned16(st, nst) ? 1 : 0,
                                                           reinterpret_cast<unsigned long long*>(bad));
  TGNX_LAUNCH_CHECK("grow_store");
  return TGNX_OK;
}

}  // namespace

extern "C" {

int tgnx_tgn_grow_store(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t n_new, int64_t* new_store,
                        int64_t* bad, void* stream) {
  const char* who = "tgnx_tgn_grow_store";
  int rc = check_common(who, cfg, buf, n_new, bad);
  if (rc) return rc;
  rc = check_store(who, buf->store, new_store);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  TGNX_HIP_CHECK(hipMemsetAsync(bad, 0, 8, s));
  return launch_store(cfg, buf->store, n_new, new_store, bad, s);
}

int tgnx_tgn_grow_nodes(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t n_new, int64_t row_capacity,
                        const tgnx_tgn_grow_out* out, int64_t* bad, void* stream) {
  const char* who = "tgnx_tgn_grow_nodes";
  int rc = check_common(who, cfg, buf, n_new, bad);
  if (rc) return rc;
  TGNX_CHECK_ARG(out, "%s: null output block", who);
  TGNX_CHECK_ARG(row_capacity >= n_new, "%s: row_capacity = %lld below n_new = %lld", who, (long long)row_capacity,
                 (long long)n_new);
  if (row_capacity >= (1ll << 31)) {
    set_error("%s: row_capacity = %lld: node ids are below 2^31", who, (long long)row_capacity);
    return TGNX_ETOOBIG;
  }
  const int64_t N = cfg->num_nodes, K = cfg->ring, D = cfg->mem_dim;
  const struct {
    const void* src;
    void* dst;
    int64_t row_bytes;
    uint32_t fill;
    const char* name;
  } T[NROW] = {{buf->nbr, out->nbr, K * 8, 0xFFFFFFFFu, "nbr"},          {buf->eid, out->eid, K * 8, 0xFFFFFFFFu, "eid"},
               {buf->rt, out->rt, K * 4, 0xBF800000u, "rt"},             {buf->assoc, out->assoc, 8, 0u, "assoc"},
               {buf->memory, out->memory, D * 4, 0u, "memory"},          {buf->last_update, out->last_update, 8, 0u, "last_update"},
               {buf->node_gen, out->node_gen, 4, 0u, "node_gen"}};
  RowJobs J;
  J.n = 0;
  J.pieces = 0;
  for (int i = 0; i < NROW; ++i) {
    if (!T[i].src && !T[i].dst) continue;   // (a loader or a model grown on its own passes its tensors only)
    TGNX_CHECK_ARG(T[i].src && T[i].dst && T[i].src != T[i].dst, "%s: %s needs both its old and its new allocation", who,
                   T[i].name);
    TGNX_CHECK_ARG(((reinterpret_cast<uintptr_t>(T[i].src) | reinterpret_cast<uintptr_t>(T[i].dst)) & 3) == 0,
                   "%s: %s must be 4-B aligned", who, T[i].name);
    RowJob& r = J.j[J.n++];
    r.src = reinterpret_cast<const char*>(T[i].src);
    r.dst = reinterpret_cast<char*>(T[i].dst);
    r.old_bytes = N * T[i].row_bytes;
    r.new_bytes = row_capacity * T[i].row_bytes;
    r.piece0 = J.pieces;
    r.fill = T[i].fill;
    r.vec = aligned16(T[i].src, T[i].dst) ? 1 : 0;
    J.pieces += (r.new_bytes + 15) / 16;
  }
  const bool store = buf->store || out->store;
  TGNX_CHECK_ARG(J.n > 0 || store, "%s: nothing to grow (every tensor null)", who);
  for (int i = J.n; i < NROW; ++i) J.j[i] = RowJob{nullptr, nullptr, 0, 0, J.pieces, 0u, 0};
  hipStream_t s = as_stream(stream);
  if (store) {   // (checked before the first launch: a refused call launches nothing)
    rc = check_store(who, buf->store, out->store);
    if (rc) return rc;
  }
  TGNX_HIP_CHECK(hipMemsetAsync(bad, 0, 8, s));
  if (J.n > 0) {
    grow_rows<<<grid_for(J.pieces), GT, 0, s>>>(J);
    TGNX_LAUNCH_CHECK("grow_rows");
  }
  if (store) return launch_store(cfg, buf->store, n_new, out->store, bad, s);
  return TGNX_OK;
}

}  // extern "C"
