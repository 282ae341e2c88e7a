// Live (source, destination) pair set: an open-addressing hash table in device memory, for gfx950.
// DESIGN §3b-14 has the contract; tests/pairset_ref.py restates it as a dict.
//
// Table (one allocation of tgnx_pairset_bytes(capacity) = 20 * capacity bytes, capacity a power of two >= 64):
//   key     uint64[capacity]   (uint64)src << 32 | dst; all ones = EMPTY
//   count   uint32[capacity]   occurrences                                      identity 0
//   t_first uint32[capacity]   smallest stamp, as an order-preserving uint32    identity 0xFFFFFFFF
//   t_last  uint32[capacity]   largest stamp, likewise                          identity 0
// Home slot = (key * 0x9E3779B97F4A7C15) >> (64 - log2(capacity)); probing is linear and wraps.
//
// Every value update of a present key is a commutative integer atomic (add / min / max) and the value fields hold
// their identities before a key is published, so a thread that finds a key another thread has just claimed updates
// it without a handshake, and the contents are a function of the multiset of inserted events.  The slot layout is
// not (it depends on which thread claims first); no entry point's output depends on it, except the order of
// tgnx_pairset_export's rows, which the caller sorts.
//
// Every loop is bounded: a probe visits at most `capacity` slots, the claim is one 64-bit compare-and-swap per
// visited slot (never a spin), and an event that finds no slot is counted in status[2] and dropped.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "tgnx_common.h"

namespace tgnx {
namespace pairset {

constexpr int T = 256;
constexpr int64_t MAX_GRID = 1 << 16;
constexpr uint64_t EMPTY = ~0ull;
constexpr uint64_t FIB = 0x9E3779B97F4A7C15ull;
constexpr uint32_t TF_ID = 0xFFFFFFFFu, TL_ID = 0u;
constexpr int SEL_ITERS = 4;                 // a select block covers SEL_ITERS * T candidates of one source
constexpr int64_t SEL_CHUNK = SEL_ITERS * T;

struct Table {
  uint64_t* key;
  uint32_t *count, *t_first, *t_last;
  int64_t cap;
  int log2cap;
};

static Table view(void* table, int64_t cap) {
  Table t;
  unsigned char* p = static_cast<unsigned char*>(table);
  t.key = reinterpret_cast<uint64_t*>(p);
  t.count = reinterpret_cast<uint32_t*>(p + 8 * cap);
  t.t_first = t.count + cap;
  t.t_last = t.t_first + cap;
  t.cap = cap;
  t.log2cap = 0;
  while ((int64_t(1) << t.log2cap) < cap) ++t.log2cap;
  return t;
}

static bool cap_ok(int64_t cap) { return cap >= 64 && cap <= (int64_t(1) << 40) && (cap & (cap - 1)) == 0; }
static bool nodes_ok(int64_t N) { return N > 0 && N <= (int64_t(1) << 32) - 1; }  // (2^32 - 1, 2^32 - 1) would be EMPTY
static unsigned grid_for(int64_t items) {
  return (unsigned)std::min<int64_t>(MAX_GRID, std::max<int64_t>(1, (items + T - 1) / T));
}

// float32 stamp -> uint32 with the same order (-0.0 is stored as 0.0, so integer and float order agree everywhere)
__device__ __forceinline__ uint32_t t_enc(float t) {
  uint32_t b = __float_as_uint(t);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float t_dec(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ int64_t home(uint64_t key, int log2cap) { return (int64_t)((key * FIB) >> (64 - log2cap)); }

// slot of `key`, or -1: stops at the first EMPTY slot or after `cap` slots
__device__ __forceinline__ int64_t find(const Table& tb, uint64_t key) {
  int64_t slot = home(key, tb.log2cap);
  for (int64_t i = 0; i < tb.cap; ++i) {
    const uint64_t k = tb.key[slot];
    if (k == key) return slot;
    if (k == EMPTY) return -1;
    slot = (slot + 1) & (tb.cap - 1);
  }
  return -1;
}

// find or claim the slot of `key` and fold (c, tf, tl) into its values.  0: folded into a present key, 1: a new key
// was claimed, -1: no slot within `cap` probes (nothing written)
__device__ __forceinline__ int upsert(const Table& tb, uint64_t key, uint32_t c, uint32_t tf, uint32_t tl) {
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(tb.key);
  int64_t slot = home(key, tb.log2cap);
  int claimed = 0;
  int64_t i = 0;
  for (; i < tb.cap; ++i) {
    uint64_t k = __hip_atomic_load(&tb.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == EMPTY) {
      k = atomicCAS(&keys[slot], (unsigned long long)EMPTY, (unsigned long long)key);
      if (k == EMPTY) {
        claimed = 1;
        break;
      }
    }
    if (k == key) break;
    slot = (slot + 1) & (tb.cap - 1);
  }
  if (i == tb.cap) return -1;
  atomicAdd(&tb.count[slot], c);
  atomicMin(&tb.t_first[slot], tf);
  atomicMax(&tb.t_last[slot], tl);
  return claimed;
}

// status[which] += the number of lanes of the wave with `flag`; called by every lane of the block, reconverged
__device__ __forceinline__ void wave_count(unsigned long long* status, int which, bool flag) {
  const uint64_t b = __ballot(flag);
  if ((threadIdx.x & (WAVE - 1)) == 0 && b) atomicAdd(&status[which], (unsigned long long)__popcll(b));
}

__global__ void __launch_bounds__(T) k_init(Table tb) {
  for (int64_t i = blockIdx.x * (int64_t)T + threadIdx.x; i < tb.cap; i += (int64_t)gridDim.x * T) {
    tb.key[i] = EMPTY;
    tb.count[i] = 0;
    tb.t_first[i] = TF_ID;
    tb.t_last[i] = TL_ID;
  }
}

// one thread per event (the trip count is uniform over the block so the ballots see whole waves)
__global__ void __launch_bounds__(T) k_insert(Table tb, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                              const float* __restrict__ t, int64_t n, int64_t N,
                                              unsigned long long* __restrict__ status) {
  for (int64_t b0 = blockIdx.x * (int64_t)T; b0 < n; b0 += (int64_t)gridDim.x * T) {
    const int64_t i = b0 + threadIdx.x;
    int r = 0;
    bool bad = false;
    if (i < n) {
      const int64_t s = src[i], d = dst[i];
      const float ti = t[i];
      bad = s < 0 || s >= N || d < 0 || d >= N || ti != ti;
      if (!bad) {
        const uint32_t u = t_enc(ti);
        r = upsert(tb, ((uint64_t)s << 32) | (uint64_t)d, 1u, u, u);
      }
    }
    wave_count(status, 0, r == 1);
    wave_count(status, 1, bad);
    wave_count(status, 2, r < 0);
  }
}

// insert with given values (a checkpoint's rows): count 0, an id out of range or a NaN stamp is invalid
__global__ void __launch_bounds__(T) k_import(Table tb, const int64_t* __restrict__ keys, const int64_t* __restrict__ count,
                                              const float* __restrict__ t_first, const float* __restrict__ t_last,
                                              int64_t n, int64_t N, unsigned long long* __restrict__ status) {
  for (int64_t b0 = blockIdx.x * (int64_t)T; b0 < n; b0 += (int64_t)gridDim.x * T) {
    const int64_t i = b0 + threadIdx.x;
    int r = 0;
    bool bad = false;
    if (i < n) {
      const uint64_t key = (uint64_t)keys[i];
      const int64_t s = (int64_t)(key >> 32), d = (int64_t)(key & 0xFFFFFFFFull), c = count[i];
      const float tf = t_first[i], tl = t_last[i];
      bad = s >= N || d >= N || c <= 0 || c > 0xFFFFFFFFll || tf != tf || tl != tl;
      if (!bad) r = upsert(tb, key, (uint32_t)c, t_enc(tf), t_enc(tl));
    }
    wave_count(status, 0, r == 1);
    wave_count(status, 1, bad);
    wave_count(status, 2, r < 0);
  }
}

__global__ void __launch_bounds__(T) k_lookup(Table tb, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                              int64_t n, int64_t N, const float* __restrict__ since, float since_all,
                                              uint8_t* __restrict__ out_seen, int64_t* __restrict__ out_count,
                                              float* __restrict__ out_tf, float* __restrict__ out_tl) {
  for (int64_t i = blockIdx.x * (int64_t)T + threadIdx.x; i < n; i += (int64_t)gridDim.x * T) {
    const int64_t s = src[i], d = dst[i];
    int64_t slot = -1;
    if (s >= 0 && s < N && d >= 0 && d < N) slot = find(tb, ((uint64_t)s << 32) | (uint64_t)d);
    const float tl = slot >= 0 ? t_dec(tb.t_last[slot]) : -INFINITY;
    if (out_seen) out_seen[i] = slot >= 0 && tl >= (since ? since[i] : since_all) ? 1 : 0;
    if (out_count) out_count[i] = slot >= 0 ? (int64_t)tb.count[slot] : 0;
    if (out_tf) out_tf[i] = slot >= 0 ? t_dec(tb.t_first[slot]) : INFINITY;
    if (out_tl) out_tl[i] = tl;
  }
}

// One work item = (source q, chunk of SEL_CHUNK candidates).  The count pass stores the item's hits in cnt[item];
// the fill pass writes them from off[item] on in candidate order (ballot + prefix over the block, no cursor), so
// the output is the same for every grid.
template <bool FILL>
__global__ void __launch_bounds__(T) k_select(Table tb, const int64_t* __restrict__ src, int64_t Q,
                                              const int64_t* __restrict__ cand, int64_t C, int64_t nchunk, int64_t N,
                                              const float* __restrict__ since, float since_all, int64_t* __restrict__ cnt,
                                              const int64_t* __restrict__ off, int64_t* __restrict__ out_ids,
                                              int64_t out_cap) {
  __shared__ int wsum[T / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int64_t items = Q * nchunk;
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) cnt[items] = 0;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t q = w / nchunk, ch = w - q * nchunk;
    const int64_t s = src[q];
    const bool s_ok = s >= 0 && s < N;
    const float cut = since ? since[q] : since_all;
    const int64_t base = FILL ? off[w] : 0;
    int total = 0;
    for (int it = 0; it < SEL_ITERS; ++it) {
      const int64_t c = ch * SEL_CHUNK + (int64_t)it * T + threadIdx.x;
      bool hit = false;
      int64_t d = -1;
      if (s_ok && c < C) {
        d = cand[c];
        if (d >= 0 && d < N) {
          const int64_t slot = find(tb, ((uint64_t)s << 32) | (uint64_t)d);
          hit = slot >= 0 && t_dec(tb.t_last[slot]) >= cut;
        }
      }
      const uint64_t b = __ballot(hit);
      if (lane == 0) wsum[wv] = __popcll(b);
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int i = 0; i < T / WAVE; ++i) {
        if (i < wv) before += wsum[i];
        all += wsum[i];
      }
      if (FILL && hit) {
        const int64_t pos = base + total + before + __popcll(b & ((1ull << lane) - 1ull));
        if (pos < out_cap) out_ids[pos] = d;
      }
      total += all;
      __syncthreads();
    }
    if (!FILL && threadIdx.x == 0) cnt[w] = total;
  }
}

__global__ void __launch_bounds__(T) k_select_ptr(const int64_t* __restrict__ off, int64_t Q, int64_t nchunk,
                                                  int64_t* __restrict__ ptr) {
  for (int64_t q = blockIdx.x * (int64_t)T + threadIdx.x; q <= Q; q += (int64_t)gridDim.x * T) ptr[q] = off[q * nchunk];
}

// every live entry of `old` whose endpoints are not flagged goes into `nw` with its values
__global__ void __launch_bounds__(T) k_rehash(Table old, Table nw, const uint8_t* __restrict__ drop, int64_t N,
                                              unsigned long long* __restrict__ status) {
  for (int64_t b0 = blockIdx.x * (int64_t)T; b0 < old.cap; b0 += (int64_t)gridDim.x * T) {
    const int64_t i = b0 + threadIdx.x;
    int r = 0;
    if (i < old.cap) {
      const uint64_t key = old.key[i];
      if (key != EMPTY) {
        const int64_t s = (int64_t)(key >> 32), d = (int64_t)(key & 0xFFFFFFFFull);
        bool keep = true;
        if (drop) keep = s < N && d < N && !drop[s] && !drop[d];  // (the flags have N entries)
        if (keep) r = upsert(nw, key, old.count[i], old.t_first[i], old.t_last[i]);
      }
    }
    wave_count(status, 0, r == 1);
    wave_count(status, 2, r < 0);
  }
}

// the live entries, compacted through a wave-aggregated cursor: the order follows the layout and the schedule, the
// caller sorts by key.  Rows beyond max_out are counted in out_n but not written.
__global__ void __launch_bounds__(T) k_export(Table tb, int64_t* __restrict__ out_keys, int64_t* __restrict__ out_count,
                                              float* __restrict__ out_tf, float* __restrict__ out_tl, int64_t max_out,
                                              unsigned long long* __restrict__ out_n) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (int64_t b0 = blockIdx.x * (int64_t)T; b0 < tb.cap; b0 += (int64_t)gridDim.x * T) {
    const int64_t i = b0 + threadIdx.x;
    const uint64_t key = i < tb.cap ? tb.key[i] : EMPTY;
    const bool live = key != EMPTY;
    const uint64_t b = __ballot(live);
    unsigned long long base = 0;
    if (lane == 0 && b) base = atomicAdd(out_n, (unsigned long long)__popcll(b));
    base = __shfl(base, 0, WAVE);
    if (live) {
      const int64_t pos = (int64_t)base + __popcll(b & ((1ull << lane) - 1ull));
      if (pos < max_out) {
        out_keys[pos] = (int64_t)key;
        out_count[pos] = (int64_t)tb.count[i];
        out_tf[pos] = t_dec(tb.t_first[i]);
        out_tl[pos] = t_dec(tb.t_last[i]);
      }
    }
  }
}

struct SelWs {
  size_t cnt, off, temp, temp_bytes, total;
};
static size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
static int64_t sel_chunks(int64_t C) { return (C + SEL_CHUNK - 1) / SEL_CHUNK; }
static bool sel_ok(int64_t Q, int64_t C) {
  return Q >= 0 && C >= 0 && C < (int64_t(1) << 40) && Q < (int64_t(1) << 31) &&
         (Q == 0 || sel_chunks(C) < ((int64_t(1) << 31) - 1) / std::max<int64_t>(Q, 1));
}
static SelWs sel_ws(int64_t Q, int64_t C) {
  SelWs w;
  const int64_t items = Q * sel_chunks(C) + 1;
  size_t scan = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int64_t*)nullptr, (int64_t*)nullptr, (int)items);
  size_t o = 0;
  w.cnt = o; o += al256((size_t)items * 8);
  w.off = o; o += al256((size_t)items * 8);
  w.temp_bytes = scan;
  w.temp = o; o += al256(std::max<size_t>(scan, 1));
  w.total = o;
  return w;
}

}  // namespace pairset
}  // namespace tgnx

using namespace tgnx;
using namespace tgnx::pairset;

extern "C" {

size_t tgnx_pairset_bytes(int64_t capacity) { return cap_ok(capacity) ? (size_t)capacity * 20 : 0; }

int tgnx_pairset_init(void* table, int64_t capacity, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_init: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(table, "tgnx_pairset_init: null pointer");
  k_init<<<grid_for(capacity), T, 0, as_stream(stream)>>>(view(table, capacity));
  TGNX_LAUNCH_CHECK("pairset_init");
  return TGNX_OK;
}

int tgnx_pairset_insert(void* table, int64_t capacity, const int64_t* src, const int64_t* dst, const float* t, int64_t n,
                        int64_t num_nodes, int64_t* status, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_insert: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(nodes_ok(num_nodes), "tgnx_pairset_insert: num_nodes must be in [1, 2^32 - 1]");
  TGNX_CHECK_ARG(n >= 0, "tgnx_pairset_insert: n < 0");
  if (n == 0) return TGNX_OK;
  TGNX_CHECK_ARG(table && src && dst && t && status, "tgnx_pairset_insert: null pointer");
  k_insert<<<grid_for(n), T, 0, as_stream(stream)>>>(view(table, capacity), src, dst, t, n, num_nodes,
                                                     reinterpret_cast<unsigned long long*>(status));
  TGNX_LAUNCH_CHECK("pairset_insert");
  return TGNX_OK;
}

int tgnx_pairset_import(void* table, int64_t capacity, const int64_t* keys, const int64_t* count, const float* t_first,
                        const float* t_last, int64_t n, int64_t num_nodes, int64_t* status, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_import: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(nodes_ok(num_nodes), "tgnx_pairset_import: num_nodes must be in [1, 2^32 - 1]");
  TGNX_CHECK_ARG(n >= 0, "tgnx_pairset_import: n < 0");
  if (n == 0) return TGNX_OK;
  TGNX_CHECK_ARG(table && keys && count && t_first && t_last && status, "tgnx_pairset_import: null pointer");
  k_import<<<grid_for(n), T, 0, as_stream(stream)>>>(view(table, capacity), keys, count, t_first, t_last, n, num_nodes,
                                                     reinterpret_cast<unsigned long long*>(status));
  TGNX_LAUNCH_CHECK("pairset_import");
  return TGNX_OK;
}

int tgnx_pairset_lookup(const void* table, int64_t capacity, int64_t num_nodes, const int64_t* src, const int64_t* dst,
                        int64_t n, const float* since, float since_all, uint8_t* out_seen, int64_t* out_count,
                        float* out_t_first, float* out_t_last, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_lookup: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(nodes_ok(num_nodes), "tgnx_pairset_lookup: num_nodes must be in [1, 2^32 - 1]");
  TGNX_CHECK_ARG(n >= 0, "tgnx_pairset_lookup: n < 0");
  if (n == 0) return TGNX_OK;
  TGNX_CHECK_ARG(table && src && dst, "tgnx_pairset_lookup: null pointer");
  k_lookup<<<grid_for(n), T, 0, as_stream(stream)>>>(view(const_cast<void*>(table), capacity), src, dst, n, num_nodes,
                                                     since, since_all, out_seen, out_count, out_t_first, out_t_last);
  TGNX_LAUNCH_CHECK("pairset_lookup");
  return TGNX_OK;
}

size_t tgnx_pairset_select_ws_bytes(int64_t Q, int64_t C) { return sel_ok(Q, C) ? sel_ws(Q, C).total : 0; }

int tgnx_pairset_select_count(const void* table, int64_t capacity, int64_t num_nodes, const int64_t* src, int64_t Q,
                              const int64_t* cand, int64_t C, const float* since, float since_all, int64_t* out_ptr,
                              void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_select_count: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(nodes_ok(num_nodes), "tgnx_pairset_select_count: num_nodes must be in [1, 2^32 - 1]");
  TGNX_CHECK_ARG(sel_ok(Q, C), "tgnx_pairset_select_count: Q / C out of range");
  TGNX_CHECK_ARG(table && out_ptr && ws && (Q == 0 || src) && (C == 0 || cand), "tgnx_pairset_select_count: null pointer");
  const SelWs L = sel_ws(Q, C);
  TGNX_CHECK_ARG(ws_bytes >= L.total, "tgnx_pairset_select_count: workspace too small");
  hipStream_t s = as_stream(stream);
  const int64_t nchunk = sel_chunks(C), items = Q * nchunk;
  if (items == 0) {
    TGNX_HIP_CHECK(hipMemsetAsync(out_ptr, 0, (size_t)(Q + 1) * 8, s));
    return TGNX_OK;
  }
  unsigned char* w = static_cast<unsigned char*>(ws);
  int64_t* cnt = reinterpret_cast<int64_t*>(w + L.cnt);
  int64_t* off = reinterpret_cast<int64_t*>(w + L.off);
  k_select<false><<<(unsigned)std::min<int64_t>(items, MAX_GRID), T, 0, s>>>(
      view(const_cast<void*>(table), capacity), src, Q, cand, C, nchunk, num_nodes, since, since_all, cnt, nullptr,
      nullptr, 0);
  TGNX_LAUNCH_CHECK("pairset_select_count");
  size_t temp = L.temp_bytes;
  TGNX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w + L.temp, temp, cnt, off, (int)(items + 1), s));
  k_select_ptr<<<grid_for(Q + 1), T, 0, s>>>(off, Q, nchunk, out_ptr);
  TGNX_LAUNCH_CHECK("pairset_select_ptr");
  return TGNX_OK;
}

int tgnx_pairset_select_fill(const void* table, int64_t capacity, int64_t num_nodes, const int64_t* src, int64_t Q,
                             const int64_t* cand, int64_t C, const float* since, float since_all, int64_t* out_ids,
                             int64_t out_cap, const void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_select_fill: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(nodes_ok(num_nodes), "tgnx_pairset_select_fill: num_nodes must be in [1, 2^32 - 1]");
  TGNX_CHECK_ARG(sel_ok(Q, C) && out_cap >= 0, "tgnx_pairset_select_fill: Q / C / out_cap out of range");
  const int64_t nchunk = sel_chunks(C), items = Q * nchunk;
  if (items == 0 || out_cap == 0) return TGNX_OK;
  TGNX_CHECK_ARG(table && out_ids && ws && src && cand, "tgnx_pairset_select_fill: null pointer");
  const SelWs L = sel_ws(Q, C);
  TGNX_CHECK_ARG(ws_bytes >= L.total, "tgnx_pairset_select_fill: workspace too small");
  const unsigned char* w = static_cast<const unsigned char*>(ws);
  k_select<true><<<(unsigned)std::min<int64_t>(items, MAX_GRID), T, 0, as_stream(stream)>>>(
      view(const_cast<void*>(table), capacity), src, Q, cand, C, nchunk, num_nodes, since, since_all, nullptr,
      reinterpret_cast<const int64_t*>(w + L.off), out_ids, out_cap);
  TGNX_LAUNCH_CHECK("pairset_select_fill");
  return TGNX_OK;
}

int tgnx_pairset_rehash(const void* old_table, int64_t old_capacity, void* new_table, int64_t new_capacity,
                        const uint8_t* drop_flags, int64_t num_nodes, int64_t* status, void* stream) {
  TGNX_CHECK_ARG(cap_ok(old_capacity) && cap_ok(new_capacity), "tgnx_pairset_rehash: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(nodes_ok(num_nodes), "tgnx_pairset_rehash: num_nodes must be in [1, 2^32 - 1]");
  TGNX_CHECK_ARG(old_table && new_table && status && old_table != new_table, "tgnx_pairset_rehash: null or aliased pointer");
  hipStream_t s = as_stream(stream);
  TGNX_HIP_CHECK(hipMemsetAsync(status, 0, 8, s));
  k_rehash<<<grid_for(old_capacity), T, 0, s>>>(view(const_cast<void*>(old_table), old_capacity),
                                                view(new_table, new_capacity), drop_flags, num_nodes,
                                                reinterpret_cast<unsigned long long*>(status));
  TGNX_LAUNCH_CHECK("pairset_rehash");
  return TGNX_OK;
}

int tgnx_pairset_export(const void* table, int64_t capacity, int64_t* out_keys, int64_t* out_count, float* out_t_first,
                        float* out_t_last, int64_t max_out, int64_t* out_n, void* stream) {
  TGNX_CHECK_ARG(cap_ok(capacity), "tgnx_pairset_export: capacity must be a power of two >= 64");
  TGNX_CHECK_ARG(max_out >= 0, "tgnx_pairset_export: max_out < 0");
  TGNX_CHECK_ARG(table && out_n && (max_out == 0 || (out_keys && out_count && out_t_first && out_t_last)),
                 "tgnx_pairset_export: null pointer");
  hipStream_t s = as_stream(stream);
  TGNX_HIP_CHECK(hipMemsetAsync(out_n, 0, 8, s));
  k_export<<<grid_for(capacity), T, 0, s>>>(view(const_cast<void*>(table), capacity), out_keys, out_count, out_t_first,
                                            out_t_last, max_out, reinterpret_cast<unsigned long long*>(out_n));
  TGNX_LAUNCH_CHECK("pairset_export");
  return TGNX_OK;
}

}  // extern "C"
