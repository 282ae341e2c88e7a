// TGB-style evaluation negatives (hist_rnd) from a device (source, destination) pair index, for gfx950.
// DESIGN §3b-12 has the contract; tests/tgb_negs_ref.py restates it in numpy.
//
// Pair index (tgnx_pair_index_build): one stable radix sort (hipCUB) of (src << 32 | dst) keys carrying the row number
// leaves every duplicate run starting at its smallest row; head flags, an exclusive scan and a scatter give the CSR
// (indptr, indices = each source's distinct destinations ascending, first = the pair's first row).  A query
// (tgnx_pair_index_contains) is one binary search per lane in the source's row.
//
// Generator (tgnx_negs_hist_rnd), per call:
//   1. the CSR restricted to first < hist_hi: flag / scan / scatter over nnz; the scan's packed 64-bit sums carry, in
//      the high word, how many kept entries are in the pool (|valid| needs |pool ∩ Hc| per source);
//   2. the split's rows grouped by (source, equal-time run) with destinations ascending inside a group: a sort by
//      destination, then a stable sort by (src << 32 | first row of the run).  An event's same-time positives P are
//      then one contiguous, sorted run found by two binary searches, whatever the length of the timestamp's run;
//   3. one 256-thread workgroup per event row: draws 256 at a time, membership in Hc and P by binary search, the
//      accepted values in an LDS hash set keyed by value and holding the smallest draw index (so "the first `target`
//      distinct valid values of the sequence" is a flag, a block scan and a cut), each part sorted in LDS and stored.
// Nothing depends on the grid: row r of the output is computed by block r from (seed, tag, event row, draw index).
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "tgnx_common.h"

namespace tgnx {
namespace negs {

constexpr int T = 256;          // threads of a row's workgroup = draws per chunk
constexpr int MAX_K = 1024;
constexpr int TAB_BITS = 12;    // LDS hash set: at most MAX_K accepted + T of the last chunk of 4,096 slots
constexpr int TAB = 1 << TAB_BITS;
constexpr uint64_t EMPTY = ~0ull;
constexpr uint64_t TAG_HIST = 0x68697374ull, TAG_RND = 0x726E6473ull;

// ---------------------------------------------------------------- searches
// first position in [0, n) with a[pos] >= v
template <class A, class V>
__device__ __forceinline__ int64_t lower_bound(const A* __restrict__ a, int64_t n, V v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
template <class A, class V>
__device__ __forceinline__ int64_t upper_bound(const A* __restrict__ a, int64_t n, V v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
template <class A, class V>
__device__ __forceinline__ bool in_sorted(const A* __restrict__ a, int64_t n, V v) {
  const int64_t p = lower_bound(a, n, v);
  return p < n && a[p] == v;
}

// ---------------------------------------------------------------- pair index
__global__ void pair_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t n, int64_t N,
                          uint64_t* __restrict__ key, uint32_t* __restrict__ val, int* __restrict__ flags) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t s = src[j], d = dst[j];
    if (s < 0 || s >= N || d < 0 || d >= (int64_t(1) << 32)) {  // reported by the host; the key stays in range
      flags[0] = 1;
      s = 0;
      d = 0;
    }
    key[j] = ((uint64_t)s << 32) | (uint64_t)d;
    val[j] = (uint32_t)j;
  }
}

__global__ void pair_heads(const uint64_t* __restrict__ key, int64_t n, int* __restrict__ head) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
    head[i] = i < n && (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

__global__ void pair_fill(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, const int* __restrict__ pos,
                          int64_t n, int64_t N, int64_t* __restrict__ indptr, int64_t* __restrict__ indices,
                          int64_t* __restrict__ first) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p <= n; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t node = p < n ? (int64_t)(key[p] >> 32) : N;
    const int64_t prev = p > 0 ? (int64_t)(key[p - 1] >> 32) : -1;
    for (int64_t v = prev + 1; v <= node; ++v) indptr[v] = pos[p];  // rows (prev, node] start at p's compact position
    if (p < n && (p == 0 || key[p] != key[p - 1])) {
      indices[pos[p]] = (int64_t)(key[p] & 0xFFFFFFFFull);
      first[pos[p]] = (int64_t)val[p];  // stable sort: the run's head is its smallest row
    }
  }
}

__global__ void pair_contains(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                              const int64_t* __restrict__ first, int64_t N, const int64_t* __restrict__ src,
                              const int64_t* __restrict__ dst, int64_t n, const int64_t* __restrict__ before,
                              int64_t before_all, uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = src[i], d = dst[i];
    bool r = false;
    if (s >= 0 && s < N) {
      const int64_t a = indptr[s], len = indptr[s + 1] - a;
      const int64_t p = lower_bound(indices + a, len, d);
      r = p < len && indices[a + p] == d && first[a + p] < (before ? before[i] : before_all);
    }
    out[i] = r ? 1 : 0;
  }
}

struct SortWs {
  size_t keys_a, keys_b, vals_a, vals_b, head, pos, flags, temp, temp_bytes, total;
};
static size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

static size_t sort_temp_bytes(int64_t n) {
  size_t temp = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, temp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int)n, 0, 64);  // size query only
  return temp;
}

static SortWs pair_ws(int64_t n) {
  SortWs w;
  size_t scan = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int*)nullptr, (int*)nullptr, (int)(n + 1));
  size_t o = 0;
  w.keys_a = o; o += al256((size_t)n * 8);
  w.keys_b = o; o += al256((size_t)n * 8);
  w.vals_a = o; o += al256((size_t)n * 4);
  w.vals_b = o; o += al256((size_t)n * 4);
  w.head = o; o += al256((size_t)(n + 1) * 4);
  w.pos = o; o += al256((size_t)(n + 1) * 4);
  w.flags = o; o += 256;
  w.temp_bytes = std::max(sort_temp_bytes(n), scan);
  w.temp = o; o += al256(w.temp_bytes);
  w.total = o;
  return w;
}

static int bits_for(int64_t n) {
  int b = 1;
  while (b < 32 && (int64_t(1) << b) < n) ++b;  // ids < n fit in b bits
  return b;
}

// ---------------------------------------------------------------- generator, passes over nnz and over the split
// S_in[i] = kept | (kept and in the pool) << 32; entry nnz is 0 so the exclusive scan's last element is the total
__global__ void restrict_flags(const int64_t* __restrict__ first, const int64_t* __restrict__ indices, int64_t nnz,
                               int64_t hist_hi, const int64_t* __restrict__ pool, int64_t n_pool,
                               uint64_t* __restrict__ S_in) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nnz; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t f = 0;
    if (i < nnz && first[i] < hist_hi) f = 1ull | ((uint64_t)in_sorted(pool, n_pool, indices[i]) << 32);
    S_in[i] = f;
  }
}

__global__ void restrict_scatter(const int64_t* __restrict__ first, const int64_t* __restrict__ indices, int64_t nnz,
                                 int64_t hist_hi, const uint64_t* __restrict__ S, int64_t* __restrict__ rind) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x)
    if (first[i] < hist_hi) rind[(uint32_t)S[i]] = indices[i];
}

__global__ void split_keys_dst(const int64_t* __restrict__ dst, int64_t lo, int64_t n, uint64_t* __restrict__ key,
                               uint32_t* __restrict__ val) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    key[j] = (uint64_t)dst[lo + j] & 0xFFFFFFFFull;
    val[j] = (uint32_t)j;
  }
}

// rows arrive in destination order (perm); the key of the second, stable sort is (src << 32 | first row of the row's
// equal-time run), the carried value the destination
template <class TT>
__global__ void split_keys_group(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                 const TT* __restrict__ t, int64_t lo, int64_t n, const uint32_t* __restrict__ perm,
                                 uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = perm[i];
    const uint64_t run = (uint64_t)lower_bound(t + lo, n, t[lo + j]);
    key[i] = ((uint64_t)src[lo + j] << 32) | run;
    val[i] = (uint32_t)dst[lo + j];
  }
}

struct NegWs {
  size_t S_in, S, rind, keys_a, keys_b, vals_a, vals_b, temp, temp_bytes, total;
};
static NegWs neg_ws(int64_t nnz, int64_t n) {
  NegWs w;
  size_t scan = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)(nnz + 1));
  size_t o = 0;
  w.S_in = o; o += al256((size_t)(nnz + 1) * 8);
  w.S = o; o += al256((size_t)(nnz + 1) * 8);
  w.rind = o; o += al256((size_t)std::max<int64_t>(nnz, 1) * 8);
  w.keys_a = o; o += al256((size_t)n * 8);
  w.keys_b = o; o += al256((size_t)n * 8);
  w.vals_a = o; o += al256((size_t)n * 4);
  w.vals_b = o; o += al256((size_t)n * 4);
  w.temp_bytes = std::max(sort_temp_bytes(std::max<int64_t>(n, 1)), scan);
  w.temp = o; o += al256(w.temp_bytes);
  w.total = o;
  return w;
}

// ---------------------------------------------------------------- generator, one workgroup per event row
struct RowArgs {
  const int64_t* src;
  const void* t;
  int64_t lo, n;
  int k, q;
  const int64_t* indptr;
  int64_t N;
  const uint64_t* S;       // exclusive packed scan over the index entries, nnz + 1 long
  const int64_t* rind;     // the restricted CSR's destinations
  const uint64_t* gkey;    // the split's rows by (src << 32 | run), n long
  const uint32_t* gdst;    // ... their destinations, ascending inside a group
  const int64_t* pool;
  int64_t n_pool;
  uint64_t seed;
  int64_t max_draws;
  int64_t* out;
  int32_t* k_hist;
  unsigned long long* status;
};

__device__ __forceinline__ int tab_slot(int64_t v) { return (int)(((uint32_t)v * 0x9E3779B1u) >> (32 - TAB_BITS)); }

__device__ __forceinline__ bool tab_has(const uint64_t* tab, int64_t v) {
  for (int sl = tab_slot(v);; sl = (sl + 1) & (TAB - 1)) {
    const uint64_t x = tab[sl];
    if (x == EMPTY) return false;
    if ((int64_t)(x >> 32) == v) return true;
  }
}

// The first `target` distinct values of the sequence table[idx(a)], a = 0, 1, ... < cap, that `banned` does not
// refuse, into okey[0, got) in draw order; returns got.  tab ends holding exactly the accepted values when got <
// target (the cap cut the sequence: every new value of every chunk was accepted).
template <class Banned>
__device__ int draw_part(uint64_t seed, uint64_t tag, int64_t e, const int64_t* __restrict__ table, int64_t n_table,
                         int target, int64_t max_draws, Banned banned, uint64_t* tab, uint64_t* okey, int* sh) {
  const int tid = threadIdx.x;
  for (int i = tid; i < TAB; i += T) tab[i] = EMPTY;
  __syncthreads();
  const int64_t cap = max_draws > 0 ? max_draws : 16 * (int64_t)target + 256;
  int got = 0;
  for (int64_t base = 0; base < cap && got < target; base += T) {  // (uniform)
    const int64_t a = base + tid;
    int64_t v = 0;
    bool ok = false;
    if (a < cap) {  // the last chunk is cut by draw index
      const uint64_t h = hash4(seed, tag, (uint64_t)e, (uint64_t)a);
      v = table[(int64_t)(((__uint128_t)(h >> 11) * (uint64_t)n_table) >> 53)];
      ok = !banned(v);
    }
    const uint64_t pk = ((uint64_t)v << 32) | (uint64_t)(uint32_t)a;
    int sl = 0;
    if (ok) {  // the slot of v keeps the smallest draw index that produced it
      for (sl = tab_slot(v);; sl = (sl + 1) & (TAB - 1)) {
        const uint64_t old = atomicCAS((unsigned long long*)&tab[sl], (unsigned long long)EMPTY, (unsigned long long)pk);
        if (old == EMPTY) break;
        if ((old >> 32) == (pk >> 32)) {
          atomicMin((unsigned long long*)&tab[sl], (unsigned long long)pk);
          break;
        }
      }
    }
    __syncthreads();
    const int isnew = ok && tab[sl] == pk ? 1 : 0;  // first occurrence, and not of an earlier chunk (smaller index)
    int tot;
    const int ex = block_excl_scan(isnew, sh, &tot);
    if (isnew && got + ex < target) okey[got + ex] = (uint64_t)v;  // the cut: the first target - got new values
    got = min(target, got + tot);
  }
  return got;
}

// okey[got, target) <- the smallest values of table (ascending) that `elig` admits and tab does not hold
template <class Elig>
__device__ int fill_up(const int64_t* __restrict__ table, int64_t n_table, int got, int target, Elig elig,
                       const uint64_t* tab, uint64_t* okey, int* sh) {
  for (int64_t base = 0; base < n_table && got < target; base += T) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < n_table ? table[i] : 0;
    const int f = i < n_table && elig(v) && !tab_has(tab, v) ? 1 : 0;
    int tot;
    const int ex = block_excl_scan(f, sh, &tot);
    if (f && got + ex < target) okey[got + ex] = (uint64_t)v;
    got = min(target, got + tot);
  }
  return got;
}

// okey[0, cnt) <- the values of table (ascending) that `elig` admits, at most `room` of them; returns cnt
template <class Elig>
__device__ int take_all(const int64_t* __restrict__ table, int64_t n_table, int room, Elig elig, uint64_t* okey, int* sh) {
  int cnt = 0;
  for (int64_t base = 0; base < n_table && cnt < room; base += T) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < n_table ? table[i] : 0;
    const int f = i < n_table && elig(v) ? 1 : 0;
    int tot;
    const int ex = block_excl_scan(f, sh, &tot);
    if (f && cnt + ex < room) okey[cnt + ex] = (uint64_t)v;
    cnt = min(room, cnt + tot);
  }
  return cnt;
}

__device__ __forceinline__ void sort_and_store(uint64_t* okey, uint64_t* otmp, int n, int64_t* __restrict__ out) {
  __syncthreads();
  if (n > 1) sort_u64(okey, otmp, n, next_pow2(n), false, true);
  for (int i = threadIdx.x; i < n; i += T) out[i] = (int64_t)okey[i];
  __syncthreads();
}

template <class TT>
__global__ void __launch_bounds__(T) negs_rows(const RowArgs A) {
  __shared__ uint64_t tab[TAB];
  __shared__ uint64_t okey[MAX_K];
  __shared__ uint64_t otmp[MAX_K];
  __shared__ int sh[40];
  __shared__ int64_t run[2];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x, e = A.lo + r;
  const int64_t s = A.src[e];
  const TT* t = static_cast<const TT*>(A.t);
  if (tid == 0) {  // the event's group in the (source, equal-time run) order: its same-time positives P
    const uint64_t key = ((uint64_t)s << 32) | (uint64_t)lower_bound(t + A.lo, A.n, t[e]);
    run[0] = lower_bound(A.gkey, A.n, key);
    run[1] = upper_bound(A.gkey, A.n, key);
  }
  __syncthreads();
  const uint32_t* P = A.gdst + run[0];
  const int64_t nP = run[1] - run[0];
  const bool known = s >= 0 && s < A.N;  // (a source outside the index has no history)
  const uint64_t Sa = A.S[known ? A.indptr[s] : 0], Sb = A.S[known ? A.indptr[s + 1] : 0];
  const int64_t* Hc = A.rind + (uint32_t)Sa;
  const int64_t nHc = (int64_t)(uint32_t)Sb - (int64_t)(uint32_t)Sa;
  const int64_t pool_hc = (int64_t)(Sb >> 32) - (int64_t)(Sa >> 32);
  auto inP = [&](int64_t v) { return in_sorted(P, nP, (uint32_t)v); };
  auto inHc = [&](int64_t v) { return in_sorted(Hc, nHc, v); };
  auto inX = [&](int64_t v) { return inHc(v) || inP(v); };
  auto notP = [&](int64_t v) { return !inP(v); };
  auto notX = [&](int64_t v) { return !inX(v); };

  // |Hc ∩ P| and |P \ Hc ∩ pool| over P's distinct values
  int c_hp = 0, c_ex = 0;
  for (int64_t i = tid; i < nP; i += T) {
    const uint32_t d = P[i];
    if (i == 0 || P[i - 1] != d) {
      if (inHc((int64_t)d)) ++c_hp;
      else if (in_sorted(A.pool, A.n_pool, (int64_t)d)) ++c_ex;
    }
  }
  int x0, x1, n_hp, n_ex;
  block_excl_scan2(c_hp, c_ex, sh, &x0, &x1, &n_hp, &n_ex);
  const int64_t nHn = nHc - n_hp, nValid = A.n_pool - pool_hc - n_ex;
  int64_t* out = A.out + r * A.k;

  // ---- historical part
  int kh;
  if (nHn <= A.q) {
    kh = take_all(Hc, nHc, (int)nHn, notP, okey, sh);  // ascending already
    __syncthreads();
    for (int i = tid; i < kh; i += T) out[i] = (int64_t)okey[i];
    __syncthreads();
  } else {
    kh = A.q;
    int got = draw_part(A.seed, TAG_HIST, e, Hc, nHc, kh, A.max_draws, inP, tab, okey, sh);
    if (got < kh) {
      got = fill_up(Hc, nHc, got, kh, notP, tab, okey, sh);
      if (tid == 0) atomicAdd(A.status + 1, 1ull);
    }
    sort_and_store(okey, otmp, kh, out);
  }
  if (tid == 0) A.k_hist[r] = kh;

  // ---- random part
  const int kr = A.k - kh;
  out += kh;
  if (kr == 0) return;
  if (nValid <= 0) {  // unusable row: reported, filled with -1
    for (int i = tid; i < kr; i += T) out[i] = -1;
    if (tid == 0) atomicMin(A.status, (unsigned long long)r);
  } else if (nValid < kr) {  // fewer valid destinations than slots: valid[i mod |valid|]
    const int m = take_all(A.pool, A.n_pool, (int)nValid, notX, otmp, sh);
    __syncthreads();
    for (int i = tid; i < kr; i += T) okey[i] = otmp[i % max(m, 1)];
    if (tid == 0) atomicAdd(A.status + 3, 1ull);
    sort_and_store(okey, otmp, kr, out);
  } else {
    int got = draw_part(A.seed, TAG_RND, e, A.pool, A.n_pool, kr, A.max_draws, inX, tab, okey, sh);
    if (got < kr) {
      got = fill_up(A.pool, A.n_pool, got, kr, notX, tab, okey, sh);
      if (tid == 0) atomicAdd(A.status + 2, 1ull);
    }
    sort_and_store(okey, otmp, kr, out);
  }
}

static int grid_for(int64_t n) { return (int)std::min<int64_t>(4096, (std::max<int64_t>(n, 1) + 255) / 256); }

}  // namespace negs
}  // namespace tgnx

using namespace tgnx;
using namespace tgnx::negs;

extern "C" {

size_t tgnx_pair_index_build_ws_bytes(int64_t num_rows) {
  if (num_rows <= 0 || num_rows >= (int64_t(1) << 31) - 1) return 256;
  return pair_ws(num_rows).total;
}

int tgnx_pair_index_build(const int64_t* src, const int64_t* dst, int64_t num_rows, int64_t num_nodes, int64_t* indptr,
                          int64_t* indices, int64_t* first, int64_t* nnz, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(num_nodes > 0 && num_nodes <= (int64_t(1) << 32), "tgnx_pair_index_build: ids must be below 2^32");
  TGNX_CHECK_ARG(num_rows >= 0 && num_rows < (int64_t(1) << 31) - 1, "tgnx_pair_index_build: more than 2^31 rows");
  TGNX_CHECK_ARG(indptr && ws && (num_rows == 0 || (src && dst && indices && first)),
                 "tgnx_pair_index_build: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_pair_index_build_ws_bytes(num_rows), "tgnx_pair_index_build: workspace too small");
  hipStream_t s = as_stream(stream);
  if (nnz) *nnz = 0;
  if (num_rows == 0) {
    TGNX_HIP_CHECK(hipMemsetAsync(indptr, 0, (size_t)(num_nodes + 1) * 8, s));
    return TGNX_OK;
  }
  unsigned char* w = static_cast<unsigned char*>(ws);
  const SortWs L = pair_ws(num_rows);
  uint64_t* ka = reinterpret_cast<uint64_t*>(w + L.keys_a);
  uint64_t* kb = reinterpret_cast<uint64_t*>(w + L.keys_b);
  uint32_t* va = reinterpret_cast<uint32_t*>(w + L.vals_a);
  uint32_t* vb = reinterpret_cast<uint32_t*>(w + L.vals_b);
  int* head = reinterpret_cast<int*>(w + L.head);
  int* pos = reinterpret_cast<int*>(w + L.pos);
  int* flags = reinterpret_cast<int*>(w + L.flags);
  TGNX_HIP_CHECK(hipMemsetAsync(flags, 0, 256, s));
  const int grid = grid_for(num_rows + 1);
  pair_keys<<<grid, 256, 0, s>>>(src, dst, num_rows, num_nodes, ka, va, flags);
  TGNX_LAUNCH_CHECK("pair_keys");
  size_t temp = L.temp_bytes;
  TGNX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(w + L.temp, temp, ka, kb, va, vb, (int)num_rows, 0,
                                                    32 + bits_for(num_nodes), s));
  pair_heads<<<grid, 256, 0, s>>>(kb, num_rows, head);
  TGNX_LAUNCH_CHECK("pair_heads");
  temp = L.temp_bytes;
  TGNX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w + L.temp, temp, head, pos, (int)(num_rows + 1), s));
  pair_fill<<<grid, 256, 0, s>>>(kb, vb, pos, num_rows, num_nodes, indptr, indices, first);
  TGNX_LAUNCH_CHECK("pair_fill");
  // offline preprocessing: a synchronous read of the id flag and of nnz is fine here
  int bad = 0, cnt = 0;
  TGNX_HIP_CHECK(hipMemcpyAsync(&bad, flags, sizeof(int), hipMemcpyDeviceToHost, s));
  TGNX_HIP_CHECK(hipMemcpyAsync(&cnt, pos + num_rows, sizeof(int), hipMemcpyDeviceToHost, s));
  TGNX_HIP_CHECK(hipStreamSynchronize(s));
  TGNX_CHECK_ARG(!bad, "tgnx_pair_index_build: a source outside [0, num_nodes) or a destination outside [0, 2^32)");
  if (nnz) *nnz = cnt;
  return TGNX_OK;
}

int tgnx_pair_index_contains(const int64_t* indptr, const int64_t* indices, const int64_t* first, int64_t num_nodes,
                             const int64_t* src, const int64_t* dst, int64_t n, const int64_t* before,
                             int64_t before_all, uint8_t* out, void* stream) {
  TGNX_CHECK_ARG(num_nodes > 0 && n >= 0, "tgnx_pair_index_contains: bad sizes");
  if (n == 0) return TGNX_OK;
  TGNX_CHECK_ARG(indptr && src && dst && out, "tgnx_pair_index_contains: null pointer");
  pair_contains<<<grid_for(n), 256, 0, as_stream(stream)>>>(indptr, indices, first, num_nodes, src, dst, n, before,
                                                           before_all, out);
  TGNX_LAUNCH_CHECK("pair_contains");
  return TGNX_OK;
}

size_t tgnx_negs_hist_rnd_ws_bytes(int64_t nnz, int64_t num_rows) {
  if (nnz < 0 || num_rows < 0 || nnz >= (int64_t(1) << 31) - 1 || num_rows >= (int64_t(1) << 31) - 1) return 256;
  return neg_ws(nnz, num_rows).total;
}

int tgnx_negs_hist_rnd(const int64_t* src, const int64_t* dst, const void* t, int32_t t_f64, int64_t num_events,
                       int64_t lo, int64_t hi, int32_t k, int32_t q, int64_t hist_hi, const int64_t* indptr,
                       const int64_t* indices, const int64_t* first, int64_t num_nodes, int64_t nnz,
                       const int64_t* pool, int64_t n_pool, uint64_t seed, int64_t max_draws, int64_t* out,
                       int32_t* k_hist, int64_t* status, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(k > 0 && k <= MAX_K, "tgnx_negs_hist_rnd: k must be in [1, 1024]");
  TGNX_CHECK_ARG(q >= 0 && q <= k, "tgnx_negs_hist_rnd: q must be in [0, k]");
  TGNX_CHECK_ARG(0 <= lo && lo <= hi && hi <= num_events && hi - lo < (int64_t(1) << 31) - 1,
                 "tgnx_negs_hist_rnd: rows [lo, hi) outside the event table");
  TGNX_CHECK_ARG(num_nodes > 0 && num_nodes <= (int64_t(1) << 32) && nnz >= 0 && nnz < (int64_t(1) << 31) - 1,
                 "tgnx_negs_hist_rnd: bad index sizes");
  TGNX_CHECK_ARG(n_pool > 0 && max_draws >= 0 && max_draws < (int64_t(1) << 31), "tgnx_negs_hist_rnd: bad pool / max_draws");
  TGNX_CHECK_ARG(src && dst && t && indptr && pool && status && ws && (nnz == 0 || (indices && first)) &&
                     (hi == lo || (out && k_hist)),
                 "tgnx_negs_hist_rnd: null pointer");
  const int64_t n = hi - lo;
  TGNX_CHECK_ARG(ws_bytes >= tgnx_negs_hist_rnd_ws_bytes(nnz, n), "tgnx_negs_hist_rnd: workspace too small");
  hipStream_t s = as_stream(stream);
  TGNX_HIP_CHECK(hipMemsetAsync(status, 0xFF, 8, s));  // -1: no unusable row (rows take an unsigned minimum)
  TGNX_HIP_CHECK(hipMemsetAsync(status + 1, 0, 24, s));
  if (n == 0) return TGNX_OK;
  unsigned char* w = static_cast<unsigned char*>(ws);
  const NegWs L = neg_ws(nnz, n);
  uint64_t* S_in = reinterpret_cast<uint64_t*>(w + L.S_in);
  uint64_t* S = reinterpret_cast<uint64_t*>(w + L.S);
  int64_t* rind = reinterpret_cast<int64_t*>(w + L.rind);
  uint64_t* ka = reinterpret_cast<uint64_t*>(w + L.keys_a);
  uint64_t* kb = reinterpret_cast<uint64_t*>(w + L.keys_b);
  uint32_t* va = reinterpret_cast<uint32_t*>(w + L.vals_a);
  uint32_t* vb = reinterpret_cast<uint32_t*>(w + L.vals_b);
  // 1. the index restricted to first < hist_hi
  restrict_flags<<<grid_for(nnz + 1), 256, 0, s>>>(first, indices, nnz, hist_hi, pool, n_pool, S_in);
  TGNX_LAUNCH_CHECK("negs_restrict_flags");
  size_t temp = L.temp_bytes;
  TGNX_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w + L.temp, temp, S_in, S, (int)(nnz + 1), s));
  if (nnz > 0) {
    restrict_scatter<<<grid_for(nnz), 256, 0, s>>>(first, indices, nnz, hist_hi, S, rind);
    TGNX_LAUNCH_CHECK("negs_restrict_scatter");
  }
  // 2. the split's rows by (source, equal-time run), destinations ascending inside a group
  split_keys_dst<<<grid_for(n), 256, 0, s>>>(dst, lo, n, ka, va);
  TGNX_LAUNCH_CHECK("negs_split_keys_dst");
  temp = L.temp_bytes;
  TGNX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(w + L.temp, temp, ka, kb, va, vb, (int)n, 0, 32, s));
  if (t_f64)
    split_keys_group<double><<<grid_for(n), 256, 0, s>>>(src, dst, static_cast<const double*>(t), lo, n, vb, ka, va);
  else
    split_keys_group<float><<<grid_for(n), 256, 0, s>>>(src, dst, static_cast<const float*>(t), lo, n, vb, ka, va);
  TGNX_LAUNCH_CHECK("negs_split_keys_group");
  temp = L.temp_bytes;
  TGNX_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(w + L.temp, temp, ka, kb, va, vb, (int)n, 0, 64, s));
  // 3. the rows
  RowArgs A;
  A.src = src; A.t = t; A.lo = lo; A.n = n; A.k = k; A.q = q;
  A.indptr = indptr; A.N = num_nodes; A.S = S; A.rind = rind; A.gkey = kb; A.gdst = vb;
  A.pool = pool; A.n_pool = n_pool; A.seed = seed; A.max_draws = max_draws;
  A.out = out; A.k_hist = k_hist; A.status = reinterpret_cast<unsigned long long*>(status);
  if (t_f64) negs_rows<double><<<(unsigned)n, T, 0, s>>>(A);
  else negs_rows<float><<<(unsigned)n, T, 0, s>>>(A);
  TGNX_LAUNCH_CHECK("negs_rows");
  return TGNX_OK;
}

}  // extern "C"
