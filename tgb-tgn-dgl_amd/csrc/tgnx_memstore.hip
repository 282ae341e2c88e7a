// The device message store of tgnx.nn.TGNMemory / DyRepMemory (modules/memory_module.py:140-145, :180-207;
// DyRep :376-412): put a batch, count + gather the stored events of a node set, build the message rows.
//
//   tgnx_memstore_put         _update_msg_store of both directions (:133-134, :180-191)      one launch
//   tgnx_memstore_count       per-node counts of a node set, scanned on the device           two launches
//   tgnx_memstore_gather      [msg_s of n_id[0], n_id[1], ...; msg_d of n_id[0], ...]: slot, owner, t and the
//                             per-owner max of t (:176)                                        one launch
//   tgnx_memstore_build_msg   [memory[src] | memory[dst] | raw_msg | cos(w t_rel + b)] rows (:193-207)
//
// Layout: an append-only event log (src, dst, t int64[cap], raw_msg f32[cap, d]) holds every
// batch once; the node table int64[4 N] is {s_off, s_cnt, d_off, d_cnt} per node, offsets into the arena
// int64[2 cap] of log slots; the batch that starts at log slot s owns arena entries [2s, 2s + 2B): its slots sorted
// stably by src, then sorted stably by dst.  A node that reappears points at its new run; the old one is dead.
//
// Determinism: no float atomics, no order-dependent sums; the only atomics count invalid ids.
#include <algorithm>

#include "tgnx_common.h"
#include "tgnx_math.h"

using namespace tgnx;

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_WAVES = MS_BLOCK / WAVE;
constexpr int MS_ITEMS = 4;                       // nodes per thread in the count / gather tiles
constexpr int MS_TILE = MS_BLOCK * MS_ITEMS;      // nodes per workgroup
constexpr int64_t MS_MAX_GRID = 2048;             // grid-stride above this many workgroups

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct alignas(16) NodeRow {
  int64_t s_off, s_cnt, d_off, d_cnt;
};

__device__ __forceinline__ void count_bad(int64_t* n_bad) {
  if (n_bad) atomicAdd(reinterpret_cast<unsigned long long*>(n_bad), 1ull);
}

// ------------------------------------------------------------------ (a) put
// x < 2B walks the two sorted key rows (src then dst): arena entry, and at the first element of a node's run the
// node's (off, cnt) — the run's end by a binary search in the sorted keys.  The log rows ride in the same launch.
__global__ void __launch_bounds__(MS_BLOCK) memstore_put_k(
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const int64_t* __restrict__ t,
    const float* __restrict__ raw, int64_t B, int64_t d, const int64_t* __restrict__ sorted,
    const int64_t* __restrict__ perm, int64_t start, int64_t N, int64_t* __restrict__ log_src,
    int64_t* __restrict__ log_dst, int64_t* __restrict__ log_t, float* __restrict__ log_raw,
    int64_t* __restrict__ arena, int64_t* __restrict__ node_tab, int64_t* n_bad, int vec_raw) {
  const int64_t stride = (int64_t)gridDim.x * MS_BLOCK, g = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  float* lr = log_raw + start * d;
  const int64_t nraw = B * d;
  if (vec_raw) {  // start * d and B * d multiples of 4, both bases 16-B aligned
    const float4* s4 = reinterpret_cast<const float4*>(raw);
    float4* d4 = reinterpret_cast<float4*>(lr);
    for (int64_t x = g; x < nraw / 4; x += stride) d4[x] = s4[x];
  } else {
    for (int64_t x = g; x < nraw; x += stride) lr[x] = raw[x];
  }
  for (int64_t x = g; x < 2 * B; x += stride) {
    const int dir = x >= B;
    const int64_t i = dir ? x - B : x;
    const int64_t* key = sorted + (dir ? B : 0);
    const int64_t node = key[i];
    int64_t p = perm[x];
    if (p < 0 || p >= B) {  // not a permutation of the batch: keep the slot inside the batch
      count_bad(n_bad);
      p = 0;
    }
    arena[2 * start + x] = start + p;
    if (!dir) {
      log_src[start + i] = src[i];
      log_dst[start + i] = dst[i];
      log_t[start + i] = t[i];
    }
    if (i == 0 || key[i - 1] != node) {
      if (node < 0 || node >= N) {
        count_bad(n_bad);
        continue;
      }
      int64_t lo = i + 1, hi = B;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] <= node) lo = mid + 1;
        else hi = mid;
      }
      node_tab[4 * node + 2 * dir] = 2 * start + x;
      node_tab[4 * node + 2 * dir + 1] = lo - i;
    }
  }
}

// ------------------------------------------------------------------ (b) count + gather
// One workgroup per tile of MS_TILE entries of n_id, MS_ITEMS consecutive ones per thread.
__device__ __forceinline__ NodeRow node_row(const int64_t* node_tab, int64_t N, const int64_t* n_id, int64_t M,
                                            int64_t i, int64_t* n_bad) {
  NodeRow r{0, 0, 0, 0};
  if (i < M) {
    const int64_t node = n_id[i];
    if (node >= 0 && node < N) r = reinterpret_cast<const NodeRow*>(node_tab)[node];
    else count_bad(n_bad);
    if (r.s_cnt < 0) r.s_cnt = 0;
    if (r.d_cnt < 0) r.d_cnt = 0;
  }
  return r;
}

__global__ void __launch_bounds__(MS_BLOCK) memstore_count_k(const int64_t* __restrict__ node_tab, int64_t N,
                                                             const int64_t* __restrict__ n_id, int64_t M,
                                                             int64_t* __restrict__ tile_sums, int64_t* n_bad) {
  __shared__ int sh[40];
  const int64_t i0 = ((int64_t)blockIdx.x * MS_BLOCK + threadIdx.x) * MS_ITEMS;
  int a = 0, b = 0;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    const NodeRow r = node_row(node_tab, N, n_id, M, i0 + k, n_bad);
    a += (int)r.s_cnt;
    b += (int)r.d_cnt;
  }
  int ra, rb, ta, tb;
  block_excl_scan2(a, b, sh, &ra, &rb, &ta, &tb);
  if (threadIdx.x == 0) {
    tile_sums[2 * blockIdx.x] = ta;
    tile_sums[2 * blockIdx.x + 1] = tb;
  }
}

// tile sums -> exclusive tile offsets (in place), totals = {n_s, n_d, invalid ids}.  One workgroup: thread k
// sums a contiguous share of the tiles, the 256 shares are scanned through LDS.
__global__ void __launch_bounds__(MS_BLOCK) memstore_scan_k(int64_t nt, int64_t* __restrict__ tiles,
                                                            int64_t* __restrict__ totals, const int64_t* put_bad) {
  __shared__ int64_t sh[2][MS_BLOCK];
  const int tid = threadIdx.x;
  const int64_t per = (nt + MS_BLOCK - 1) / MS_BLOCK;
  const int64_t b0 = min(nt, tid * per), b1 = min(nt, b0 + per);
  int64_t ss = 0, sd = 0;
  for (int64_t b = b0; b < b1; ++b) {
    ss += tiles[2 * b];
    sd += tiles[2 * b + 1];
  }
  sh[0][tid] = ss;
  sh[1][tid] = sd;
  __syncthreads();
  for (int o = 1; o < MS_BLOCK; o <<= 1) {
    const int64_t a = tid >= o ? sh[0][tid - o] : 0, c = tid >= o ? sh[1][tid - o] : 0;
    __syncthreads();
    sh[0][tid] += a;
    sh[1][tid] += c;
    __syncthreads();
  }
  int64_t es = sh[0][tid] - ss, ed = sh[1][tid] - sd;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t a = tiles[2 * b], c = tiles[2 * b + 1];
    tiles[2 * b] = es;
    tiles[2 * b + 1] = ed;
    es += a;
    ed += c;
  }
  if (tid == MS_BLOCK - 1) {
    totals[0] = sh[0][tid];
    totals[1] = sh[1][tid];
  }
  if (tid == 0 && put_bad) totals[2] += *put_bad;  // (the count kernel's own invalid ids are already there)
}

__device__ __forceinline__ void emit_run(const int64_t* __restrict__ arena, int64_t arena_len,
                                         const int64_t* __restrict__ log_t, int64_t fill, int64_t off, int64_t cnt,
                                         int64_t base, int64_t limit, int64_t owner, int64_t* __restrict__ out_slot,
                                         int64_t* __restrict__ out_owner, int64_t* __restrict__ out_t, bool& any,
                                         int64_t& mx) {
  for (int64_t k = 0; k < cnt; ++k) {
    const int64_t p = base + k, a = off + k;
    if (p >= limit) break;
    int64_t slot = (a >= 0 && a < arena_len) ? arena[a] : -1;
    const bool ok = slot >= 0 && slot < fill;
    const int64_t tv = ok ? log_t[slot] : 0;
    out_slot[p] = ok ? slot : -1;
    out_owner[p] = owner;
    out_t[p] = tv;
    mx = any ? max(mx, tv) : tv;
    any = true;
  }
}

__global__ void __launch_bounds__(MS_BLOCK) memstore_gather_k(
    const int64_t* __restrict__ node_tab, int64_t N, const int64_t* __restrict__ arena, int64_t arena_len,
    const int64_t* __restrict__ log_t, int64_t fill, const int64_t* __restrict__ n_id, int64_t M, int64_t n_s,
    int64_t n_d, const int64_t* __restrict__ tiles, int64_t* __restrict__ out_slot, int64_t* __restrict__ out_owner,
    int64_t* __restrict__ out_t, int64_t* __restrict__ out_lu) {
  __shared__ int sh[40];
  const int64_t i0 = ((int64_t)blockIdx.x * MS_BLOCK + threadIdx.x) * MS_ITEMS;
  NodeRow r[MS_ITEMS];
  int a = 0, b = 0;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    r[k] = node_row(node_tab, N, n_id, M, i0 + k, nullptr);
    a += (int)r[k].s_cnt;
    b += (int)r[k].d_cnt;
  }
  int ra, rb, ta, tb;
  block_excl_scan2(a, b, sh, &ra, &rb, &ta, &tb);
  int64_t ps = tiles[2 * blockIdx.x] + ra, pd = n_s + tiles[2 * blockIdx.x + 1] + rb;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i >= M) break;
    bool any = false;
    int64_t mx = 0;
    emit_run(arena, arena_len, log_t, fill, r[k].s_off, r[k].s_cnt, ps, n_s, i, out_slot, out_owner, out_t, any, mx);
    emit_run(arena, arena_len, log_t, fill, r[k].d_off, r[k].d_cnt, pd, n_s + n_d, i, out_slot, out_owner, out_t, any,
             mx);
    ps += r[k].s_cnt;
    pd += r[k].d_cnt;
    out_lu[i] = mx;
  }
}

// ------------------------------------------------------------------ (c) message rows
struct BuildArgs {
  const int64_t* slot;
  int64_t n_msg, n_s;
  const int64_t *log_src, *log_dst, *log_t;
  const float* log_raw;
  int64_t fill, N, D, d, T;
  const float* memory;
  const int64_t* last_update;
  const float *w, *b;
  const float* emb;       // DyRep: [E, D] (NULL: none)
  int64_t E;
  const int64_t* assoc;   // node -> row of emb
  const int64_t* stamp;   // the module's _assoc: node -> position in n_id, as the gather's caller stamped it
  const int64_t* n_id;
  int64_t M;
  int emb_flags;          // bit 0: owner rows from emb, bit 1: the other endpoint's
  int vec;                // bit g: column group g moves as 16-B vectors
  float *out, *t_rel;
};

// one wave per row: n floats from src (zeros when src is NULL) to dst
__device__ __forceinline__ void copy_cols(float* __restrict__ dst, const float* __restrict__ src, int64_t n, bool vec,
                                          int lane) {
  if (vec) {
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int64_t c = lane; c < n / 4; c += WAVE) d4[c] = src ? s4[c] : float4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int64_t c = lane; c < n; c += WAVE) dst[c] = src ? src[c] : 0.f;
  }
}

// x in n_id  <=>  stamp[x] < M and n_id[stamp[x]] == x (stale stamps of an earlier node set fail the second test)
__device__ __forceinline__ const float* endpoint_row(const BuildArgs& a, int64_t node, bool use_emb) {
  if (node < 0 || node >= a.N) return nullptr;
  if (use_emb) {
    const int64_t s = a.stamp[node];
    if (s >= 0 && s < a.M && a.n_id[s] == node) {
      const int64_t row = a.assoc[node];
      if (row >= 0 && row < a.E) return a.emb + row * a.D;
    }
  }
  return a.memory + node * a.D;
}

__global__ void __launch_bounds__(MS_BLOCK) memstore_build_k(BuildArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t W = 2 * a.D + a.d + a.T, nw = (int64_t)gridDim.x * MS_WAVES;
  for (int64_t p = (int64_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6); p < a.n_msg; p += nw) {
    const int64_t slot = a.slot[p];
    const bool ok = slot >= 0 && slot < a.fill;
    const int64_t es = ok ? a.log_src[slot] : -1, ed = ok ? a.log_dst[slot] : -1;
    const bool sdir = p < a.n_s;  // the owner is the event's src in the s store, its dst in the d store
    const int64_t own = sdir ? es : ed, oth = sdir ? ed : es;
    float trel = 0.f;
    if (own >= 0 && own < a.N) trel = (float)(a.log_t[slot] - a.last_update[own]);
    if (lane == 0) a.t_rel[p] = trel;
    float* o = a.out + p * W;
    copy_cols(o, endpoint_row(a, own, a.emb_flags & 1), a.D, a.vec & 1, lane);
    copy_cols(o + a.D, endpoint_row(a, oth, a.emb_flags & 2), a.D, a.vec & 2, lane);
    copy_cols(o + 2 * a.D, ok ? a.log_raw + slot * a.d : nullptr, a.d, a.vec & 4, lane);
    float* te = o + 2 * a.D + a.d;
    if (a.vec & 8) {
      for (int64_t c = 4 * lane; c < a.T; c += 4 * WAVE) {
        const float4 w4 = *reinterpret_cast<const float4*>(a.w + c), b4 = *reinterpret_cast<const float4*>(a.b + c);
        float4 v;
        v.x = te_cos(fmaf(w4.x, trel, b4.x));
        v.y = te_cos(fmaf(w4.y, trel, b4.y));
        v.z = te_cos(fmaf(w4.z, trel, b4.z));
        v.w = te_cos(fmaf(w4.w, trel, b4.w));
        *reinterpret_cast<float4*>(te + c) = v;
      }
    } else {
      for (int64_t c = lane; c < a.T; c += WAVE) te[c] = te_cos(fmaf(a.w[c], trel, a.b[c]));
    }
  }
}

size_t gather_ws_bytes(int64_t M) { return (size_t)(2 * std::max<int64_t>(ceil_div(M, MS_TILE), 1)) * 8; }

}  // namespace

extern "C" {

int tgnx_memstore_put(const int64_t* src, const int64_t* dst, const int64_t* t, const float* raw_msg, int64_t B,
                      int64_t msg_dim, const int64_t* sorted, const int64_t* perm, int64_t start, int64_t cap,
                      int64_t num_nodes, int64_t* log_src, int64_t* log_dst, int64_t* log_t, float* log_raw,
                      int64_t* arena, int64_t* node_tab, int64_t* n_bad, void* stream) {
  TGNX_CHECK_ARG(B >= 0 && msg_dim >= 0 && start >= 0 && cap >= 0 && num_nodes >= 0 && B < (int64_t(1) << 31) &&
                     msg_dim < (int64_t(1) << 24) && cap < (int64_t(1) << 40),
                 "tgnx_memstore_put: bad sizes (B %lld, msg_dim %lld, start %lld, cap %lld, num_nodes %lld)",
                 (long long)B, (long long)msg_dim, (long long)start, (long long)cap, (long long)num_nodes);
  TGNX_CHECK_ARG(start + B <= cap, "tgnx_memstore_put: capacity too small: start %lld + B %lld > cap %lld",
                 (long long)start, (long long)B, (long long)cap);
  if (B == 0) return TGNX_OK;
  TGNX_CHECK_ARG(src && dst && t && (msg_dim == 0 || (raw_msg && log_raw)) && sorted && perm && log_src && log_dst &&
                     log_t && arena && node_tab,
                 "tgnx_memstore_put: null pointer");
  const int vec = msg_dim > 0 && (start * msg_dim) % 4 == 0 && (B * msg_dim) % 4 == 0 && aligned16(raw_msg) &&
                  aligned16(log_raw);
  const int64_t work = std::max<int64_t>(2 * B, vec ? B * msg_dim / 4 : B * msg_dim);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(work, MS_BLOCK), MS_MAX_GRID));
  hipLaunchKernelGGL(memstore_put_k, grid, dim3(MS_BLOCK), 0, as_stream(stream), src, dst, t, raw_msg, B, msg_dim,
                     sorted, perm, start, num_nodes, log_src, log_dst, log_t, log_raw, arena, node_tab, n_bad, vec);
  TGNX_LAUNCH_CHECK("memstore_put");
  return TGNX_OK;
}

size_t tgnx_memstore_gather_ws_bytes(int64_t M) { return gather_ws_bytes(M < 0 ? 0 : M); }

int tgnx_memstore_count(const int64_t* node_tab, int64_t num_nodes, const int64_t* n_id, int64_t M,
                        const int64_t* put_bad, int64_t* totals, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(M >= 0 && num_nodes >= 0 && M < (int64_t(1) << 40), "tgnx_memstore_count: bad sizes (M %lld, "
                 "num_nodes %lld)", (long long)M, (long long)num_nodes);
  TGNX_CHECK_ARG(totals && ws && (M == 0 || (node_tab && n_id)), "tgnx_memstore_count: null pointer");
  TGNX_CHECK_ARG(aligned16(node_tab), "tgnx_memstore_count: node_tab must be 16-byte aligned");
  TGNX_CHECK_ARG(ws_bytes >= gather_ws_bytes(M), "tgnx_memstore_count: workspace too small: %zu < %zu", ws_bytes,
                 gather_ws_bytes(M));
  hipStream_t s = as_stream(stream);
  TGNX_HIP_CHECK(hipMemsetAsync(totals, 0, 3 * 8, s));
  const int64_t nt = ceil_div(M, MS_TILE);
  int64_t* tiles = reinterpret_cast<int64_t*>(ws);
  if (nt > 0) {
    hipLaunchKernelGGL(memstore_count_k, dim3((unsigned)nt), dim3(MS_BLOCK), 0, s, node_tab, num_nodes, n_id, M, tiles,
                       totals + 2);
    TGNX_LAUNCH_CHECK("memstore_count");
  }
  hipLaunchKernelGGL(memstore_scan_k, dim3(1), dim3(MS_BLOCK), 0, s, nt, tiles, totals, put_bad);
  TGNX_LAUNCH_CHECK("memstore_scan");
  return TGNX_OK;
}

int tgnx_memstore_gather(const int64_t* node_tab, int64_t num_nodes, const int64_t* arena, const int64_t* log_t,
                         int64_t fill, const int64_t* n_id, int64_t M, int64_t n_s, int64_t n_d, int64_t* out_slot,
                         int64_t* out_owner, int64_t* out_t, int64_t* out_lu, const void* ws, size_t ws_bytes,
                         void* stream) {
  TGNX_CHECK_ARG(M >= 0 && num_nodes >= 0 && fill >= 0 && n_s >= 0 && n_d >= 0 && M < (int64_t(1) << 40) &&
                     n_s <= fill && n_d <= fill,
                 "tgnx_memstore_gather: bad sizes (M %lld, fill %lld, n_s %lld, n_d %lld)", (long long)M,
                 (long long)fill, (long long)n_s, (long long)n_d);
  if (M == 0) return TGNX_OK;
  TGNX_CHECK_ARG(node_tab && n_id && out_lu && ws &&
                     (n_s + n_d == 0 || (arena && log_t && out_slot && out_owner && out_t)),
                 "tgnx_memstore_gather: null pointer");
  TGNX_CHECK_ARG(aligned16(node_tab), "tgnx_memstore_gather: node_tab must be 16-byte aligned");
  TGNX_CHECK_ARG(ws_bytes >= gather_ws_bytes(M), "tgnx_memstore_gather: workspace too small: %zu < %zu", ws_bytes,
                 gather_ws_bytes(M));
  hipLaunchKernelGGL(memstore_gather_k, dim3((unsigned)ceil_div(M, MS_TILE)), dim3(MS_BLOCK), 0, as_stream(stream),
                     node_tab, num_nodes, arena, 2 * fill, log_t, fill, n_id, M, n_s, n_d,
                     reinterpret_cast<const int64_t*>(ws), out_slot, out_owner, out_t, out_lu);
  TGNX_LAUNCH_CHECK("memstore_gather");
  return TGNX_OK;
}

int tgnx_memstore_build_msg(const int64_t* slot, int64_t n_msg, int64_t n_s, const int64_t* log_src,
                            const int64_t* log_dst, const int64_t* log_t, const float* log_raw, int64_t fill,
                            int64_t num_nodes, int64_t mem_dim, int64_t msg_dim, int64_t time_dim, const float* memory,
                            const int64_t* last_update, const float* w, const float* b, const float* emb,
                            int64_t emb_rows, const int64_t* assoc, const int64_t* stamp, const int64_t* n_id, int64_t M,
                            int32_t emb_flags, float* out, float* t_rel, void* stream) {
  TGNX_CHECK_ARG(n_msg >= 0 && n_s >= 0 && n_s <= n_msg && fill >= 0 && num_nodes >= 0 && mem_dim >= 0 &&
                     msg_dim >= 0 && time_dim >= 0 && M >= 0 && emb_rows >= 0 && n_msg < (int64_t(1) << 40) &&
                     mem_dim < (1 << 24) && msg_dim < (1 << 24) && time_dim < (1 << 24),
                 "tgnx_memstore_build_msg: bad sizes (n_msg %lld, n_s %lld, fill %lld)", (long long)n_msg,
                 (long long)n_s, (long long)fill);
  TGNX_CHECK_ARG(emb_flags >= 0 && emb_flags <= 3, "tgnx_memstore_build_msg: emb_flags must be 0..3");
  if (n_msg == 0) return TGNX_OK;
  TGNX_CHECK_ARG(slot && log_src && log_dst && log_t && (msg_dim == 0 || log_raw) && (mem_dim == 0 || memory) &&
                     last_update && (time_dim == 0 || (w && b)) && out && t_rel,
                 "tgnx_memstore_build_msg: null pointer");
  if (!emb) emb_flags = 0;
  TGNX_CHECK_ARG(emb_flags == 0 || (assoc && stamp && (M == 0 || n_id)),
                 "tgnx_memstore_build_msg: embeddings need assoc, the stamps and n_id");
  BuildArgs a;
  a.slot = slot, a.n_msg = n_msg, a.n_s = n_s;
  a.log_src = log_src, a.log_dst = log_dst, a.log_t = log_t, a.log_raw = log_raw;
  a.fill = fill, a.N = num_nodes, a.D = mem_dim, a.d = msg_dim, a.T = time_dim;
  a.memory = memory, a.last_update = last_update, a.w = w, a.b = b;
  a.emb = emb, a.E = emb_rows, a.assoc = assoc, a.stamp = stamp, a.n_id = n_id, a.M = M, a.emb_flags = emb_flags;
  a.out = out, a.t_rel = t_rel;
  // a column group moves as float4 when its rows start 16-B aligned on both sides and hold whole vectors
  const int64_t W = 2 * mem_dim + msg_dim + time_dim;
  const bool rows = W % 4 == 0 && aligned16(out);
  const bool mem = rows && mem_dim % 4 == 0 && aligned16(memory) && (emb_flags == 0 || aligned16(emb));
  a.vec = (mem ? 3 : 0) | (rows && mem_dim % 2 == 0 && msg_dim % 4 == 0 && aligned16(log_raw) ? 4 : 0) |
          (rows && (2 * mem_dim + msg_dim) % 4 == 0 && time_dim % 4 == 0 && aligned16(w) && aligned16(b) ? 8 : 0);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n_msg, MS_WAVES), MS_MAX_GRID));
  hipLaunchKernelGGL(memstore_build_k, grid, dim3(MS_BLOCK), 0, as_stream(stream), a);
  TGNX_LAUNCH_CHECK("memstore_build_msg");
  return TGNX_OK;
}

}  // extern "C"
