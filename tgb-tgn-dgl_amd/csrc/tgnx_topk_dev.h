// Device and host pieces shared by the selection kernels of csrc/tgnx_topk.hip (LinkPredictor top-k / rank) and
// csrc/tgnx_knn.hip (embedding-space nearest neighbours): the tile and chunk constants, the workspace layout
// (carve_ws), the exclusion-by-key staging (stage_filter / excluded_mask), the chunk select (select_chunk) and the exact
// merge of the partial lists (topk_merge / launch_merge).  Written once; each including file gets its own copy of
// the kernels in its anonymous namespace.  The selection order, the padding and the clamping rules are described in
// tgnx_topk.hip's header and include/tgnx.h.
#pragma once
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "tgnx_common.h"

using namespace tgnx;

namespace {

constexpr int TK_BLOCK = 256;
constexpr int TK_TQ = 16;        // sources per workgroup (four per wave in the select)
constexpr int TK_CHUNK_MIN = 256, TK_CHUNK_MAX = 512;  // candidates per workgroup (LDS: 16 x chunk logits, <= 32 KB)
constexpr int64_t TK_DMAX = 256;
constexpr int TK_G = 4;          // 16-B vectors of a candidate's Hd row per load group (two groups in registers)
constexpr int TK_EXCAP = 1024;  // exclusion keys of a source tile staged in LDS (8 KB; above: searched in global memory)
constexpr int TK_LCHUNK = 256;  // list entries per workgroup of the per-source-list kernel (one per thread)
constexpr int TK_MTILE = 896;    // partial entries per merge pass (+ the running list: 1024 entries, 8 KB per wave)

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
int64_t ld_of(int64_t D) { return (D + 3) & ~int64_t(3); }
// 512 candidates per workgroup (half the select rounds per candidate) once that still gives every CU a workgroup
int chunk_of(int64_t n_src, int64_t n_cand) {
  return ceil_div(n_src, TK_TQ) * ceil_div(n_cand, TK_CHUNK_MAX) >= 256 ? TK_CHUNK_MAX : TK_CHUNK_MIN;
}

// partial lists per source.  Dense: sized for the smaller chunk (the larger count), so the size is monotone in n_cand
int64_t dense_lists(int64_t n_cand) { return ceil_div(n_cand, TK_CHUNK_MIN); }

// The workspace of every entry point: Hs, Hd, `lists` partial lists of k (value, position) per source (rank: none),
// then the GEMM scratch from `used` on.
struct TopkWs {
  float *hs, *hd, *pval;
  int* pidx;
  char* gemm;
  size_t used;
};
TopkWs carve_ws(void* ws, int64_t n_src, int64_t n_cand, int64_t D, int32_t k, int64_t lists) {
  const int64_t ldh = ld_of(D);
  char* p = reinterpret_cast<char*>(ws);
  size_t off = 0;
  TopkWs w;
  w.hs = reinterpret_cast<float*>(p + off);
  off += align256((size_t)n_src * ldh * 4);
  w.hd = reinterpret_cast<float*>(p + off);
  off += align256((size_t)n_cand * ldh * 4);
  w.pval = reinterpret_cast<float*>(p + off);
  off += align256((size_t)n_src * lists * k * 4);
  w.pidx = reinterpret_cast<int*>(p + off);
  off += align256((size_t)n_src * lists * k * 4);
  w.gemm = p + off;
  w.used = off;
  return w;
}

constexpr float TK_QNAN = __builtin_bit_cast(float, 0x7fc00000);  // the quiet NaN of skipped and excluded entries

// the pick after (pv, pj) in the order among a lane's entries (v, j): larger v, then smaller j
__device__ __forceinline__ bool after(float v, int j, float pv, int pj) { return v < pv || (v == pv && j > pj); }
// the wave's best (value, position) from every lane's best (position INT_MAX: none); every lane gets it
__device__ __forceinline__ void wave_best(float& bv, int& bj) {
  const float m = wave_max_f(bv);
  bj = wave_min_i(bv == m ? bj : INT_MAX);
  bv = m;
}

// Per-source exclusions by key (tgnx_link_predictor_topk_filtered): candidate c is out for source q when its key
// (cand_key[c], or c itself) equals src_key[q] or occurs in excl_key[excl_ptr[q] : excl_ptr[q + 1]] (ascending).
struct TopkFilter {
  const int64_t *cand_key, *src_key, *excl_ptr, *excl_key;
  int64_t nnz;
};
// LDS of the filtered kernels (stage_filter): the tile's exclusion segments when they fit, their bounds, the source keys
struct TopkFilterLds {
  int64_t key[TK_EXCAP];
  int64_t lo[TK_TQ], hi[TK_TQ], skey[TK_TQ];
  int off[TK_TQ];
  int has_skey[TK_TQ];
  int staged;
};
__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// key in a[lo, hi)?  A lower bound that never leaves [lo, hi), whatever the segment holds
template <typename Int>
__device__ __forceinline__ bool seg_has(const int64_t* a, Int lo, Int hi, int64_t key) {
  Int n = hi - lo;
  while (n > 0) {
    const Int half = n >> 1;
    if (a[lo + half] < key) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo < hi && a[lo] == key;
}

// The tile's segments, their pointers clamped into [0, nnz] and a decreasing pair read as empty: whatever excl_ptr
// holds, no read leaves excl_key.  Staged in LDS when the tile's keys fit (ring rows: 16 x <= 32), searched in global
// memory otherwise.  (Two barriers inside; the caller's barrier after stage_tile publishes the keys.)
__device__ __forceinline__ void stage_filter(TopkFilterLds* X, const TopkFilter& f, int64_t q0, int nq, int tid) {
  if (tid < TK_TQ) {
    int64_t lo = 0, hi = 0;
    if (f.excl_ptr && tid < nq) {
      lo = clamp64(f.excl_ptr[q0 + tid], 0, f.nnz);
      hi = max(lo, clamp64(f.excl_ptr[q0 + tid + 1], 0, f.nnz));
    }
    X->lo[tid] = lo;
    X->hi[tid] = hi;
    X->has_skey[tid] = f.src_key && tid < nq;
    X->skey[tid] = (f.src_key && tid < nq) ? f.src_key[q0 + tid] : 0;
  }
  __syncthreads();
  if (tid == 0) {
    int64_t tot = 0;
    for (int i = 0; i < TK_TQ; ++i) {
      X->off[i] = (int)min(tot, (int64_t)TK_EXCAP);
      tot += X->hi[i] - X->lo[i];
    }
    X->staged = tot <= TK_EXCAP;
  }
  __syncthreads();
  if (X->staged)
    for (int i = 0; i < TK_TQ; ++i) {
      const int64_t lo = X->lo[i];
      const int len = (int)(X->hi[i] - lo), off = X->off[i];
      for (int x = tid; x < len; x += TK_BLOCK) X->key[off + x] = f.excl_key[lo + x];
    }
}
// bit i: the candidate with key ck is out for the tile's source i
__device__ __forceinline__ unsigned excluded_mask(const TopkFilterLds* X, const TopkFilter& f, int nq, int64_t ck) {
  unsigned excl = 0;
  const bool staged = X->staged;
  for (int i = 0; i < nq; ++i) {
    bool out = X->has_skey[i] && X->skey[i] == ck;
    const int64_t lo = X->lo[i], hi = X->hi[i];
    if (!out && hi > lo)
      out = staged ? seg_has<int>(X->key, X->off[i], X->off[i] + (int)(hi - lo), ck)
                   : seg_has<int64_t>(f.excl_key, lo, hi, ck);
    excl |= (unsigned)out << i;
  }
  return excl;
}

// A wave's k rounds of pick-after-previous over QW rows of logits in LDS (row u at L + u * stride, entries
// [0, nvalid)), side by side: QW independent scan / reduce chains per round.  Row u < nrows is source row0 + u, whose
// partial list for chunk cj gets the picks in order, positions offset by pos0; none left: (-inf, -1), the padding.
template <int QW>
__device__ __forceinline__ void select_chunk(const float* L, int stride, int nvalid, int k, int lane, int64_t row0,
                                             int nrows, int nc, int64_t cj, int pos0, float* __restrict__ pval,
                                             int* __restrict__ pidx) {
  float pv[QW];
  int pj[QW];
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    pv[u] = INFINITY;
    pj[u] = -1;
  }
  for (int r = 0; r < k; ++r) {
    float bv[QW];
    int bj[QW];
#pragma unroll
    for (int u = 0; u < QW; ++u) {
      bv[u] = -INFINITY;
      bj[u] = INT_MAX;
    }
    for (int j = lane; j < nvalid; j += WAVE) {  // j ascends: the first of a lane's equal values stays
#pragma unroll
      for (int u = 0; u < QW; ++u) {
        const float v = L[u * stride + j];
        if (after(v, j, pv[u], pj[u]) && (v > bv[u] || bj[u] == INT_MAX)) {
          bv[u] = v;
          bj[u] = j;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < QW; ++u) {
      wave_best(bv[u], bj[u]);
      if (lane == 0 && u < nrows) {
        pval[((row0 + u) * nc + cj) * k + r] = bj[u] == INT_MAX ? -INFINITY : L[u * stride + bj[u]];
        pidx[((row0 + u) * nc + cj) * k + r] = bj[u] == INT_MAX ? -1 : pos0 + bj[u];
      }
      pv[u] = bv[u];
      pj[u] = bj[u];
    }
  }
}

// Wave per source: the k best of its nc chunk lists (k entries each, sorted in the order, position -1: the padding
// at the tail of a short chunk's list), then padding.  A k-way merge by list heads: the lists are staged in LDS,
// TK_MTILE / k of them per pass beside the running list of the picks so far (itself sorted; one pass at the wiki
// shape: 37 lists of 10), a lane looks at the heads of its lists, the wave picks the best head and its lane advances
// that list.  A round costs lists / 64 head reads and one reduction whatever k is.  (Rescanning every staged entry
// per round was k times that: 1.2 ms at k = 128 over 37 chunks; scanning the lists in global memory paid a dependent
// L2 round trip per round.)
__global__ void __launch_bounds__(TK_BLOCK) topk_merge(int64_t n_src, int nc, int k, const float* __restrict__ pval,
                                                       const int* __restrict__ pidx, int sigmoid,
                                                       float* __restrict__ out_val, int64_t* __restrict__ out_idx) {
  constexpr int WPB = TK_BLOCK / WAVE, CAP = TGNX_TOPK_MAX + TK_MTILE;
  __shared__ float sv[WPB][CAP];
  __shared__ int si[WPB][CAP];
  __shared__ int sh[WPB][TK_MTILE + 1];  // list heads: [0] the running list, [1 + l] the pass's list l
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t q = blockIdx.x * (int64_t)WPB + wv;
  const bool live = q < n_src;  // (wave-uniform; a dead wave keeps the block's barriers)
  const float* v0 = pval + (live ? q : 0) * (int64_t)nc * k;
  const int* j0 = pidx + (live ? q : 0) * (int64_t)nc * k;
  float* V = sv[wv];
  int* I = si[wv];
  int* H = sh[wv];
  for (int x = lane; x < TGNX_TOPK_MAX; x += WAVE) I[x] = -1;  // the running list: empty
  float kv[2] = {-INFINITY, -INFINITY};  // this lane's picks r = lane, lane + 64 of the latest pass
  int kj[2] = {INT_MAX, INT_MAX};
  const int lpt = TK_MTILE / k;  // lists per pass (>= 7)
  for (int c0 = 0; c0 == 0 || c0 < nc; c0 += lpt) {  // (block-uniform; nc = 0: one pass over nothing)
    const int nl = max(0, min(lpt, nc - c0)), nt = nl * k;
    const int64_t t0 = (int64_t)c0 * k;
    for (int x0 = lane; x0 < nt; x0 += 4 * WAVE) {  // four entries per lane in flight
      float tv[4];
      int tj[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int x = x0 + u * WAVE;
        const bool ok = live && x < nt;
        tv[u] = ok ? v0[t0 + x] : 0.f;
        tj[u] = ok ? j0[t0 + x] : -1;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int x = x0 + u * WAVE;
        if (x < nt) {
          V[TGNX_TOPK_MAX + x] = tv[u];
          I[TGNX_TOPK_MAX + x] = tj[u];
        }
      }
    }
    for (int l = lane; l <= nl; l += WAVE) H[l] = 0;
    __syncthreads();
    for (int r = 0; r < k; ++r) {
      float bv = -INFINITY;
      int bj = INT_MAX, bl = 0;
      for (int l = lane; l <= nl; l += WAVE) {
        const int h = H[l];
        const int e = l == 0 ? min(h, TGNX_TOPK_MAX - 1) : TGNX_TOPK_MAX + (l - 1) * k + min(h, k - 1);
        const int j = h < k ? I[e] : -1;
        const float v = V[e];
        if (j >= 0 && (bj == INT_MAX || v > bv || (v == bv && j < bj))) {
          bv = v;
          bj = j;
          bl = l;
        }
      }
      const float bx = bv;  // the entry's own value (-0 / +0 compare equal: the reduced max may be the other)
      const int mine = bj;
      wave_best(bv, bj);
      const unsigned long long who = __ballot(mine == bj && bj != INT_MAX);  // (positions are distinct: one lane)
      const int wl = who ? __ffsll((long long)who) - 1 : 0;
      const float val = who ? lane_f(bx, wl) : -INFINITY;
      if (who && lane == wl) H[bl] += 1;
      if (lane == (r & 63)) {
        kv[r >> 6] = val;
        kj[r >> 6] = bj;
      }
    }
    __syncthreads();  // every read of this pass is done: the picks (sorted) become the running list
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (lane + 64 * h < k) {
        V[lane + 64 * h] = kv[h];
        I[lane + 64 * h] = kj[h] == INT_MAX ? -1 : kj[h];
      }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = lane + 64 * h;
    if (!live || r >= k) continue;
    const bool none = kj[h] == INT_MAX;
    out_val[q * k + r] = none ? (sigmoid ? 0.f : -INFINITY) : (sigmoid ? 1.f / (1.f + expf(-kv[h])) : kv[h]);
    out_idx[q * k + r] = none ? -1 : kj[h];
  }
}

// out_val / out_idx = the k best of every source's nc partial lists (nc = 0: every slot is padding)
int launch_merge(hipStream_t s, int64_t n_src, int64_t nc, int32_t k, const TopkWs& w, int32_t sigmoid, float* out_val,
                 int64_t* out_idx) {
  hipLaunchKernelGGL(topk_merge, dim3((unsigned)ceil_div(n_src, TK_BLOCK / WAVE)), dim3(TK_BLOCK), 0, s, n_src, (int)nc,
                     (int)k, (const float*)w.pval, (const int*)w.pidx, (int)sigmoid, out_val, out_idx);
  TGNX_LAUNCH_CHECK("topk_merge");
  return TGNX_OK;
}

}  // namespace
