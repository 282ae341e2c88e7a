// Event-table compaction of the TGN engine on gfx950: retire every row of the resident event table
// that neither the neighbour ring nor a node's message store references, renumber the survivors in order
// (new id = rank among the live rows) and rewrite every holder of an event id.
//
// Two phases, because the host sizes the new allocations from one number in between:
//   plan   (5 launches, writes only the workspace)
//     compact_clear   zero the live bitmap (bit e = row e is live), stamp the record
//     compact_mark    ring slots (thread per slot), store runs (wave per node, looping over the run: a run can be
//                     longer than a wave), rows >= upto (thread per bitmap word); integer atomicOr into the bitmap.
//                     An id outside [0, num_events) is counted, never used as an index
//     compact_reduce  per workgroup of 256 bitmap words (256 nodes): the sum of popcounts (of run lengths)
//     compact_sums    one workgroup per sequence: exclusive scan of the workgroup sums in index order; the totals
//                     n_live and the live arena entry count go to the record
//     compact_prefix  per workgroup again: the exclusive prefix of every bitmap word (new id of its first live row)
//                     and of every node (start of its repacked runs)
//   The scan is multi-workgroup and fixed-order: integer sums of fixed chunks, no float, no order-dependent atomics,
//   so every output is deterministic.
//   apply  (4 launches)
//     compact_rows    src / dst / t of the live rows into the new table and kept[new] = old; a wave walks 64 bitmap
//                     words at a time, a lane per row of each nonzero word
//     compact_msg     the row gather, wave per NEW row from kept: msg rows move as float4 (16 B) pieces with a scalar
//                     tail, or scalar throughout when a row start is not 16-B aligned (msg_dim % 4 != 0)
//     compact_ring    e_id of every valid ring slot remapped in place; ctl BATCH_START = CUR_EID = n_live
//     compact_store   the node table and arena rewritten into the new store: node by node, s run then d run, from
//                     the node prefix; counts unchanged, empty runs at offset 0
//   Every apply kernel first checks the record (made for this table, no bad id, the new allocations hold the live
//   rows) and returns without a store otherwise; all stores are ordinary vector stores.
#include <algorithm>

#include "tgnx_common.h"

using namespace tgnx;

namespace {

constexpr int CT = 256;                       // workgroup size; the scan's chunk: 256 bitmap words = 8192 rows
constexpr int64_t REC_MAGIC = 0x74676e78636d70ll;
constexpr int64_t MAX_GRID = 2048;            // grid-stride kernels: 8 workgroups per CU cover the 256 CUs
// record words (int64, the head of the workspace)
enum { REC_LIVE = 0, REC_ARENA = 1, REC_BAD = 2, REC_NEV = 4, REC_UPTO = 5, REC_MAGIC_W = 6, REC_WORDS = 8 };

struct WsLay {
  size_t bm, wpre, npre, bsum, total;
  int64_t W;      // bitmap words
  int nbw, nbn;   // scan workgroups over the words / the nodes
};

size_t carve(size_t& off, size_t bytes) {
  const size_t at = off;
  off += (bytes + 255) & ~(size_t)255;
  return at;
}

WsLay make_lay(int64_t N, int64_t nev) {
  WsLay L;
  L.W = (nev + 31) / 32;
  L.nbw = (int)((L.W + CT - 1) / CT);
  L.nbn = (int)((N + CT - 1) / CT);
  size_t off = 0;
  carve(off, REC_WORDS * 8);
  L.bm = carve(off, (size_t)std::max<int64_t>(L.W, 1) * 4);
  L.wpre = carve(off, (size_t)std::max<int64_t>(L.W, 1) * 4);
  L.npre = carve(off, (size_t)N * 4);
  L.bsum = carve(off, (size_t)(L.nbw + L.nbn + 1) * 4);
  L.total = off;
  return L;
}

// a store run {off, cnt} that can be walked: non-empty and inside the arena words the table's valid rows can own
__device__ __forceinline__ bool run_ok(int64_t off, int64_t cnt, int64_t lim) {
  return cnt > 0 && off >= 0 && cnt <= lim && off <= lim - cnt;
}

__device__ __forceinline__ int64_t remap(const uint32_t* __restrict__ bm, const int* __restrict__ wpre, int64_t e) {
  return (int64_t)wpre[e >> 5] + __popc(bm[e >> 5] & ((1u << (e & 31)) - 1u));
}

__global__ void __launch_bounds__(CT) compact_clear(uint32_t* __restrict__ bm, int64_t W, int64_t* __restrict__ rec,
                                                    int64_t nev, int64_t upto) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < W; i += nt) bm[i] = 0u;
  if (tid < REC_WORDS) rec[tid] = tid == REC_NEV ? nev : tid == REC_UPTO ? upto : tid == REC_MAGIC_W ? REC_MAGIC : 0;
}

__global__ void __launch_bounds__(CT) compact_mark(const int64_t* __restrict__ nbr, const int64_t* __restrict__ eid,
                                                   int64_t NK, const int64_t* __restrict__ st,
                                                   const int64_t* __restrict__ arena, int64_t N, int64_t nev,
                                                   int64_t upto, uint32_t* __restrict__ bm, int64_t W,
                                                   int64_t* __restrict__ rec) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id();
  unsigned long long bad = 0;
  for (int64_t i = tid; i < NK; i += nt) {
    if (nbr[i] == -1) continue;
    const int64_t e = eid[i];
    if (e < 0 || e >= nev) ++bad;
    else atomicOr(&bm[e >> 5], 1u << (e & 31));
  }
  const int64_t lim = 2 * nev;
  for (int64_t v = tid >> 6; v < N; v += nt >> 6) {   // wave per node
    for (int dir = 0; dir < 2; ++dir) {
      const int64_t off = st[4 * v + 2 * dir], cnt = st[4 * v + 2 * dir + 1];
      if (cnt == 0) continue;
      if (!run_ok(off, cnt, lim)) {
        if (lane == 0) ++bad;
        continue;
      }
      for (int64_t k = lane; k < cnt; k += WAVE) {
        const int64_t e = arena[off + k];
        if (e < 0 || e >= nev) ++bad;
        else atomicOr(&bm[e >> 5], 1u << (e & 31));
      }
    }
  }
  for (int64_t w = (upto >> 5) + tid; w < W; w += nt) {   // rows [upto, nev): kept verbatim
    const int64_t lo = w * 32;
    uint32_t m = ~0u;
    if (upto > lo) m &= ~0u << (int)(upto - lo);
    if (nev < lo + 32) m &= (1u << (int)(nev - lo)) - 1u;
    if (m) atomicOr(&bm[w], m);
  }
  if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(rec + REC_BAD), bad);
}

// the scanned sequences: popcount of bitmap word i; walkable run length s + d of node i
__device__ __forceinline__ int scan_val(bool words, int64_t i, const uint32_t* __restrict__ bm, int64_t W,
                                        const int64_t* __restrict__ st, int64_t N, int64_t lim) {
  if (words) return i < W ? __popc(bm[i]) : 0;
  if (i >= N) return 0;
  const int64_t so = st[4 * i], sc = st[4 * i + 1], dof = st[4 * i + 2], dc = st[4 * i + 3];
  return (int)((run_ok(so, sc, lim) ? sc : 0) + (run_ok(dof, dc, lim) ? dc : 0));
}

__global__ void __launch_bounds__(CT) compact_reduce(const uint32_t* __restrict__ bm, int64_t W, int nbw,
                                                     const int64_t* __restrict__ st, int64_t N, int64_t lim,
                                                     int* __restrict__ bsum) {
  __shared__ int sh[20];
  const int b = blockIdx.x;
  const bool words = b < nbw;
  const int64_t i = (int64_t)(words ? b : b - nbw) * CT + threadIdx.x;
  int tot;
  block_excl_scan(scan_val(words, i, bm, W, st, N, lim), sh, &tot);
  if (threadIdx.x == 0) bsum[b] = tot;
}

// workgroup 0: the bitmap's workgroup sums, workgroup 1: the nodes'; chunks of 256 in index order with a carry
__global__ void __launch_bounds__(CT) compact_sums(int* __restrict__ bsum, int nbw, int nbn, int64_t* __restrict__ rec) {
  __shared__ int sh[20];
  const int part = blockIdx.x, base = part ? nbw : 0, n = part ? nbn : nbw;
  int carry = 0;
  for (int c = 0; c < n; c += CT) {
    const int i = c + threadIdx.x;
    int tot;
    const int ex = block_excl_scan(i < n ? bsum[base + i] : 0, sh, &tot);
    if (i < n) bsum[base + i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) rec[part ? REC_ARENA : REC_LIVE] = carry;
}

__global__ void __launch_bounds__(CT) compact_prefix(const uint32_t* __restrict__ bm, int64_t W, int nbw,
                                                     const int64_t* __restrict__ st, int64_t N, int64_t lim,
                                                     const int* __restrict__ bsum, int* __restrict__ wpre,
                                                     int* __restrict__ npre) {
  __shared__ int sh[20];
  const int b = blockIdx.x;
  const bool words = b < nbw;
  const int64_t i = (int64_t)(words ? b : b - nbw) * CT + threadIdx.x;
  int tot;
  const int ex = block_excl_scan(scan_val(words, i, bm, W, st, N, lim), sh, &tot);
  if (words) {
    if (i < W) wpre[i] = bsum[b] + ex;
  } else if (i < N) {
    npre[i] = bsum[b] + ex;
  }
}

// the plan in the workspace is for this table, found no bad id, and the new allocations hold what it keeps
__device__ __forceinline__ bool apply_ok(const int64_t* __restrict__ rec, int64_t nev, int64_t new_cap, int64_t kept_len) {
  return rec[REC_MAGIC_W] == REC_MAGIC && rec[REC_NEV] == nev && rec[REC_BAD] == 0 && rec[REC_LIVE] >= 0 &&
         rec[REC_LIVE] <= new_cap && rec[REC_LIVE] <= kept_len && rec[REC_ARENA] >= 0 && rec[REC_ARENA] <= 2 * new_cap;
}

__device__ __forceinline__ void copy_row(const float* __restrict__ s, float* __restrict__ q, int d, int lane) {
  if ((((uintptr_t)s | (uintptr_t)q) & 15) == 0) {   // (wave-uniform)
    const int d4 = d >> 2;
    for (int k = lane; k < d4; k += WAVE) reinterpret_cast<float4*>(q)[k] = reinterpret_cast<const float4*>(s)[k];
    for (int k = (d4 << 2) + lane; k < d; k += WAVE) q[k] = s[k];
  } else {
    for (int k = lane; k < d; k += WAVE) q[k] = s[k];
  }
}

__global__ void __launch_bounds__(CT) compact_rows(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                   const float* __restrict__ t, int64_t nev, const uint32_t* __restrict__ bm,
                                                   const int* __restrict__ wpre, int64_t W,
                                                   const int64_t* __restrict__ rec, int64_t new_cap, int64_t kept_len,
                                                   int64_t* __restrict__ nsrc, int64_t* __restrict__ ndst,
                                                   float* __restrict__ nt_, int64_t* __restrict__ kept) {
  if (!apply_ok(rec, nev, new_cap, kept_len)) return;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id();
  const int64_t n_live = rec[REC_LIVE];
  for (int64_t c = (tid >> 6) * WAVE; c < W; c += (nt >> 6) * WAVE) {   // 64 bitmap words per wave and round
    const int64_t i = c + lane;
    const uint32_t w = i < W ? bm[i] : 0u;
    const int p = i < W ? wpre[i] : 0;
    unsigned long long nz = __ballot(w != 0u);
    while (nz) {
      const int j = __ffsll(nz) - 1;
      nz &= nz - 1;
      const uint32_t wj = (uint32_t)__shfl((int)w, j, WAVE);
      const int64_t pj = __shfl(p, j, WAVE), row0 = (c + j) * 32;
      if (lane < 32 && ((wj >> lane) & 1u)) {
        const int64_t o = row0 + lane, n = pj + __popc(wj & ((1u << lane) - 1u));
        if (o < nev && n < n_live) {
          nsrc[n] = src[o];
          ndst[n] = dst[o];
          nt_[n] = t[o];
          kept[n] = o;
        }
      }
    }
  }
}

// the row gather, parallel over the NEW rows (wave per row, after compact_rows wrote kept)
__global__ void __launch_bounds__(CT) compact_msg(const float* __restrict__ msg, int d, int64_t nev,
                                                  const int64_t* __restrict__ rec, int64_t new_cap, int64_t kept_len,
                                                  const int64_t* __restrict__ kept, float* __restrict__ nmsg) {
  if (!apply_ok(rec, nev, new_cap, kept_len)) return;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id();
  const int64_t n_live = rec[REC_LIVE];
  for (int64_t n = tid >> 6; n < n_live; n += nt >> 6) {
    const int64_t o = kept[n];
    if (o >= 0 && o < nev) copy_row(msg + o * d, nmsg + n * d, d, lane);
  }
}

__global__ void __launch_bounds__(CT) compact_ring(const int64_t* __restrict__ nbr, int64_t* __restrict__ eid, int64_t NK,
                                                   int64_t nev, const uint32_t* __restrict__ bm,
                                                   const int* __restrict__ wpre, const int64_t* __restrict__ rec,
                                                   int64_t new_cap, int64_t kept_len, int64_t* __restrict__ ctl) {
  if (!apply_ok(rec, nev, new_cap, kept_len)) return;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < NK; i += nt) {
    if (nbr[i] == -1) continue;
    const int64_t e = eid[i];
    if (e >= 0 && e < nev) eid[i] = remap(bm, wpre, e);
  }
  if (tid == 0) {
    ctl[TGNX_CTL_BATCH_START] = rec[REC_LIVE];
    ctl[TGNX_CTL_CUR_EID] = rec[REC_LIVE];
  }
}

__global__ void __launch_bounds__(CT) compact_store(const int64_t* __restrict__ st, const int64_t* __restrict__ arena,
                                                    int64_t N, int64_t nev, const uint32_t* __restrict__ bm,
                                                    const int* __restrict__ wpre, const int* __restrict__ npre,
                                                    const int64_t* __restrict__ rec, int64_t new_cap, int64_t kept_len,
                                                    int64_t* __restrict__ nst, int64_t* __restrict__ narena) {
  if (!apply_ok(rec, nev, new_cap, kept_len)) return;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id();
  const int64_t lim = 2 * nev;
  for (int64_t v = tid >> 6; v < N; v += nt >> 6) {   // wave per node
    const int64_t so = st[4 * v], dof = st[4 * v + 2];
    int64_t sc = st[4 * v + 1], dc = st[4 * v + 3];
    if (!run_ok(so, sc, lim)) sc = 0;
    if (!run_ok(dof, dc, lim)) dc = 0;
    const int64_t base = npre[v];
    if (base < 0 || base + sc + dc > 2 * new_cap) sc = dc = 0;
    if (lane == 0) {
      nst[4 * v] = sc ? base : 0;
      nst[4 * v + 1] = sc;
      nst[4 * v + 2] = dc ? base + sc : 0;
      nst[4 * v + 3] = dc;
    }
    for (int64_t k = lane; k < sc; k += WAVE) {
      const int64_t e = arena[so + k];
      narena[base + k] = e >= 0 && e < nev ? remap(bm, wpre, e) : 0;
    }
    for (int64_t k = lane; k < dc; k += WAVE) {
      const int64_t e = arena[dof + k];
      narena[base + sc + k] = e >= 0 && e < nev ? remap(bm, wpre, e) : 0;
    }
  }
}

unsigned grid_for(int64_t work_items) {
  return (unsigned)std::min<int64_t>(MAX_GRID, std::max<int64_t>(1, (work_items + CT - 1) / CT));
}

int check_args(const char* who, const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* b, int64_t num_events,
               const void* ws, size_t ws_bytes, WsLay& L) {
  TGNX_CHECK_ARG(cfg, "%s: null config", who);
  TGNX_CHECK_ARG(cfg->num_nodes > 0 && cfg->num_nodes < (1ll << 31) && cfg->ring > 0 && cfg->msg_dim >= 0 &&
                     cfg->num_events > 0,
                 "%s: bad num_nodes / ring / msg_dim / num_events", who);
  TGNX_CHECK_ARG(num_events >= 0 && num_events <= cfg->num_events,
                 "%s: %lld valid rows outside the table's capacity %lld", who, (long long)num_events,
                 (long long)cfg->num_events);
  if (num_events >= (1ll << 30)) {
    set_error("%s: %lld rows: the 32-bit prefix holds fewer than 2^30", who, (long long)num_events);
    return TGNX_ETOOBIG;
  }
  TGNX_CHECK_ARG(b && b->ctl && b->nbr && b->eid && b->store, "%s: null buffer (ctl / nbr / eid / store)", who);
  L = make_lay(cfg->num_nodes, num_events);
  TGNX_CHECK_ARG(ws && ws_bytes >= L.total && ((uintptr_t)ws & 15) == 0,
                 "%s: workspace of tgnx_tgn_compact_ws_bytes(...) = %zu bytes, 16-B aligned", who, L.total);
  return TGNX_OK;
}

}  // namespace

extern "C" {

size_t tgnx_tgn_compact_ws_bytes(const tgnx_tgn_config* cfg, int64_t num_events) {
  if (!cfg || cfg->num_nodes <= 0 || cfg->num_nodes >= (1ll << 31) || num_events < 0 || num_events >= (1ll << 30)) {
    set_error("tgnx_tgn_compact_ws_bytes: bad config / row count");
    return 0;
  }
  return make_lay(cfg->num_nodes, num_events).total;
}

int tgnx_tgn_compact_plan(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events, int64_t upto,
                          void* ws, size_t ws_bytes, void* stream) {
  WsLay L;
  int rc = check_args("tgnx_tgn_compact_plan", cfg, buf, num_events, ws, ws_bytes, L);
  if (rc) return rc;
  TGNX_CHECK_ARG(upto >= 0 && upto <= num_events, "tgnx_tgn_compact_plan: upto = %lld outside [0, %lld]",
                 (long long)upto, (long long)num_events);
  char* w = reinterpret_cast<char*>(ws);
  int64_t* rec = reinterpret_cast<int64_t*>(w);
  uint32_t* bm = reinterpret_cast<uint32_t*>(w + L.bm);
  int* wpre = reinterpret_cast<int*>(w + L.wpre);
  int* npre = reinterpret_cast<int*>(w + L.npre);
  int* bsum = reinterpret_cast<int*>(w + L.bsum);
  const int64_t N = cfg->num_nodes, NK = N * cfg->ring;
  const int64_t* st = buf->store;
  const int64_t* arena = buf->store + 4 * N;
  hipStream_t s = as_stream(stream);
  compact_clear<<<grid_for(L.W), CT, 0, s>>>(bm, L.W, rec, num_events, upto);
  TGNX_LAUNCH_CHECK("compact_clear");
  compact_mark<<<grid_for(std::max(NK, N * WAVE)), CT, 0, s>>>(buf->nbr, buf->eid, NK, st, arena, N, num_events, upto,
                                                                bm, L.W, rec);
  TGNX_LAUNCH_CHECK("compact_mark");
  const unsigned nb = (unsigned)(L.nbw + L.nbn);
  compact_reduce<<<nb, CT, 0, s>>>(bm, L.W, L.nbw, st, N, 2 * num_events, bsum);
  TGNX_LAUNCH_CHECK("compact_reduce");
  compact_sums<<<2, CT, 0, s>>>(bsum, L.nbw, L.nbn, rec);
  TGNX_LAUNCH_CHECK("compact_sums");
  compact_prefix<<<nb, CT, 0, s>>>(bm, L.W, L.nbw, st, N, 2 * num_events, bsum, wpre, npre);
  TGNX_LAUNCH_CHECK("compact_prefix");
  return TGNX_OK;
}

int tgnx_tgn_compact_apply(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events,
                           int64_t new_capacity, int64_t* new_src, int64_t* new_dst, float* new_t, float* new_msg,
                           int64_t* new_store, int64_t* kept, int64_t kept_len, const void* ws, size_t ws_bytes,
                           void* stream) {
  WsLay L;
  int rc = check_args("tgnx_tgn_compact_apply", cfg, buf, num_events, ws, ws_bytes, L);
  if (rc) return rc;
  TGNX_CHECK_ARG(buf->ev_src && buf->ev_dst && buf->ev_t && buf->ev_msg, "tgnx_tgn_compact_apply: null event table");
  TGNX_CHECK_ARG(new_capacity > 0 && new_capacity < (1ll << 30) && kept_len >= 0,
                 "tgnx_tgn_compact_apply: bad new capacity / kept length");
  TGNX_CHECK_ARG(new_src && new_dst && new_t && new_msg && new_store && kept,
                 "tgnx_tgn_compact_apply: null output (new table / new store / kept)");
  const char* w = reinterpret_cast<const char*>(ws);
  const int64_t* rec = reinterpret_cast<const int64_t*>(w);
  const uint32_t* bm = reinterpret_cast<const uint32_t*>(w + L.bm);
  const int* wpre = reinterpret_cast<const int*>(w + L.wpre);
  const int* npre = reinterpret_cast<const int*>(w + L.npre);
  const int64_t N = cfg->num_nodes, NK = N * cfg->ring;
  hipStream_t s = as_stream(stream);
  compact_rows<<<grid_for(L.W), CT, 0, s>>>(buf->ev_src, buf->ev_dst, buf->ev_t, num_events, bm, wpre, L.W, rec,
                                           new_capacity, kept_len, new_src, new_dst, new_t, kept);
  TGNX_LAUNCH_CHECK("compact_rows");
  // (the grid is sized by the old row count, an upper bound of n_live, which only the device knows)
  compact_msg<<<grid_for(std::min(num_events, kept_len) * WAVE), CT, 0, s>>>(buf->ev_msg, cfg->msg_dim, num_events, rec,
                                                                            new_capacity, kept_len, kept, new_msg);
  TGNX_LAUNCH_CHECK("compact_msg");
  compact_store<<<grid_for(N * WAVE), CT, 0, s>>>(buf->store, buf->store + 4 * N, N, num_events, bm, wpre, npre, rec,
                                                  new_capacity, kept_len, new_store, new_store + 4 * N);
  TGNX_LAUNCH_CHECK("compact_store");
  compact_ring<<<grid_for(NK), CT, 0, s>>>(buf->nbr, buf->eid, NK, num_events, bm, wpre, rec, new_capacity, kept_len,
                                          buf->ctl);
  TGNX_LAUNCH_CHECK("compact_ring");
  return TGNX_OK;
}

}  // extern "C"
