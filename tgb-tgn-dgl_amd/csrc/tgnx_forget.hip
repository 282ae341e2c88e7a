// Forgetting nodes of the TGN engine on gfx950: make the rows of a node set F what a never-seen
// node has, and remove every stored reference to F from the other nodes' ring rows and message-store runs, in place.
//
// Two phases, so that a bad id leaves everything untouched and the call costs one host read:
//   plan   (3 launches, writes only the workspace [record | N-bit bitmap of F | one "row touched" byte per node])
//     forget_clear   zero the bitmap and the bytes, stamp the record
//     forget_mark    a thread per id: integer atomicOr into the bitmap (the thread that sets a bit counts the node);
//                    an id outside [0, N) is counted as bad and skipped
//     forget_count   one pass over the ring (the row layout below) and one over the runs (wave per node, looping
//                    over a run in chunks of 64): ring slots to remove, ring rows that lose one (their byte is set),
//                    store entries to drop, bad ids.  Integer sums: the record does not depend on the launch shape
//   apply  (2 launches; each checks the record first and stores nothing unless it is this state's clean plan)
//     forget_ring    rows that lose a slot and rows of F are rewritten, nothing else is stored
//     forget_store   wave per node: runs of u not in F are packed in place, rows of F get their reset words
//   Ring layout of both passes: a wave owns R = 64 / K consecutive rows, lane l holds slot l % K of row l / K, so the
//   R * K active lanes of a wave, and consecutive waves, read consecutive 8-byte words; a row never straddles a wave
//   and its survivors' positions are a ballot and a popcount of the keep mask under the row's lanes.  No cursor
//   atomics; all stores are ordinary vector stores.
//   A slot is valid when e_id >= 0 and nbr != -1 (reset_state leaves stale nbr under e_id = -1; compaction tests
//   nbr, the embedding table e_id: both must hold here).
#include <algorithm>

#include "tgnx_common.h"
#include "tgnx_ring_dev.h"

using namespace tgnx;

namespace {

constexpr int FT = 256;              // workgroup size
constexpr int64_t MAX_GRID = 2048;   // grid-stride kernels: 8 workgroups per CU cover the 256 CUs
constexpr int64_t REC_MAGIC = 0x74676e7866726774ll;
// record words (int64, the head of the workspace)
enum { REC_NODES = 0, REC_SLOTS = 1, REC_ROWS = 2, REC_ENTRIES = 3, REC_BAD = 4, REC_N = 5, REC_NEV = 6,
       REC_MAGIC_W = 7, REC_WORDS = 8 };
constexpr int64_t NO_TABLE = INT64_MAX;   // num_events of a ring without an event table (no upper bound on e_id)

struct WsLay {
  size_t bm, rowf, total;
  int64_t W;   // bitmap words
};

WsLay make_lay(int64_t N) {
  WsLay L;
  L.W = (N + 31) / 32;
  L.bm = REC_WORDS * 8;
  L.rowf = L.bm + (((size_t)L.W * 4 + 15) & ~(size_t)15);
  L.total = L.rowf + (((size_t)N + 15) & ~(size_t)15);
  return L;
}

typedef unsigned long long u64;

__device__ __forceinline__ bool in_f(const uint32_t* __restrict__ bm, int64_t N, int64_t v) {
  return v >= 0 && v < N && ((bm[v >> 5] >> (v & 31)) & 1u);
}

__device__ __forceinline__ bool run_ok(int64_t off, int64_t cnt, int64_t lim) {
  return cnt > 0 && off >= 0 && cnt <= lim && off <= lim - cnt;
}

// this lane's place in the ring layout: row wv * R + lane / K, slot lane % K
struct RowLane {
  int64_t row;
  int sl, base;
  bool on;
  u64 mask;   // the row's lanes
};
__device__ __forceinline__ RowLane row_lane(int64_t wv, int lane, int K, int64_t N) {
  const int R = WAVE / K, r = lane / K;
  RowLane q;
  q.sl = lane - r * K;
  q.base = r * K;
  q.row = wv * R + r;
  q.on = r < R && q.row < N;
  q.mask = q.on ? ((1ull << K) - 1ull) << q.base : 0ull;
  return q;
}

__global__ void __launch_bounds__(FT) forget_clear(uint32_t* __restrict__ bm, int64_t W, uint8_t* __restrict__ rowf,
                                                   int64_t N, int64_t* __restrict__ rec, int64_t nev) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < W; i += nt) bm[i] = 0u;
  for (int64_t i = tid; i < N; i += nt) rowf[i] = 0;
  if (tid < REC_WORDS) rec[tid] = tid == REC_N ? N : tid == REC_NEV ? nev : tid == REC_MAGIC_W ? REC_MAGIC : 0;
}

__global__ void __launch_bounds__(FT) forget_mark(const int64_t* __restrict__ ids, int64_t n, int64_t N,
                                                  uint32_t* __restrict__ bm, int64_t* __restrict__ rec) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  u64 bad = 0, fresh = 0;
  for (int64_t i = tid; i < n; i += nt) {
    const int64_t v = ids[i];
    if (v < 0 || v >= N) {
      ++bad;
      continue;
    }
    const uint32_t bit = 1u << (v & 31);
    if (!(atomicOr(&bm[v >> 5], bit) & bit)) ++fresh;   // (one thread per node sees the bit unset)
  }
  if (bad) atomicAdd(reinterpret_cast<u64*>(rec + REC_BAD), bad);
  if (fresh) atomicAdd(reinterpret_cast<u64*>(rec + REC_NODES), fresh);
}

// st / arena / ev_src / ev_dst NULL: the ring alone
__global__ void __launch_bounds__(FT) forget_count(const int64_t* __restrict__ nbr, const int64_t* __restrict__ eid,
                                                   int64_t N, int K, const int64_t* __restrict__ st,
                                                   const int64_t* __restrict__ arena,
                                                   const int64_t* __restrict__ ev_src,
                                                   const int64_t* __restrict__ ev_dst, int64_t nev,
                                                   const uint32_t* __restrict__ bm, uint8_t* __restrict__ rowf,
                                                   int64_t* __restrict__ rec) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id(), R = WAVE / K;
  u64 bad = 0, slots = 0, rows = 0, entries = 0;
  for (int64_t wv = tid >> 6; wv * R < N; wv += nt >> 6) {   // (wave-uniform trip count: the ballot sees whole waves)
    const RowLane q = row_lane(wv, lane, K, N);
    int64_t u = -1, e = -1;
    if (q.on) {
      u = nbr[q.row * K + q.sl];
      e = eid[q.row * K + q.sl];
    }
    const bool valid = q.on && e >= 0 && u != -1;
    if (valid && (u < 0 || u >= N || e >= nev)) ++bad;
    const bool remove = valid && in_f(bm, N, u) && !in_f(bm, N, q.row);
    const u64 m = __ballot(remove);
    if (remove) ++slots;
    if (q.on && q.sl == 0 && (m & q.mask)) {
      ++rows;
      rowf[q.row] = 1;
    }
  }
  if (st) {
    const int64_t lim = nev < (1ll << 62) ? 2 * nev : nev;
    for (int64_t v = tid >> 6; v < N; v += nt >> 6) {   // wave per node
      const bool own = in_f(bm, N, v);
      for (int dir = 0; dir < 2; ++dir) {
        const int64_t off = st[4 * v + 2 * dir], cnt = st[4 * v + 2 * dir + 1];
        if (cnt == 0) continue;
        if (!run_ok(off, cnt, lim)) {
          if (lane == 0) ++bad;
          continue;
        }
        if (own) continue;   // (the run of a node of F is dropped whole: not walked, not counted)
        const int64_t* __restrict__ partner = dir == 0 ? ev_dst : ev_src;
        for (int64_t k = lane; k < cnt; k += WAVE) {
          const int64_t e = arena[off + k];
          if (e < 0 || e >= nev) {
            ++bad;
            continue;
          }
          const int64_t p = partner[e];
          if (p < 0 || p >= N) ++bad;
          else if (in_f(bm, N, p)) ++entries;
        }
      }
    }
  }
  if (bad) atomicAdd(reinterpret_cast<u64*>(rec + REC_BAD), bad);
  if (slots) atomicAdd(reinterpret_cast<u64*>(rec + REC_SLOTS), slots);
  if (rows) atomicAdd(reinterpret_cast<u64*>(rec + REC_ROWS), rows);
  if (entries) atomicAdd(reinterpret_cast<u64*>(rec + REC_ENTRIES), entries);
}

// the plan in the workspace is for this node count and table and found no bad id
__device__ __forceinline__ bool apply_ok(const int64_t* __restrict__ rec, int64_t N, int64_t nev) {
  return rec[REC_MAGIC_W] == REC_MAGIC && rec[REC_N] == N && rec[REC_NEV] == nev && rec[REC_BAD] == 0;
}

// ev_t NULL: the t column drops the slots e_id drops; embT NULL: no embedding table
__global__ void __launch_bounds__(FT) forget_ring(int64_t* __restrict__ nbr, int64_t* __restrict__ eid,
                                                  float* __restrict__ rt, const float* __restrict__ ev_t, int64_t N,
                                                  int K, int64_t nev, const uint32_t* __restrict__ bm,
                                                  const uint8_t* __restrict__ rowf, const int64_t* __restrict__ rec,
                                                  uint8_t* __restrict__ embT) {
  if (!apply_ok(rec, N, nev)) return;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id(), R = WAVE / K;
  for (int64_t wv = tid >> 6; wv * R < N; wv += nt >> 6) {
    const RowLane q = row_lane(wv, lane, K, N);
    const bool own = q.on && in_f(bm, N, q.row);
    const bool touched = q.on && (own || rowf[q.row] != 0);
    if (!__ballot(touched)) continue;   // (most waves: N bytes read, no ring word)
    const int64_t at = q.row * K;       // (used under q.on only)
    int64_t u = -1, e = -1;
    float ct = -1.0f;
    if (touched) {
      u = nbr[at + q.sl];
      e = eid[at + q.sl];
      if (!ev_t) ct = rt[at + q.sl];
    }
    const bool keep = touched && !own && e >= 0 && u != -1 && !in_f(bm, N, u);
    if (ev_t && keep && e < nev) ct = ev_t[e];
    const u64 m = __ballot(keep);   // (every load of the wave is complete here: the stores below depend on m)
    const u64 mk = m & q.mask;
    const int s = __popcll(mk), pos = __popcll(mk & ((1ull << lane) - 1ull));
    int rk = pos;
    if (ev_t) {   // t ranked on its own, descending, ties by slot: the comparison loop of ring_merge_run
      rk = 0;
      for (int j = 0; j < K; ++j) {
        const float ot = __shfl(ct, (q.base + j) & (WAVE - 1), WAVE);
        const bool oj = (m >> ((q.base + j) & (WAVE - 1))) & 1ull;
        rk += oj && (ot > ct || (ot == ct && j < q.sl));
      }
    }
    if (!touched) continue;
    if (keep) {
      nbr[at + pos] = u;
      eid[at + pos] = e;
      rt[at + rk] = ct;
    }
    if (q.sl >= s) {
      nbr[at + q.sl] = -1;
      eid[at + q.sl] = -1;
      rt[at + q.sl] = -1.0f;
    }
    if (embT && q.sl == 0) embT[q.row] = 1;
  }
}

__device__ __forceinline__ void zero_row(float* __restrict__ q, int d, int lane) {
  if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) {   // (wave-uniform)
    const int d4 = d >> 2;
    for (int k = lane; k < d4; k += WAVE) reinterpret_cast<float4*>(q)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = (d4 << 2) + lane; k < d; k += WAVE) q[k] = 0.f;
  } else {
    for (int k = lane; k < d; k += WAVE) q[k] = 0.f;
  }
}

__global__ void __launch_bounds__(FT) forget_store(int64_t* __restrict__ st, int64_t* __restrict__ arena,
                                                   const int64_t* __restrict__ ev_src,
                                                   const int64_t* __restrict__ ev_dst, int64_t N, int64_t nev,
                                                   const uint32_t* __restrict__ bm, const int64_t* __restrict__ rec,
                                                   float* __restrict__ memory, int D, int64_t* __restrict__ last_update,
                                                   int32_t* __restrict__ node_gen) {
  if (!apply_ok(rec, N, nev)) return;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int lane = lane_id();
  const int64_t lim = 2 * nev;
  const u64 below = (1ull << lane) - 1ull;
  for (int64_t v = tid >> 6; v < N; v += nt >> 6) {   // wave per node
    if (in_f(bm, N, v)) {   // the node's own rows: what grow_rows / grow_store leave for a new node
      if (lane < 4) st[4 * v + lane] = 0;
      zero_row(memory + v * D, D, lane);
      if (lane == 0) {
        last_update[v] = 0;
        node_gen[v] = 0;
      }
      continue;
    }
    for (int dir = 0; dir < 2; ++dir) {
      const int64_t off = st[4 * v + 2 * dir], cnt = st[4 * v + 2 * dir + 1];
      if (!run_ok(off, cnt, lim)) continue;
      const int64_t* __restrict__ partner = dir == 0 ? ev_dst : ev_src;
      int64_t kept = 0;
      for (int64_t c = 0; c < cnt; c += WAVE) {
        const int64_t k = c + lane;
        const bool in = k < cnt;
        const int64_t e = in ? arena[off + k] : -1;
        const bool keep = in && !(e >= 0 && e < nev && in_f(bm, N, partner[e]));
        const u64 m = __ballot(keep);   // (the chunk's loads are complete; the write index never passes the read index)
        const int64_t w = kept + __popcll(m & below);
        if (keep && w != k) arena[off + w] = e;
        kept += __popcll(m);
      }
      if (kept != cnt && lane == 0) {
        st[4 * v + 2 * dir] = kept ? off : 0;
        st[4 * v + 2 * dir + 1] = kept;
      }
    }
  }
}

unsigned grid_for(int64_t work_items) {
  return (unsigned)std::min<int64_t>(MAX_GRID, std::max<int64_t>(1, (work_items + FT - 1) / FT));
}

int64_t ring_waves(int64_t N, int K) { return (N + WAVE / K - 1) / (WAVE / K); }

int check_ring(const char* who, int64_t N, int K, const void* nbr, const void* eid, const void* rt) {
  TGNX_CHECK_ARG(N > 0 && K > 0 && K <= KMAX, "%s: num_nodes = %lld, ring = %d (1..%d)", who, (long long)N, K, KMAX);
  if (N >= (1ll << 31)) {
    set_error("%s: num_nodes = %lld: node ids are below 2^31", who, (long long)N);
    return TGNX_ETOOBIG;
  }
  TGNX_CHECK_ARG(nbr && eid && rt, "%s: null ring (nbr / eid / rt)", who);
  return TGNX_OK;
}

int check_ws(const char* who, int64_t N, const void* ws, size_t ws_bytes, WsLay& L) {
  L = make_lay(N);
  TGNX_CHECK_ARG(ws && ws_bytes >= L.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                 "%s: workspace of tgnx_tgn_forget_ws_bytes(...) = %zu bytes, 16-B aligned", who, L.total);
  return TGNX_OK;
}

int check_engine(const char* who, const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* b, int64_t num_events) {
  TGNX_CHECK_ARG(cfg && b, "%s: null config / buffers", who);
  TGNX_CHECK_ARG(cfg->mem_dim > 0 && cfg->num_events > 0 && num_events >= 0 && num_events <= cfg->num_events,
                 "%s: bad mem_dim / num_events (%lld valid rows, capacity %lld)", who, (long long)num_events,
                 cfg ? (long long)cfg->num_events : 0ll);
  int rc = check_ring(who, cfg->num_nodes, cfg->ring, b->nbr, b->eid, b->rt);
  if (rc) return rc;
  TGNX_CHECK_ARG(!b->xrows, "%s: one device only (buf->xrows set: a data-parallel engine)", who);
  TGNX_CHECK_ARG(b->store && b->ev_src && b->ev_dst && b->ev_t && b->memory && b->last_update && b->node_gen,
                 "%s: null buffer (store / event table / memory / last_update / node_gen)", who);
  return TGNX_OK;
}

int launch_plan(const int64_t* nbr, const int64_t* eid, int64_t N, int K, const int64_t* st, const int64_t* ev_src,
                const int64_t* ev_dst, int64_t nev, const int64_t* ids, int64_t n, char* w, const WsLay& L,
                hipStream_t s) {
  int64_t* rec = reinterpret_cast<int64_t*>(w);
  uint32_t* bm = reinterpret_cast<uint32_t*>(w + L.bm);
  uint8_t* rowf = reinterpret_cast<uint8_t*>(w + L.rowf);
  forget_clear<<<grid_for(N), FT, 0, s>>>(bm, L.W, rowf, N, rec, nev);
  TGNX_LAUNCH_CHECK("forget_clear");
  if (n > 0) {
    forget_mark<<<grid_for(n), FT, 0, s>>>(ids, n, N, bm, rec);
    TGNX_LAUNCH_CHECK("forget_mark");
  }
  forget_count<<<grid_for(std::max(ring_waves(N, K), st ? N : 0) * WAVE), FT, 0, s>>>(
      nbr, eid, N, K, st, st ? st + 4 * N : nullptr, ev_src, ev_dst, nev, bm, rowf, rec);
  TGNX_LAUNCH_CHECK("forget_count");
  return TGNX_OK;
}

}  // namespace

extern "C" {

size_t tgnx_tgn_forget_ws_bytes(const tgnx_tgn_config* cfg) {
  if (!cfg || cfg->num_nodes <= 0 || cfg->num_nodes >= (1ll << 31)) {
    set_error("tgnx_tgn_forget_ws_bytes: bad config / node count");
    return 0;
  }
  return make_lay(cfg->num_nodes).total;
}

int tgnx_tgn_forget_plan(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events,
                         const int64_t* ids, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "tgnx_tgn_forget_plan";
  int rc = check_engine(who, cfg, buf, num_events);
  if (rc) return rc;
  TGNX_CHECK_ARG(n >= 0 && n < (1ll << 31) && (n == 0 || ids), "%s: %lld ids / null id list", who, (long long)n);
  WsLay L;
  rc = check_ws(who, cfg->num_nodes, ws, ws_bytes, L);
  if (rc) return rc;
  return launch_plan(buf->nbr, buf->eid, cfg->num_nodes, cfg->ring, buf->store, buf->ev_src, buf->ev_dst, num_events,
                     ids, n, reinterpret_cast<char*>(ws), L, as_stream(stream));
}

int tgnx_tgn_forget_apply(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, int64_t num_events, const void* ws,
                          size_t ws_bytes, uint8_t* emb_flags, void* stream) {
  const char* who = "tgnx_tgn_forget_apply";
  int rc = check_engine(who, cfg, buf, num_events);
  if (rc) return rc;
  WsLay L;
  rc = check_ws(who, cfg->num_nodes, ws, ws_bytes, L);
  if (rc) return rc;
  const char* w = reinterpret_cast<const char*>(ws);
  const int64_t* rec = reinterpret_cast<const int64_t*>(w);
  const uint32_t* bm = reinterpret_cast<const uint32_t*>(w + L.bm);
  const uint8_t* rowf = reinterpret_cast<const uint8_t*>(w + L.rowf);
  const int64_t N = cfg->num_nodes;
  hipStream_t s = as_stream(stream);
  forget_ring<<<grid_for(ring_waves(N, cfg->ring) * WAVE), FT, 0, s>>>(buf->nbr, buf->eid, buf->rt, buf->ev_t, N,
                                                                      cfg->ring, num_events, bm, rowf, rec, emb_flags);
  TGNX_LAUNCH_CHECK("forget_ring");
  forget_store<<<grid_for(N * WAVE), FT, 0, s>>>(buf->store, buf->store + 4 * N, buf->ev_src, buf->ev_dst, N,
                                                 num_events, bm, rec, buf->memory, cfg->mem_dim, buf->last_update,
                                                 buf->node_gen);
  TGNX_LAUNCH_CHECK("forget_store");
  return TGNX_OK;
}

int tgnx_ring_forget(int64_t* nbr, int64_t* eid, float* rt, const float* ev_t, int64_t num_events, int64_t N,
                     int32_t K, const int64_t* ids, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "tgnx_ring_forget";
  int rc = check_ring(who, N, K, nbr, eid, rt);
  if (rc) return rc;
  TGNX_CHECK_ARG(n >= 0 && n < (1ll << 31) && (n == 0 || ids), "%s: %lld ids / null id list", who, (long long)n);
  TGNX_CHECK_ARG(!ev_t || num_events >= 0, "%s: %lld event rows", who, (long long)num_events);
  WsLay L;
  rc = check_ws(who, N, ws, ws_bytes, L);
  if (rc) return rc;
  char* w = reinterpret_cast<char*>(ws);
  const int64_t nev = ev_t ? num_events : NO_TABLE;
  hipStream_t s = as_stream(stream);
  rc = launch_plan(nbr, eid, N, K, nullptr, nullptr, nullptr, nev, ids, n, w, L, s);
  if (rc) return rc;
  forget_ring<<<grid_for(ring_waves(N, K) * WAVE), FT, 0, s>>>(
      nbr, eid, rt, ev_t, N, K, nev, reinterpret_cast<const uint32_t*>(w + L.bm),
      reinterpret_cast<const uint8_t*>(w + L.rowf), reinterpret_cast<const int64_t*>(w), nullptr);
  TGNX_LAUNCH_CHECK("forget_ring");
  return TGNX_OK;
}

}  // extern "C"
