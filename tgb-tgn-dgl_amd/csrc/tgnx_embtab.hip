// Stale-row bookkeeping of the embedding table on gfx950: which rows of a materialised [N, D] table
// of eval-mode embeddings a batch of events has made stale, as an ascending id list tgnx_tgn_embed_into recomputes.
//
// Three byte planes [3][N] (T, D1, D2; plane p starts N bytes after plane p - 1):
//   T    nodes whose memory / last_update / ring row was written: the endpoints of every observed batch
//   D1   nodes with a valid ring slot (e_id >= 0) naming a node of T
//   D2   nodes with a valid ring slot naming a node of T | D1        (layers = 2 only)
// Kernels:
//   embtab_touch   a thread per endpoint stores 1 into T (ids outside [0, N) skipped)
//   embtab_expand  flat over the ring's (node, slot) pairs, so consecutive lanes load consecutive 8-byte words of
//                  nbr / eid; a hit stores 1 into the node's byte of the output plane.  Pass 1 reads T, writes D1;
//                  pass 2 reads T and D1, writes D2: no pass reads the plane it writes
//   embtab_count / embtab_scan / embtab_emit
//                  the ascending list: a workgroup owns 256 consecutive nodes, a wave 64 of them (ballot + popcount
//                  give each set node its place in the wave), embtab_scan turns the workgroups' counts into their
//                  offsets in block order, embtab_emit writes the ids and clears the three planes
//   Every flag write is a plain store of one byte value by whoever sees the condition (idempotent: no atomics, no
//   read-modify-write), and the list's order comes from the scan, not from a cursor: run-to-run identical.
#include <algorithm>

#include "tgnx_common.h"

using namespace tgnx;

namespace {

constexpr int ET = 256;              // workgroup size; also the nodes one workgroup of the list kernels owns
constexpr int64_t MAX_GRID = 2048;   // grid-stride kernels: 8 workgroups per CU cover the 256 CUs
constexpr int SCAN_T = 1024;         // embtab_scan's single workgroup

__global__ void __launch_bounds__(ET) embtab_touch(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                   int64_t B, int64_t N, uint8_t* __restrict__ T) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < 2 * B; i += nt) {
    const int64_t v = i < B ? src[i] : dst[i - B];
    if (v >= 0 && v < N) T[v] = 1;
  }
}

// in1 may be NULL (pass 1)
__global__ void __launch_bounds__(ET) embtab_expand(const int64_t* __restrict__ nbr, const int64_t* __restrict__ eid,
                                                    int64_t N, int K, const uint8_t* __restrict__ in0,
                                                    const uint8_t* __restrict__ in1, uint8_t* __restrict__ out) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t slots = N * K;
  for (int64_t p = tid; p < slots; p += nt) {
    const int64_t u = nbr[p];
    if (eid[p] < 0 || u < 0 || u >= N) continue;   // (reset_state leaves stale ids under e_id = -1)
    if (in0[u] | (in1 ? in1[u] : 0)) out[p / K] = 1;
  }
}

// (D2 is read at layers = 2 only: nothing writes it at layers = 1)
__device__ __forceinline__ bool any_plane(const uint8_t* f, int64_t N, int64_t v, int layers) {
  return v < N && (f[v] | f[N + v] | (layers == 2 ? f[2 * N + v] : 0)) != 0;
}

__global__ void __launch_bounds__(ET) embtab_count(const uint8_t* __restrict__ f, int64_t N, int layers,
                                                   int* __restrict__ cnt) {
  __shared__ int wc[ET / WAVE];
  const int64_t v = blockIdx.x * (int64_t)ET + threadIdx.x;
  const unsigned long long m = __ballot(any_plane(f, N, v, layers));
  if (lane_id() == 0) wc[threadIdx.x / WAVE] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < ET / WAVE; ++w) s += wc[w];
    cnt[blockIdx.x] = s;
  }
}

// cnt[b] -> the exclusive prefix in block order, in place; *total = the sum
__global__ void __launch_bounds__(SCAN_T) embtab_scan(int* __restrict__ cnt, int64_t nb, int64_t* __restrict__ total) {
  __shared__ int sh[32];
  int carry = 0;
  for (int64_t base = 0; base < nb; base += SCAN_T) {
    const int64_t b = base + threadIdx.x;
    const int c = b < nb ? cnt[b] : 0;
    int sum;
    const int ex = block_excl_scan(c, sh, &sum);
    if (b < nb) cnt[b] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(ET) embtab_emit(uint8_t* __restrict__ f, int64_t N, int layers,
                                                  const int* __restrict__ off, int64_t* __restrict__ ids) {
  __shared__ int wc[ET / WAVE];
  const int64_t v = blockIdx.x * (int64_t)ET + threadIdx.x;
  const bool set = any_plane(f, N, v, layers);
  const unsigned long long m = __ballot(set);
  const int w = threadIdx.x / WAVE, l = lane_id();
  if (l == 0) wc[w] = __popcll(m);
  __syncthreads();
  int before = 0;
  for (int i = 0; i < w; ++i) before += wc[i];
  if (set) ids[(int64_t)off[blockIdx.x] + before + __popcll(m & ((1ull << l) - 1ull))] = v;
  if (v < N) f[v] = f[N + v] = f[2 * N + v] = 0;
}

unsigned grid_for(int64_t work_items) {
  return (unsigned)std::min<int64_t>(MAX_GRID, std::max<int64_t>(1, (work_items + ET - 1) / ET));
}

int64_t list_blocks(int64_t N) { return (N + ET - 1) / ET; }

int check_nodes(const char* who, int64_t N) {
  TGNX_CHECK_ARG(N > 0, "%s: num_nodes = %lld", who, (long long)N);
  if (N >= (1ll << 31)) {
    set_error("%s: num_nodes = %lld: node ids are below 2^31", who, (long long)N);
    return TGNX_ETOOBIG;
  }
  return TGNX_OK;
}

}  // namespace

extern "C" {

int tgnx_embtab_touch(const int64_t* src, const int64_t* dst, int64_t B, int64_t N, uint8_t* flags, void* stream) {
  const char* who = "tgnx_embtab_touch";
  int rc = check_nodes(who, N);
  if (rc) return rc;
  TGNX_CHECK_ARG(B >= 0 && B < (1ll << 30), "%s: B = %lld", who, (long long)B);
  if (B == 0) return TGNX_OK;
  TGNX_CHECK_ARG(src && dst && flags, "%s: null pointer", who);
  embtab_touch<<<grid_for(2 * B), ET, 0, as_stream(stream)>>>(src, dst, B, N, flags);
  TGNX_LAUNCH_CHECK("embtab_touch");
  return TGNX_OK;
}

int tgnx_embtab_expand(const tgnx_tgn_config* cfg, const tgnx_tgn_buffers* buf, uint8_t* flags, void* stream) {
  const char* who = "tgnx_embtab_expand";
  TGNX_CHECK_ARG(cfg && buf && flags, "%s: null config / buffers / flags", who);
  TGNX_CHECK_ARG(!buf->xrows, "%s: one device only (buf->xrows set: a data-parallel engine)", who);
  int rc = check_nodes(who, cfg->num_nodes);
  if (rc) return rc;
  TGNX_CHECK_ARG(cfg->ring > 0 && buf->nbr && buf->eid, "%s: no ring", who);
  const int64_t N = cfg->num_nodes;
  hipStream_t s = as_stream(stream);
  embtab_expand<<<grid_for(N * cfg->ring), ET, 0, s>>>(buf->nbr, buf->eid, N, cfg->ring, flags, nullptr, flags + N);
  TGNX_LAUNCH_CHECK("embtab_expand");
  if (cfg->layers == 2) {
    embtab_expand<<<grid_for(N * cfg->ring), ET, 0, s>>>(buf->nbr, buf->eid, N, cfg->ring, flags, flags + N,
                                                         flags + 2 * N);
    TGNX_LAUNCH_CHECK("embtab_expand (2)");
  }
  return TGNX_OK;
}

size_t tgnx_embtab_list_ws_bytes(int64_t N) {
  if (N <= 0 || N >= (1ll << 31)) return 0;
  return (size_t)((list_blocks(N) * 4 + 15) & ~15ll);
}

int tgnx_embtab_list(uint8_t* flags, int64_t N, int32_t layers, int64_t* out_ids, int64_t* out_count, void* ws,
                     size_t ws_bytes, void* stream) {
  const char* who = "tgnx_embtab_list";
  int rc = check_nodes(who, N);
  if (rc) return rc;
  TGNX_CHECK_ARG(layers == 1 || layers == 2, "%s: layers = %d", who, (int)layers);
  TGNX_CHECK_ARG(flags && out_ids && out_count && ws, "%s: null pointer", who);
  TGNX_CHECK_ARG(ws_bytes >= tgnx_embtab_list_ws_bytes(N) && (reinterpret_cast<uintptr_t>(ws) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(out_count) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_ids) & 7) == 0,
                 "%s: workspace below tgnx_embtab_list_ws_bytes, or a misaligned pointer", who);
  hipStream_t s = as_stream(stream);
  const int64_t nb = list_blocks(N);
  int* cnt = reinterpret_cast<int*>(ws);
  embtab_count<<<(unsigned)nb, ET, 0, s>>>(flags, N, layers, cnt);
  TGNX_LAUNCH_CHECK("embtab_count");
  embtab_scan<<<1, SCAN_T, 0, s>>>(cnt, nb, out_count);
  TGNX_LAUNCH_CHECK("embtab_scan");
  embtab_emit<<<(unsigned)nb, ET, 0, s>>>(flags, N, layers, cnt, out_ids);
  TGNX_LAUNCH_CHECK("embtab_emit");
  return TGNX_OK;
}

}  // extern "C"
