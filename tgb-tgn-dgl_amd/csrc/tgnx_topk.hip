// Fused all-pairs LinkPredictor scoring + top-k selection (tgnx_link_predictor_topk; torch.ops.tgnx.predictor_topk):
// for every source row q the k candidates c with the largest
//   logit[q][c] = w_out · relu(W_src z_src[q] + b_src + W_dst z_cand[c] + b_dst) + b_out      (decoder.py:12-27)
// without the [n_src · n_cand, D] operand the tiled predictor op needs.
//
//   Hs = z_src W_src^T + b_src [n_src, ldh], Hd = z_cand W_dst^T + b_dst [n_cand, ldh] on the MFMA GEMM (ldh = D
//   rounded up to 4 floats: every row starts 16-B aligned);
//   topk_pairs   one workgroup per (tile of 16 sources, chunk of 256 / 512 candidates): the pair logits, then the
//                chunk's k best per source as a partial list;
//   topk_merge   one wave per source: the k best of its chunks' lists (staged in LDS).
//
// The pair work is n_src · n_cand · D relu-FMAs (add, max, fma per term; the ReLU sits inside the contraction, so no
// MFMA).  A thread owns one candidate: its Hd row streams through registers 16 B at a time and every element is used
// for the tile's 16 sources, whose Hs rows sit in LDS k-major ([k][16]: four ds_read_b128 per k, every lane the same
// address, a broadcast), so one LDS instruction feeds 12 vector instructions.  Each logit is one sequential fma chain
// over k = 0 .. D - 1: its value does not depend on the grid, the chunk size or the tile a source falls in.
//
// Selection is on the logits under one total order — larger logit first, equal logits (float ==, so -0 = +0) by lower
// candidate position; NaN logits are never selected.  The chunk's logits stay in LDS ([16][chunk]); a wave takes four
// sources and picks k times the best entry strictly after its previous pick in that order (a strided scan, a DPP max
// of the values, a DPP min of the positions attaining it): no marking, no sort.  Measured at 200 x 9,227 x 100: the
// pair work ~26 us, a select round ~1.7 us, i.e. 36 % of the kernel at k = 10 and the larger part from k ~ 16 (the
// select is linear in k; k <= TGNX_TOPK_MAX; a sort per chunk would win at large k and is not built).  The global top-k
// is a subset of the chunks' top-k lists, so the merge (same order, positions global) is exact.
// Chunks rather than one workgroup per source tile walking every candidate: 200 sources are 13 tiles, 13 workgroups
// on 256 CUs; chunked, the wiki shape (200 x 9,227) is 13 x 37 workgroups.  Partials cost n_src · chunks · k · 8 B.
// No atomics, no allocation, no host synchronisation: graph-capturable, run-to-run identical.
//
// Three more entry points score the same pairs.  What they have in common is written once, and every kernel below
// is described by what is its own:
//   project_rows                   (host) the Hs / Hd GEMMs into the workspace carve_ws lays out;
//   stage_tile                     a tile's Hs rows (k-major) and w_out into LDS, zero past D and past n_src;
//   pair_chain<NQ>                 THE fma chain: a candidate's Hd row against NQ staged Hs rows (16: the tile; 1: one
//                                  source).  Every logit any kernel here produces has the bits this function gives;
//   stage_filter, excluded_mask    a tile's exclusion segments, clamped into the arrays, and a candidate's mask;
//   select_chunk<QW>               k rounds of pick-after-previous over logits in LDS, the partial list written;
//   topk_merge (launch_merge)      the partial lists' k best.
// (stage_filter, excluded_mask, select_chunk, topk_merge and the workspace layout sit in tgnx_topk_dev.h, which
// tgnx_knn.hip's similarity top-k includes too.)
//
//   tgnx_link_predictor_topk_filtered  per-source exclusions by key: topk_pairs<true> writes NaN over
//                  an excluded pair's LDS entry after out_all got the logit;
//   tgnx_link_predictor_topk_lists     a candidate list per source: topk_list_pairs, one workgroup per
//                  (source, chunk of the list), positions = slots in the list; topk_list_idx.
//
// tgnx_link_predictor_rank wants less than a selection: where each source's true destination stands
// among the candidates, i.e. per source three counts (logits above the target's, equal to it, compared at all).  No
// LDS logit matrix, no select rounds, no merge:
//   rank_target  a wave per source: tl[q] = logit(q, target[q]) in pair_chain's order (NaN at a target outside
//                z_cand), and the three counters zeroed;
//   rank_pairs   one workgroup per (tile of 16 sources, chunk of 256 candidates), a thread per candidate: its 16
//                logits against the tile's 16 tl in LDS, the key rules, then per source a ballot and a population
//                count per counter (scalar instructions: exact, and cheaper than three DPP sums), the four waves'
//                counts through LDS, one 64-bit integer atomicAdd per (source, counter) and chunk.
// The chunk is 256 = one candidate per thread.  Without the [16][chunk] logits nothing rewards a larger one but the
// Hs staging (6.4 KB of LDS writes against ~19 k VALU cycles per wave at D = 100), and at 200 x 9,227 it gives
// 13 x 37 = 481 workgroups of four waves on 256 CUs, at most two waves per SIMD, all resident at once; 512 would
// leave a fifth of the CUs with one workgroup against others' two of twice the length, and 128 changes nothing (the
// same waves).  Integer atomics commute: run-to-run identical.  No float atomics, no allocation, no host
// synchronisation.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "tgnx_common.h"
#include "tgnx_topk_dev.h"

using namespace tgnx;

namespace {

size_t pairs_smem(int64_t ldh, int chunk) { return (size_t)(ldh * TK_TQ + ldh + (int64_t)TK_TQ * chunk) * sizeof(float); }

int64_t list_chunks(int64_t max_len) { return std::max<int64_t>(1, ceil_div(max_len, TK_LCHUNK)); }

// what the *_ws_bytes functions return for valid sizes
size_t ws_bytes_of(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k, int64_t lists) {
  const size_t g = std::max(n_src > 0 ? tgnx_gemm_f32_ws_bytes(n_src, D, d_in) : 0,
                            n_cand > 0 ? tgnx_gemm_f32_ws_bytes(n_cand, D, d_in) : 0);
  return carve_ws(nullptr, n_src, n_cand, D, k, lists).used + align256(g) + 256;
}

// hsT [ldh][16]: the Hs rows of sources q0 .. q0 + 15, k-major; rows past nq and columns past D zero.  wl [ldh]:
// w_out, zero past D.
__device__ __forceinline__ void stage_tile(float* hsT, float* wl, const float* __restrict__ hs,
                                           const float* __restrict__ w_out, int64_t q0, int nq, int D, int ldh,
                                           int tid) {
  for (int x = tid; x < ldh * TK_TQ; x += TK_BLOCK) {
    const int kk = x / TK_TQ, q = x % TK_TQ;
    hsT[x] = (q < nq && kk < D) ? hs[(q0 + q) * ldh + kk] : 0.f;
  }
  for (int x = tid; x < ldh; x += TK_BLOCK) wl[x] = x < D ? w_out[x] : 0.f;
}

// The chain that fixes a logit's bits: acc[q] = fma(w_k, relu(Hs[q][k] + Hd[c][k]), acc[q]) for k ascending over the
// padded row (nv 16-B vectors), the pad columns (k >= D, which the GEMM does not write) read as zero.  `row` is the
// candidate's Hd row, wl the staged w_out (zero past D), hs the staged Hs: stage_tile's [ldh][16] tile for
// NQ = TK_TQ, one row [ldh] (zero past D) for NQ = 1.  Every kernel's logits come from here (rank_target restates
// the order), which is what makes the dense, list and rank logits of a pair equal bit for bit.
// The row comes in groups of TK_G vectors, the next group's loads in flight while this one is used (a load per
// iteration and its use right behind it left the L2 latency exposed 25 times per row at D = 100).  Past the row's
// end the last vector is loaded again and not used.
template <int NQ>
__device__ __forceinline__ void pair_chain(const float4* __restrict__ row, int nv, int D, const float* __restrict__ wl,
                                           const float* __restrict__ hs, float (&acc)[NQ]) {
  static_assert(NQ == 1 || NQ == TK_TQ, "one source or a tile");
  float4 nxt[TK_G];
#pragma unroll
  for (int u = 0; u < TK_G; ++u) nxt[u] = row[min(u, nv - 1)];
  for (int v0 = 0; v0 < nv; v0 += TK_G) {
    float4 cur[TK_G];
#pragma unroll
    for (int u = 0; u < TK_G; ++u) cur[u] = nxt[u];
#pragma unroll
    for (int u = 0; u < TK_G; ++u) nxt[u] = row[min(v0 + TK_G + u, nv - 1)];
#pragma unroll
    for (int u = 0; u < TK_G; ++u) {
      if (v0 + u >= nv) break;  // (uniform)
      const float he[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk = (v0 + u) * 4 + e;
        const float hv = kk < D ? he[e] : 0.f;
        const float wk = wl[kk];
        if constexpr (NQ == 1) {
          acc[0] = fmaf(wk, fmaxf(hs[kk] + hv, 0.f), acc[0]);
        } else {
          const float4* hq = reinterpret_cast<const float4*>(hs + kk * TK_TQ);
#pragma unroll
          for (int g = 0; g < TK_TQ / 4; ++g) {
            const float4 s = hq[g];
            acc[4 * g + 0] = fmaf(wk, fmaxf(s.x + hv, 0.f), acc[4 * g + 0]);
            acc[4 * g + 1] = fmaf(wk, fmaxf(s.y + hv, 0.f), acc[4 * g + 1]);
            acc[4 * g + 2] = fmaf(wk, fmaxf(s.z + hv, 0.f), acc[4 * g + 2]);
            acc[4 * g + 3] = fmaf(wk, fmaxf(s.w + hv, 0.f), acc[4 * g + 3]);
          }
        }
      }
    }
  }
}

template <bool FILT>
__global__ void __launch_bounds__(TK_BLOCK) topk_pairs(int64_t n_src, int64_t n_cand, int D, int ldh, int chunk, int nc,
                                                       const float* __restrict__ hs, const float* __restrict__ hd,
                                                       const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                       int k, float* __restrict__ pval, int* __restrict__ pidx,
                                                       float* __restrict__ out_all, TopkFilter f) {
  extern __shared__ __attribute__((aligned(16))) float tk_smem[];
  float* hsT = tk_smem;                     // [ldh][16] (stage_tile)
  float* wl = hsT + (size_t)ldh * TK_TQ;    // [ldh]
  float* L = wl + ldh;                      // [16][chunk] the chunk's logits
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x / nc, q0 = tile * TK_TQ;
  const int64_t cj = blockIdx.x % nc, cbase = cj * chunk;
  const int nq = (int)min((int64_t)TK_TQ, n_src - q0);
  const int nvalid = (int)min((int64_t)chunk, n_cand - cbase);
  // (ldh and chunk are multiples of 4: the struct starts 16-B aligned)
  TopkFilterLds* X = reinterpret_cast<TopkFilterLds*>(L + (size_t)TK_TQ * chunk);
  if constexpr (FILT) stage_filter(X, f, q0, nq, tid);
  stage_tile(hsT, wl, hs, w_out, q0, nq, D, ldh, tid);
  __syncthreads();
  const float bo = b_out[0];
  for (int c0 = 0; c0 < chunk; c0 += TK_BLOCK) {  // (block-uniform)
    const int cl = c0 + tid;
    const bool valid = cl < nvalid;
    // a thread past the chunk's end reads the last valid row (in bounds, result discarded)
    const int64_t cpos = cbase + min(cl, nvalid - 1);
    float acc[TK_TQ];
#pragma unroll
    for (int i = 0; i < TK_TQ; ++i) acc[i] = 0.f;
    pair_chain<TK_TQ>(reinterpret_cast<const float4*>(hd + cpos * ldh), ldh >> 2, D, wl, hsT, acc);
    // an excluded pair's entry in LDS becomes NaN, which the select never picks; out_all keeps the logit
    unsigned excl = 0;
    if constexpr (FILT) excl = excluded_mask(X, f, nq, f.cand_key ? f.cand_key[cpos] : cpos);
#pragma unroll
    for (int i = 0; i < TK_TQ; ++i) {
      const float lg = acc[i] + bo;
      // (entries past nvalid are never scanned)
      L[i * chunk + cl] = (FILT && ((excl >> i) & 1u)) ? TK_QNAN : lg;
      if (out_all && valid && i < nq) out_all[(q0 + i) * n_cand + cbase + cl] = lg;
    }
  }
  __syncthreads();
  // wave w takes sources 4 w .. 4 w + 3 (rows past nq hold the zero source's logits and are not stored)
  constexpr int QW = TK_TQ / (TK_BLOCK / WAVE);
  const int i0 = (tid >> 6) * QW;
  select_chunk<QW>(L + i0 * chunk, chunk, nvalid, k, tid & 63, q0 + i0, nq - i0, nc, cj, (int)cbase, pval, pidx);
}

// Per-source candidate lists (tgnx_link_predictor_topk_lists): one workgroup per (source, chunk of TK_LCHUNK list
// entries).  Hs[q] and w_out sit in LDS; a thread owns one entry and runs its gathered Hd row through pair_chain<1>,
// so the logit of (q, c) has the bits of the dense operator's.  Wave 0 then picks the chunk's k best (select_chunk<1>),
// positions being slots in the source's list.  Skipped entries (negative, >= n_cand, slot >= max_len) hold NaN.  The
// list's bounds are clamped into [0, nnz]; slots past the grid's reach (>= nc * TK_LCHUNK) are swept by the last chunk.
__global__ void __launch_bounds__(TK_LCHUNK) topk_list_pairs(int64_t n_cand, int D, int ldh, int nc, int64_t nnz,
                                                             int64_t max_len, const int64_t* __restrict__ list_ptr,
                                                             const int64_t* __restrict__ list_idx,
                                                             const float* __restrict__ hs, const float* __restrict__ hd,
                                                             const float* __restrict__ w_out,
                                                             const float* __restrict__ b_out, int k,
                                                             float* __restrict__ pval, int* __restrict__ pidx,
                                                             float* __restrict__ out_logits,
                                                             unsigned long long* __restrict__ n_invalid) {
  extern __shared__ __attribute__((aligned(16))) float tl_smem[];
  float* hq = tl_smem;       // [ldh] Hs[q], zero past D
  float* wl = hq + ldh;      // [ldh] w_out, zero past D
  float* L = wl + ldh;       // [TK_LCHUNK] the chunk's logits
  __shared__ int bad_sh[TK_LCHUNK / WAVE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t q = blockIdx.x / nc;
  const int cj = (int)(blockIdx.x % nc);
  const int64_t lo = clamp64(list_ptr[q], 0, nnz), hi = max(lo, clamp64(list_ptr[q + 1], 0, nnz));
  const int64_t len = hi - lo;
  for (int x = tid; x < ldh; x += TK_LCHUNK) {
    hq[x] = x < D ? hs[q * ldh + x] : 0.f;
    wl[x] = x < D ? w_out[x] : 0.f;
  }
  __syncthreads();
  const int64_t s = (int64_t)cj * TK_LCHUNK + tid;
  int bad = 0;
  float lg = TK_QNAN;
  if (s < len) {
    const int64_t c = list_idx[lo + s];
    const bool within = s < max_len;
    bad = !within || c >= n_cand;
    if (within && c >= 0 && c < n_cand) {
      float acc[1] = {0.f};
      pair_chain<1>(reinterpret_cast<const float4*>(hd + c * ldh), ldh >> 2, D, wl, hq, acc);
      lg = acc[0] + b_out[0];
    }
    if (out_logits) out_logits[lo + s] = lg;
  }
  L[tid] = lg;
  if (cj == nc - 1)
    for (int64_t t = (int64_t)nc * TK_LCHUNK + tid; t < len; t += TK_LCHUNK) {
      if (out_logits) out_logits[lo + t] = TK_QNAN;
      bad += 1;
    }
  if (n_invalid) {  // (block-uniform) the one atomic: an integer count
    int b = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o, WAVE);
    if (lane == 0) bad_sh[tid >> 6] = b;
  }
  __syncthreads();
  if (tid >= WAVE) return;
  if (n_invalid && tid == 0) {
    int b = 0;
    for (int w = 0; w < TK_LCHUNK / WAVE; ++w) b += bad_sh[w];
    if (b) atomicAdd(n_invalid, (unsigned long long)b);
  }
  const int nvalid = (int)max((int64_t)0, min((int64_t)TK_LCHUNK, len - (int64_t)cj * TK_LCHUNK));
  select_chunk<1>(L, 0, nvalid, k, lane, q, 1, nc, cj, cj * TK_LCHUNK, pval, pidx);
}

// out_idx[q][r] = the candidate position at the selected slot of q's list (-1 at the padding)
__global__ void __launch_bounds__(TK_BLOCK) topk_list_idx(int64_t n_src, int k, int64_t nnz,
                                                          const int64_t* __restrict__ list_ptr,
                                                          const int64_t* __restrict__ list_idx,
                                                          const int64_t* __restrict__ out_slot,
                                                          int64_t* __restrict__ out_idx) {
  const int64_t x = blockIdx.x * (int64_t)TK_BLOCK + threadIdx.x;
  if (x >= n_src * k) return;
  const int64_t q = x / k, slot = out_slot[x];
  const int64_t at = clamp64(list_ptr[q], 0, nnz) + slot;
  out_idx[x] = (slot >= 0 && at < nnz) ? list_idx[at] : -1;
}

// ---------------------------------------------------------------- rank of a given target (tgnx_link_predictor_rank)
// tl[q] = logit(q, target[q]) with the bits of the dense operator's out_all[q][target[q]]; NaN at a target outside
// [0, n_cand).  It does not call pair_chain but has to reproduce its order: the same terms, fma'd for k ascending
// over the padded row with the pad columns zero.  A wave per source: the lanes load the two rows once, coalesced, and
// leave w_k and relu(Hs[q][k] + Hd[p][k]) in LDS; lane 0 then runs the chain's fmas in order.  (A thread per source
// walking both rows, pair_chain<1>'s form, took 9.7 us at 200 x 9,227 x 100: seven dependent rounds of loads.)  The
// three counters start at zero here, before rank_pairs adds to them.
__global__ void __launch_bounds__(TK_BLOCK) rank_target(int64_t n_src, int64_t n_cand, int D, int ldh,
                                                        const int64_t* __restrict__ target,
                                                        const float* __restrict__ hs, const float* __restrict__ hd,
                                                        const float* __restrict__ w_out,
                                                        const float* __restrict__ b_out, float* __restrict__ tlogit,
                                                        unsigned long long* __restrict__ gt,
                                                        unsigned long long* __restrict__ eq,
                                                        unsigned long long* __restrict__ n) {
  constexpr int WPB = TK_BLOCK / WAVE;
  __shared__ float sw[WPB][TK_DMAX], st[WPB][TK_DMAX];  // (ldh <= TK_DMAX)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t q = blockIdx.x * (int64_t)WPB + wv;
  const bool live = q < n_src;  // (wave-uniform; a dead wave keeps the block's barrier)
  const int64_t p = live ? target[q] : -1;
  const bool inside = p >= 0 && p < n_cand;
  if (inside)
    for (int kk = lane; kk < ldh; kk += WAVE) {
      const bool in = kk < D;  // (the rows' pad columns are not written by the GEMM)
      sw[wv][kk] = in ? w_out[kk] : 0.f;
      st[wv][kk] = fmaxf((in ? hs[q * ldh + kk] : 0.f) + (in ? hd[p * ldh + kk] : 0.f), 0.f);
    }
  __syncthreads();
  if (!live || lane != 0) return;
  float lg = TK_QNAN;
  if (inside) {
    float acc = 0.f;
    for (int kk = 0; kk < ldh; ++kk) acc = fmaf(sw[wv][kk], st[wv][kk], acc);
    lg = acc + b_out[0];
  }
  tlogit[q] = lg;
  gt[q] = 0;
  eq[q] = 0;
  n[q] = 0;
}

// LDS of rank_pairs behind hsT and wl: the tile's targets and the waves' counts
struct RankLds {
  int64_t tkey[TK_TQ];  // key(target), where the target lies inside z_cand
  float tl[TK_TQ];
  int thas[TK_TQ];
  int cnt[TK_BLOCK / WAVE][3 * TK_TQ];
};

// One workgroup per (tile of 16 sources, chunk of TK_BLOCK competing candidates), a thread per candidate and its 16
// logits from pair_chain.  Candidate c counts for source i when its logit is not NaN, its key is not the target's
// (which covers c == target), not the source's and not in the source's segment.  With tl NaN (a skipped row)
// neither comparison holds: gt = eq = 0 and n is still the size of the compared set.
template <bool FILT>
__global__ void __launch_bounds__(TK_BLOCK) rank_pairs(int64_t n_src, int64_t n_cand, int64_t n_count, int D, int ldh,
                                                       int nc, const float* __restrict__ hs,
                                                       const float* __restrict__ hd, const float* __restrict__ w_out,
                                                       const float* __restrict__ b_out,
                                                       const int64_t* __restrict__ target,
                                                       const float* __restrict__ tlogit, TopkFilter f,
                                                       unsigned long long* __restrict__ gt,
                                                       unsigned long long* __restrict__ eq,
                                                       unsigned long long* __restrict__ n) {
  extern __shared__ __attribute__((aligned(16))) float rk_smem[];
  float* hsT = rk_smem;                    // [ldh][16] (stage_tile)
  float* wl = hsT + (size_t)ldh * TK_TQ;   // [ldh]
  RankLds* R = reinterpret_cast<RankLds*>(wl + ldh);  // (17 ldh floats: 16-B aligned)
  TopkFilterLds* X = reinterpret_cast<TopkFilterLds*>(R + 1);
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x / nc, q0 = tile * TK_TQ;
  const int64_t cbase = (int64_t)(blockIdx.x % nc) * TK_BLOCK;
  const int nq = (int)min((int64_t)TK_TQ, n_src - q0);
  const int nvalid = (int)min((int64_t)TK_BLOCK, n_count - cbase);  // (>= 1: the grid covers [0, n_count))
  if (tid < TK_TQ) {
    const int64_t p = tid < nq ? target[q0 + tid] : -1;
    const bool in = p >= 0 && p < n_cand;
    R->thas[tid] = in;
    R->tkey[tid] = in ? (f.cand_key ? f.cand_key[p] : p) : 0;
    R->tl[tid] = tid < nq ? tlogit[q0 + tid] : TK_QNAN;
  }
  if constexpr (FILT) stage_filter(X, f, q0, nq, tid);
  stage_tile(hsT, wl, hs, w_out, q0, nq, D, ldh, tid);
  __syncthreads();
  const float bo = b_out[0];
  const bool valid = tid < nvalid;
  // a thread past the chunk's end reads the last valid row (in bounds, counted nowhere)
  const int64_t cpos = cbase + min(tid, nvalid - 1);
  float acc[TK_TQ];
#pragma unroll
  for (int i = 0; i < TK_TQ; ++i) acc[i] = 0.f;
  pair_chain<TK_TQ>(reinterpret_cast<const float4*>(hd + cpos * ldh), ldh >> 2, D, wl, hsT, acc);
  const int64_t ck = f.cand_key ? f.cand_key[cpos] : cpos;
  unsigned excl = 0;
  if constexpr (FILT) excl = excluded_mask(X, f, nq, ck);
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int i = 0; i < TK_TQ; ++i) {
    const float lg = acc[i] + bo, tl = R->tl[i];
    const bool in = valid && lg == lg && !(R->thas[i] && R->tkey[i] == ck) && !((excl >> i) & 1u);
    const int cn = __popcll(__ballot(in)), cg = __popcll(__ballot(in && lg > tl)), ce = __popcll(__ballot(in && lg == tl));
    if (lane == 0) {
      R->cnt[wv][3 * i + 0] = cg;
      R->cnt[wv][3 * i + 1] = ce;
      R->cnt[wv][3 * i + 2] = cn;
    }
  }
  __syncthreads();
  if (tid < 3 * TK_TQ) {
    const int i = tid / 3, which = tid % 3;
    int sum = 0;
#pragma unroll
    for (int w = 0; w < TK_BLOCK / WAVE; ++w) sum += R->cnt[w][tid];
    if (i < nq && sum > 0) atomicAdd((which == 0 ? gt : (which == 1 ? eq : n)) + q0 + i, (unsigned long long)sum);
  }
}

size_t rank_smem(int64_t ldh, bool filt) {
  return (size_t)(ldh * TK_TQ + ldh) * sizeof(float) + sizeof(RankLds) + (filt ? sizeof(TopkFilterLds) : 0);
}

// The checks the three entry points share, in one wording: k (rank passes 1), the sizes with n_cand < n_cand_end (so
// that a position plus the entry point's chunk stays inside an int), and the pointers all of them take; `own` says
// that the entry point's own pointers are there.
int check_common(const char* name, int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k,
                 int64_t n_cand_end, const void* z_cand, const void* w_src, const void* w_dst, const void* w_out,
                 const void* b_out, const void* ws, bool own) {
  TGNX_CHECK_ARG(k >= 1 && k <= TGNX_TOPK_MAX, "%s: k must be in [1, %d], got %d", name, TGNX_TOPK_MAX, k);
  TGNX_CHECK_ARG(n_src >= 0 && n_cand >= 0 && d_in >= 1 && D >= 1 && D <= TK_DMAX && d_in < (1 << 30) &&
                     n_cand < n_cand_end && n_src < (int64_t(1) << 31),
                 "%s: bad sizes (n_src, n_cand >= 0, d_in >= 1, 1 <= D <= %d)", name, (int)TK_DMAX);
  TGNX_CHECK_ARG(w_src && w_dst && w_out && b_out && ws && own && (n_cand == 0 || z_cand), "%s: null pointer", name);
  return TGNX_OK;
}

// Hs = z_src W_src^T + b_src and Hd = z_cand W_dst^T + b_dst into the workspace, the same two GEMMs for every entry
// point.  (n_cand = 0: neither is computed, neither is used.)
int project_rows(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src, const float* z_cand,
                 const float* w_src, const float* b_src, const float* w_dst, const float* b_dst, const TopkWs& w,
                 size_t ws_bytes, void* stream) {
  if (n_cand == 0) return TGNX_OK;
  const int64_t ldh = ld_of(D);
  const size_t gbytes = ws_bytes - w.used;
  const int rc =
      tgnx_gemm_f32(n_src, D, d_in, z_src, d_in, 0, w_src, d_in, 1, w.hs, ldh, b_src, 0, w.gemm, gbytes, stream);
  if (rc != TGNX_OK) return rc;
  return tgnx_gemm_f32(n_cand, D, d_in, z_cand, d_in, 0, w_dst, d_in, 1, w.hd, ldh, b_dst, 0, w.gemm, gbytes, stream);
}

// the dense operator with or without exclusions (f == nullptr: the launches tgnx_link_predictor_topk always made)
int topk_dense(const char* name, int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
               const float* z_cand, const float* w_src, const float* b_src, const float* w_dst, const float* b_dst,
               const float* w_out, const float* b_out, int32_t k, int32_t sigmoid, const TopkFilter* f, float* out_val,
               int64_t* out_idx, float* out_all, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_common(name, n_src, n_cand, d_in, D, k, (int64_t(1) << 31) - TK_CHUNK_MAX, z_cand, w_src, w_dst, w_out,
                        b_out, ws, n_src == 0 || (z_src && out_val && out_idx));
  if (rc != TGNX_OK) return rc;
  if (f)
    TGNX_CHECK_ARG(f->nnz >= 0 && (!f->excl_ptr || f->nnz == 0 || f->excl_key),
                   "%s: excl_ptr needs excl_key and nnz >= 0", name);
  TGNX_CHECK_ARG(ws_bytes >= tgnx_link_predictor_topk_ws_bytes(n_src, n_cand, d_in, D, k), "%s: workspace too small",
                 name);
  if (n_src == 0) return TGNX_OK;
  hipStream_t s = as_stream(stream);
  const TopkWs w = carve_ws(ws, n_src, n_cand, D, k, dense_lists(n_cand));
  const int64_t ldh = ld_of(D);
  const int chunk = chunk_of(n_src, n_cand);
  const int64_t nc = ceil_div(n_cand, chunk), blocks = ceil_div(n_src, TK_TQ) * nc;
  TGNX_CHECK_ARG(blocks < (int64_t(1) << 31), "%s: n_src x n_cand beyond one launch's grid", name);
  rc = project_rows(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst, w, ws_bytes, stream);
  if (rc != TGNX_OK) return rc;
  if (n_cand > 0) {  // (n_cand = 0: no chunk)
    if (f)
      hipLaunchKernelGGL(topk_pairs<true>, dim3((unsigned)blocks), dim3(TK_BLOCK),
                         pairs_smem(ldh, chunk) + sizeof(TopkFilterLds), s, n_src, n_cand, (int)D, (int)ldh, chunk,
                         (int)nc, (const float*)w.hs, (const float*)w.hd, w_out, b_out, (int)k, w.pval, w.pidx, out_all,
                         *f);
    else
      hipLaunchKernelGGL(topk_pairs<false>, dim3((unsigned)blocks), dim3(TK_BLOCK), pairs_smem(ldh, chunk), s, n_src,
                         n_cand, (int)D, (int)ldh, chunk, (int)nc, (const float*)w.hs, (const float*)w.hd, w_out, b_out,
                         (int)k, w.pval, w.pidx, out_all, TopkFilter{});
    TGNX_LAUNCH_CHECK("topk_pairs");
  }
  return launch_merge(s, n_src, nc, k, w, sigmoid, out_val, out_idx);
}

}  // namespace

extern "C" {

size_t tgnx_link_predictor_topk_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k) {
  if (n_src < 0 || n_cand < 0 || d_in <= 0 || D <= 0 || D > TK_DMAX || k < 1 || k > TGNX_TOPK_MAX) return 256;
  return ws_bytes_of(n_src, n_cand, d_in, D, k, dense_lists(n_cand));
}

int tgnx_link_predictor_topk(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                             const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                             const float* b_dst, const float* w_out, const float* b_out, int32_t k, int32_t sigmoid,
                             float* out_val, int64_t* out_idx, float* out_all, void* ws, size_t ws_bytes,
                             void* stream) {
  return topk_dense("tgnx_link_predictor_topk", n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst, w_out,
                    b_out, k, sigmoid, nullptr, out_val, out_idx, out_all, ws, ws_bytes, stream);
}

size_t tgnx_link_predictor_topk_filtered_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k) {
  return tgnx_link_predictor_topk_ws_bytes(n_src, n_cand, d_in, D, k);
}

int tgnx_link_predictor_topk_filtered(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                                      const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                                      const float* b_dst, const float* w_out, const float* b_out, int32_t k,
                                      int32_t sigmoid, const int64_t* cand_key, const int64_t* src_key,
                                      const int64_t* excl_ptr, const int64_t* excl_key, int64_t nnz, float* out_val,
                                      int64_t* out_idx, float* out_all, void* ws, size_t ws_bytes, void* stream) {
  const TopkFilter f{cand_key, src_key, excl_ptr, excl_key, nnz};
  return topk_dense("tgnx_link_predictor_topk_filtered", n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst,
                    b_dst, w_out, b_out, k, sigmoid, &f, out_val, out_idx, out_all, ws, ws_bytes, stream);
}

size_t tgnx_link_predictor_topk_lists_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, int32_t k,
                                               int64_t max_len) {
  if (n_src < 0 || n_cand < 0 || d_in <= 0 || D <= 0 || D > TK_DMAX || k < 1 || k > TGNX_TOPK_MAX || max_len < 0)
    return 256;
  return ws_bytes_of(n_src, n_cand, d_in, D, k, list_chunks(max_len));
}

int tgnx_link_predictor_topk_lists(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                                   const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                                   const float* b_dst, const float* w_out, const float* b_out, int32_t k,
                                   int32_t sigmoid, const int64_t* list_ptr, const int64_t* list_idx, int64_t nnz,
                                   int64_t max_len, float* out_val, int64_t* out_idx, int64_t* out_slot,
                                   float* out_logits, int64_t* n_invalid, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "tgnx_link_predictor_topk_lists";
  int rc = check_common(name, n_src, n_cand, d_in, D, k, int64_t(1) << 31, z_cand, w_src, w_dst, w_out, b_out, ws,
                        list_ptr && (nnz == 0 || list_idx) && (n_src == 0 || (z_src && out_val && out_idx && out_slot)));
  if (rc != TGNX_OK) return rc;
  TGNX_CHECK_ARG(nnz >= 0 && max_len >= 0 && max_len < (int64_t(1) << 31) - TK_LCHUNK,
                 "%s: nnz and max_len must be >= 0 (max_len < 2^31 - %d)", name, TK_LCHUNK);
  TGNX_CHECK_ARG(ws_bytes >= tgnx_link_predictor_topk_lists_ws_bytes(n_src, n_cand, d_in, D, k, max_len),
                 "%s: workspace too small", name);
  if (n_src == 0) return TGNX_OK;
  hipStream_t s = as_stream(stream);
  const int64_t ldh = ld_of(D), nc = list_chunks(max_len), blocks = n_src * nc;
  const TopkWs w = carve_ws(ws, n_src, n_cand, D, k, nc);
  TGNX_CHECK_ARG(blocks < (int64_t(1) << 31), "%s: n_src x max_len beyond one launch's grid", name);
  rc = project_rows(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst, w, ws_bytes, stream);
  if (rc != TGNX_OK) return rc;
  // (n_cand = 0: every entry is skipped)
  hipLaunchKernelGGL(topk_list_pairs, dim3((unsigned)blocks), dim3(TK_LCHUNK), (size_t)(2 * ldh + TK_LCHUNK) * 4, s,
                     n_cand, (int)D, (int)ldh, (int)nc, nnz, max_len, list_ptr, list_idx, (const float*)w.hs,
                     (const float*)w.hd, w_out, b_out, (int)k, w.pval, w.pidx, out_logits,
                     reinterpret_cast<unsigned long long*>(n_invalid));
  TGNX_LAUNCH_CHECK("topk_list_pairs");
  rc = launch_merge(s, n_src, nc, k, w, sigmoid, out_val, out_slot);
  if (rc != TGNX_OK) return rc;
  hipLaunchKernelGGL(topk_list_idx, dim3((unsigned)ceil_div(n_src * k, TK_BLOCK)), dim3(TK_BLOCK), 0, s, n_src, (int)k,
                     nnz, list_ptr, list_idx, (const int64_t*)out_slot, out_idx);
  TGNX_LAUNCH_CHECK("topk_list_idx");
  return TGNX_OK;
}

size_t tgnx_link_predictor_rank_ws_bytes(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D) {
  if (n_src < 0 || n_cand < 0 || d_in <= 0 || D <= 0 || D > TK_DMAX) return 256;
  return ws_bytes_of(n_src, n_cand, d_in, D, 1, 0);
}

int tgnx_link_predictor_rank(int64_t n_src, int64_t n_cand, int64_t d_in, int64_t D, const float* z_src,
                             const float* z_cand, const float* w_src, const float* b_src, const float* w_dst,
                             const float* b_dst, const float* w_out, const float* b_out, int64_t n_count,
                             const int64_t* target, const int64_t* cand_key, const int64_t* src_key,
                             const int64_t* excl_ptr, const int64_t* excl_key, int64_t nnz, int64_t* out_gt,
                             int64_t* out_eq, int64_t* out_n, float* out_tlogit, void* ws, size_t ws_bytes,
                             void* stream) {
  const char* name = "tgnx_link_predictor_rank";
  int rc = check_common(name, n_src, n_cand, d_in, D, 1, (int64_t(1) << 31) - TK_BLOCK, z_cand, w_src, w_dst, w_out,
                        b_out, ws, n_src == 0 || (z_src && target && out_gt && out_eq && out_n && out_tlogit));
  if (rc != TGNX_OK) return rc;
  TGNX_CHECK_ARG(n_count >= 0 && n_count <= n_cand, "%s: n_count must be in [0, n_cand], got %lld", name,
                 (long long)n_count);
  TGNX_CHECK_ARG(nnz >= 0 && (!excl_ptr || nnz == 0 || excl_key), "%s: excl_ptr needs excl_key and nnz >= 0", name);
  TGNX_CHECK_ARG(ws_bytes >= tgnx_link_predictor_rank_ws_bytes(n_src, n_cand, d_in, D), "%s: workspace too small",
                 name);
  if (n_src == 0) return TGNX_OK;
  hipStream_t s = as_stream(stream);
  const TopkWs w = carve_ws(ws, n_src, n_cand, D, 1, 0);
  const int64_t ldh = ld_of(D);
  const int64_t nc = ceil_div(n_count, TK_BLOCK), blocks = ceil_div(n_src, TK_TQ) * nc;
  TGNX_CHECK_ARG(blocks < (int64_t(1) << 31), "%s: n_src x n_count beyond one launch's grid", name);
  rc = project_rows(n_src, n_cand, d_in, D, z_src, z_cand, w_src, b_src, w_dst, b_dst, w, ws_bytes, stream);
  if (rc != TGNX_OK) return rc;
  // (n_cand = 0: every row is skipped)
  unsigned long long* gt = reinterpret_cast<unsigned long long*>(out_gt);
  unsigned long long* eq = reinterpret_cast<unsigned long long*>(out_eq);
  unsigned long long* nn = reinterpret_cast<unsigned long long*>(out_n);
  hipLaunchKernelGGL(rank_target, dim3((unsigned)ceil_div(n_src, TK_BLOCK / WAVE)), dim3(TK_BLOCK), 0, s, n_src, n_cand,
                     (int)D, (int)ldh, target, (const float*)w.hs, (const float*)w.hd, w_out, b_out, out_tlogit, gt, eq,
                     nn);
  TGNX_LAUNCH_CHECK("rank_target");
  if (n_count == 0) return TGNX_OK;
  const TopkFilter f{cand_key, src_key, excl_ptr, excl_key, nnz};
  if (src_key || excl_ptr)
    hipLaunchKernelGGL(rank_pairs<true>, dim3((unsigned)blocks), dim3(TK_BLOCK), rank_smem(ldh, true), s, n_src, n_cand,
                       n_count, (int)D, (int)ldh, (int)nc, (const float*)w.hs, (const float*)w.hd, w_out, b_out, target,
                       (const float*)out_tlogit, f, gt, eq, nn);
  else
    hipLaunchKernelGGL(rank_pairs<false>, dim3((unsigned)blocks), dim3(TK_BLOCK), rank_smem(ldh, false), s, n_src,
                       n_cand, n_count, (int)D, (int)ldh, (int)nc, (const float*)w.hs, (const float*)w.hd, w_out, b_out,
                       target, (const float*)out_tlogit, f, gt, eq, nn);
  TGNX_LAUNCH_CHECK("rank_pairs");
  return TGNX_OK;
}

}  // extern "C"
