// Embedding-space nearest neighbours with the selection fused in (tgnx_embed_knn; torch.ops.tgnx.embed_knn; DESIGN
// §3b-10): for every query row q the k candidate rows c with the largest
//   score[q][c] = z_q[q] · z_cand[c]                               (TGNX_KNN_DOT)
//   score[q][c] = (z_q[q] / |z_q[q]|) · (z_cand[c] / |z_cand[c]|)  (TGNX_KNN_COSINE; a row with Σ z² = 0 scales by 0)
// without the [n_q, n_cand] score matrix a GEMM + torch.topk composition writes and reads back.  Unlike the
// predictor's logit (tgnx_topk.hip: the ReLU sits inside the contraction) a similarity is a plain dot product, so the
// pair work runs on v_mfma_f32_16x16x4_f32, which on gfx950 is bit for bit a k-ordered fmaf chain.
//
//   knn_prep    16 lanes per row: the rows of z_q and z_cand copied into the workspace at pitch ldh (D rounded up
//               to 4 floats, pad columns zero: every row starts 16-B aligned whatever D and the caller's pitch are),
//               under COSINE multiplied by 1 / sqrt(Σ z²).  After it the pair kernel does not know the metric.
//   knn_pairs   one workgroup per (tile of 16 queries, chunk of 256 / 512 candidates; chunk_of's rule): the scores
//               into LDS [16][chunk], the NaN mask of the excluded pairs, then select_chunk's partial lists;
//   topk_merge  the partial lists' k best (tgnx_topk_dev.h, as the predictor top-k uses it).
//
// knn_pairs.  The query tile is the MFMA's A operand (lane l: A[row l & 15][k l >> 4]), a 16-candidate sub-tile its B
// operand (B[k l >> 4][col l & 15]).  Lane l = (r = l & 15, h = l >> 4) loads the 16-B vector 4 j + h of row r
// (floats 16 j + 4 h .. + 3), j = 0 .. NJ - 1 with NJ = ceil(ldh / 16) a template parameter, and feeds its four
// components to four consecutive MFMAs.  The query vectors stay in registers for the whole chunk (NJ float4: 28
// VGPRs at D = 100, 64 at D = 256).  A vector past the row's end (4 j + h >= ldh / 4) is zero in BOTH operands (its
// load is clamped into the row).  A wave owns chunk / 64 sub-tiles and runs them two at a time, each with its own
// accumulator: the MFMA issues every 32 cycles and a dependent accumulator waits 40.
//
// THE ORDER OF A SCORE.  score = one accumulator started at 0, through the MFMAs (j, e), j = 0 .. NJ - 1 outer,
// e = 0 .. 3 inner, each adding the products at k = 16 j + 4 h + e for h = 0, 1, 2, 3 in the instruction's own fixed
// order; i.e. the chain runs over the fixed permutation k = 16 j + e, 16 j + 4 + e, 16 j + 8 + e, 16 j + 12 + e of the
// padded row, the same for every pair.  Zero padding is exact (fma(0, 0, acc) == acc up to the sign of zero, which
// == ignores).  No split-K, no cross-wave or cross-lane sum of a score.  The row norm: lane g of the row's 16 sums
// z_k² for k = g, g + 16, ... ascending in an fmaf chain from 0, then a butterfly over the 16 partial sums (xor 8, 4,
// 2, 1; every lane gets the same bits); the scale is 1 / sqrtf(Σ) when Σ > 0, else 0 (so a NaN sum scales by 0 too
// and the row's NaN elements stay NaN: never selected).  So a pair's bits depend on its two rows, D and the metric
// only: not on n_q, n_cand, the rows' positions, the tile, the chunk or the grid.
//
// The C layout (col = lane & 15: the candidate, row = 4 (lane >> 4) + reg: the query) goes to LDS as [16][chunk + 4]
// (the 4 floats of padding put the four row groups of a store 16 banks apart) and to out_all straight from the
// registers; then a thread per candidate writes NaN over the excluded pairs (excluded_mask), which the select never
// picks.  Queries past n_q and candidates past n_cand read a clamped in-bounds row and are discarded.
// No atomics, no allocation, no host synchronisation: graph-capturable, run-to-run identical.
#include "tgnx_topk_dev.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int KN_GROUP = 16;                       // lanes per row in knn_prep; candidates per MFMA sub-tile
constexpr int KN_PREP_ROWS = TK_BLOCK / KN_GROUP;  // rows per knn_prep workgroup
constexpr int KN_PAD = 4;                          // floats of padding per LDS score row
constexpr int KN_NJMAX = (int)TK_DMAX / 16;        // 16-float k steps of the longest row

// Rows [0, n_q) are z_q's, [n_q, n_q + n_cand) z_cand's.  (A group of 16 lanes shares its row: it leaves together.)
__global__ void __launch_bounds__(TK_BLOCK) knn_prep(int64_t n_q, int64_t n_cand, int D, int ldh, int cosine,
                                                     const float* __restrict__ z_q, const float* __restrict__ z_cand,
                                                     float* __restrict__ wq, float* __restrict__ wc) {
  const int g = threadIdx.x & (KN_GROUP - 1);
  const int64_t r = blockIdx.x * (int64_t)KN_PREP_ROWS + (threadIdx.x / KN_GROUP);
  if (r >= n_q + n_cand) return;
  const bool isq = r < n_q;
  const float* src = isq ? z_q + r * D : z_cand + (r - n_q) * D;
  float* dst = isq ? wq + r * ldh : wc + (r - n_q) * ldh;
  float v[KN_NJMAX];
#pragma unroll
  for (int i = 0; i < KN_NJMAX; ++i) {
    const int kk = g + KN_GROUP * i;
    v[i] = kk < D ? src[kk] : 0.f;
  }
  float scale = 1.f;
  if (cosine) {  // (uniform)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < KN_NJMAX; ++i) s = fmaf(v[i], v[i], s);
#pragma unroll
    for (int o = KN_GROUP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
    scale = s > 0.f ? 1.f / sqrtf(s) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < KN_NJMAX; ++i) {
    const int kk = g + KN_GROUP * i;
    if (kk < ldh) dst[kk] = cosine ? v[i] * scale : v[i];
  }
}

// vector 4 j + h of a prepared row (nv = ldh / 4 vectors): the load stays inside the row, a vector past its end is zero
__device__ __forceinline__ float4 knn_vec(const float4* __restrict__ row, int v, int nv) {
  const float4 t = row[min(v, nv - 1)];
  return v < nv ? t : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int NJ, bool FILT>
__global__ void __launch_bounds__(TK_BLOCK) knn_pairs(int64_t n_q, int64_t n_cand, int ldh, int chunk, int nc,
                                                      const float* __restrict__ zq, const float* __restrict__ zc,
                                                      int k, float* __restrict__ pval, int* __restrict__ pidx,
                                                      float* __restrict__ out_all, TopkFilter f) {
  extern __shared__ __attribute__((aligned(16))) float kn_smem[];
  const int ldl = chunk + KN_PAD;
  float* L = kn_smem;  // [16][ldl] the chunk's scores
  // (ldl is a multiple of 4: the struct starts 16-B aligned)
  TopkFilterLds* X = reinterpret_cast<TopkFilterLds*>(L + (size_t)TK_TQ * ldl);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 15, h = lane >> 4;
  const int64_t tile = blockIdx.x / nc, q0 = tile * TK_TQ;
  const int64_t cj = blockIdx.x % nc, cbase = cj * chunk;
  const int nq = (int)min((int64_t)TK_TQ, n_q - q0);
  const int nvalid = (int)min((int64_t)chunk, n_cand - cbase);
  const int nv = ldh >> 2;
  if constexpr (FILT) stage_filter(X, f, q0, nq, tid);
  // the A operand: a lane past the tile's end reads the last valid query (in bounds, its rows are not stored)
  float4 a[NJ];
  {
    const float4* qrow = reinterpret_cast<const float4*>(zq + (q0 + min(r, nq - 1)) * ldh);
#pragma unroll
    for (int j = 0; j < NJ; ++j) a[j] = knn_vec(qrow, 4 * j + h, nv);
  }
  const int nsw = chunk / (KN_GROUP * (TK_BLOCK / WAVE));  // sub-tiles per wave (4 or 8)
  for (int s0 = 0; s0 < nsw; s0 += 2) {
    const int c0 = (wv * nsw + s0) * KN_GROUP, c1 = c0 + KN_GROUP;
    if (c0 >= nvalid) break;  // (wave-uniform; entries past nvalid are never scanned)
    // a lane past the chunk's end reads the last valid row (in bounds, result discarded)
    const float4* b0r = reinterpret_cast<const float4*>(zc + (cbase + min(c0 + r, nvalid - 1)) * ldh);
    const float4* b1r = reinterpret_cast<const float4*>(zc + (cbase + min(c1 + r, nvalid - 1)) * ldh);
    float4 b0[NJ], b1[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      b0[j] = knn_vec(b0r, 4 * j + h, nv);
      b1[j] = knn_vec(b1r, 4 * j + h, nv);
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b0[j].x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b1[j].x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b0[j].y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b1[j].y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b0[j].z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b1[j].z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b0[j].w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b1[j].w, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = 4 * h + e;  // the query; the candidate is the lane's column r
      L[row * ldl + c0 + r] = acc0[e];
      L[row * ldl + c1 + r] = acc1[e];
      if (out_all && row < nq) {
        float* o = out_all + (q0 + row) * n_cand + cbase;
        if (c0 + r < nvalid) o[c0 + r] = acc0[e];
        if (c1 + r < nvalid) o[c1 + r] = acc1[e];
      }
    }
  }
  __syncthreads();
  // an excluded pair's entry in LDS becomes NaN, which the select never picks; out_all keeps the score
  if constexpr (FILT) {
    for (int cl = tid; cl < nvalid; cl += TK_BLOCK) {
      const int64_t cpos = cbase + cl;
      const unsigned excl = excluded_mask(X, f, nq, f.cand_key ? f.cand_key[cpos] : cpos);
#pragma unroll
      for (int i = 0; i < TK_TQ; ++i)
        if ((excl >> i) & 1u) L[i * ldl + cl] = TK_QNAN;
    }
    __syncthreads();
  }
  // wave w takes queries 4 w .. 4 w + 3 (rows past nq repeat the last query's scores and are not stored)
  constexpr int QW = TK_TQ / (TK_BLOCK / WAVE);
  const int i0 = wv * QW;
  select_chunk<QW>(L + i0 * ldl, ldl, nvalid, k, lane, q0 + i0, nq - i0, nc, cj, (int)cbase, pval, pidx);
}

size_t knn_smem(int chunk, bool filt) {
  return (size_t)TK_TQ * (chunk + KN_PAD) * sizeof(float) + (filt ? sizeof(TopkFilterLds) : 0);
}

template <int NJ>
void launch_pairs(hipStream_t s, bool filt, int64_t blocks, int64_t n_q, int64_t n_cand, int ldh, int chunk, int nc,
                  const TopkWs& w, int k, float* out_all, const TopkFilter& f) {
  if (filt)
    hipLaunchKernelGGL((knn_pairs<NJ, true>), dim3((unsigned)blocks), dim3(TK_BLOCK), knn_smem(chunk, true), s, n_q,
                       n_cand, ldh, chunk, nc, (const float*)w.hs, (const float*)w.hd, k, w.pval, w.pidx, out_all, f);
  else
    hipLaunchKernelGGL((knn_pairs<NJ, false>), dim3((unsigned)blocks), dim3(TK_BLOCK), knn_smem(chunk, false), s, n_q,
                       n_cand, ldh, chunk, nc, (const float*)w.hs, (const float*)w.hd, k, w.pval, w.pidx, out_all,
                       TopkFilter{});
}

}  // namespace

extern "C" {

size_t tgnx_embed_knn_ws_bytes(int64_t n_q, int64_t n_cand, int64_t D, int32_t k) {
  if (n_q < 0 || n_cand < 0 || D <= 0 || D > TK_DMAX || k < 1 || k > TGNX_TOPK_MAX) return 256;
  return carve_ws(nullptr, n_q, n_cand, D, k, dense_lists(n_cand)).used + 256;
}

int tgnx_embed_knn(int64_t n_q, int64_t n_cand, int64_t D, const float* z_q, const float* z_cand, int32_t metric,
                   int32_t k, const int64_t* cand_key, const int64_t* q_key, const int64_t* excl_ptr,
                   const int64_t* excl_key, int64_t nnz, float* out_val, int64_t* out_idx, float* out_all, void* ws,
                   size_t ws_bytes, void* stream) {
  const char* name = "tgnx_embed_knn";
  TGNX_CHECK_ARG(k >= 1 && k <= TGNX_TOPK_MAX, "%s: k must be in [1, %d], got %d", name, TGNX_TOPK_MAX, k);
  TGNX_CHECK_ARG(metric == TGNX_KNN_DOT || metric == TGNX_KNN_COSINE, "%s: unknown metric %d", name, metric);
  TGNX_CHECK_ARG(n_q >= 0 && n_cand >= 0 && D >= 1 && D <= TK_DMAX && n_cand < (int64_t(1) << 31) - TK_CHUNK_MAX &&
                     n_q < (int64_t(1) << 31),
                 "%s: bad sizes (n_q, n_cand >= 0, 1 <= D <= %d)", name, (int)TK_DMAX);
  TGNX_CHECK_ARG(ws && (n_cand == 0 || z_cand) && (n_q == 0 || (z_q && out_val && out_idx)), "%s: null pointer", name);
  TGNX_CHECK_ARG(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "%s: the workspace must be 16-byte aligned", name);
  TGNX_CHECK_ARG(nnz >= 0 && (!excl_ptr || nnz == 0 || excl_key), "%s: excl_ptr needs excl_key and nnz >= 0", name);
  TGNX_CHECK_ARG(ws_bytes >= tgnx_embed_knn_ws_bytes(n_q, n_cand, D, k), "%s: workspace too small", name);
  if (n_q == 0) return TGNX_OK;
  hipStream_t s = as_stream(stream);
  const TopkWs w = carve_ws(ws, n_q, n_cand, D, k, dense_lists(n_cand));
  const int64_t ldh = ld_of(D);
  const int chunk = chunk_of(n_q, n_cand);
  const int64_t nc = ceil_div(n_cand, chunk), blocks = ceil_div(n_q, TK_TQ) * nc;
  TGNX_CHECK_ARG(blocks < (int64_t(1) << 31), "%s: n_q x n_cand beyond one launch's grid", name);
  if (n_cand > 0) {  // (n_cand = 0: no chunk, every slot is padding)
    hipLaunchKernelGGL(knn_prep, dim3((unsigned)ceil_div(n_q + n_cand, KN_PREP_ROWS)), dim3(TK_BLOCK), 0, s, n_q,
                       n_cand, (int)D, (int)ldh, (int)(metric == TGNX_KNN_COSINE), z_q, z_cand, w.hs, w.hd);
    TGNX_LAUNCH_CHECK("knn_prep");
    const TopkFilter f{cand_key, q_key, excl_ptr, excl_key, nnz};
    const bool filt = q_key || excl_ptr;  // (cand_key alone excludes nothing)
#define KNN_CASE(NJ)                                                                                           \
  case NJ:                                                                                                     \
    launch_pairs<NJ>(s, filt, blocks, n_q, n_cand, (int)ldh, chunk, (int)nc, w, (int)k, out_all, f);           \
    break;
    switch ((int)ceil_div(ldh, 16)) {
      KNN_CASE(1) KNN_CASE(2) KNN_CASE(3) KNN_CASE(4) KNN_CASE(5) KNN_CASE(6) KNN_CASE(7) KNN_CASE(8)
      KNN_CASE(9) KNN_CASE(10) KNN_CASE(11) KNN_CASE(12) KNN_CASE(13) KNN_CASE(14) KNN_CASE(15) KNN_CASE(16)
    }
#undef KNN_CASE
    TGNX_LAUNCH_CHECK("knn_pairs");
  }
  return launch_merge(s, n_q, nc, k, w, 0, out_val, out_idx);
}

}  // extern "C"
