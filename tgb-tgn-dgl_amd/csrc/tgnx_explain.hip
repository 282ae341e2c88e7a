// Leave-one-out link logits (tgnx_link_predictor_loo; torch.ops.tgnx.predictor_loo): the
// LinkPredictor logit of P pairs, and the same logit with one side's embedding replaced by each of its K
// leave-one-out rows (tgnx_tgn_explain's loo_z) while the other side keeps its full embedding:
//   logit(a, b) = w_out · relu(W_src a + b_src + W_dst b + b_dst) + b_out                     (decoder.py:12-27)
//   base[p]         = logit(z[s], z[d])                  s = src_row[p], d = dst_row[p]
//   src_logit[p][j] = logit(loo_z[s][j], z[d])           j < count[s], else base[p]'s bits
//   dst_logit[p][j] = logit(z[s], loo_z[d][j])           j < count[d], else base[p]'s bits
// z [n, d_in] and loo_z [n, K, d_in] hold one row (K rows) per UNIQUE node; the pairs index into them.
//
//   Hs = z W_src^T + b_src, Hd = z W_dst^T + b_dst [n, ldh], HsL = loo_z W_src^T + b_src, HdL = loo_z W_dst^T + b_dst
//   [n K, ldh] on the MFMA GEMM (ldh = D rounded up to 4 floats): every unique row is projected once, O(n K D^2),
//   whatever the number of pairs that name it (one source explained against k recommended destinations: k pairs, the
//   source's K + 1 rows projected once);
//   loo_rows   a thread per (pair, chain): the 1 + 2 K relu-dot chains of a pair, each one sequential fma chain over
//              the D columns in ascending order (tgnx_topk.hip's pair_chain order), so a logit's bits depend on its
//              two rows alone — not on the grid, nor on where the pair stands in the list.  A chain past the varied
//              node's count runs over the base rows: the base logit's bits.
// A row index outside [0, n) is never dereferenced: the pair's 1 + 2 K outputs are NaN and *status becomes 1 (a plain
// idempotent store).  No atomics, no allocation, no host synchronisation.
#include <math.h>

#include <algorithm>

#include "tgnx_common.h"

namespace tgnx {
void probe_begin(int id, hipStream_t s);
void probe_end(int id, hipStream_t s);
}  // namespace tgnx

using namespace tgnx;

namespace {

constexpr int64_t LOO_DMAX = 256;   // D of the projected rows (as the top-k operators)
constexpr int LOO_BLOCK = 256;
constexpr float LOO_QNAN = __builtin_bit_cast(float, 0x7fc00000);

int64_t ld_of(int64_t D) { return (D + 3) & ~int64_t(3); }
size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

struct LooWs {
  float *hs, *hd, *hsl, *hdl;
  char* gemm;
  size_t used;
};
LooWs carve_ws(void* ws, int64_t n, int64_t K, int64_t D) {
  const int64_t ldh = ld_of(D);
  char* p = reinterpret_cast<char*>(ws);
  size_t off = 0;
  LooWs w;
  auto take = [&](int64_t rows) {
    float* q = reinterpret_cast<float*>(p + off);
    off += align256((size_t)rows * ldh * sizeof(float));
    return q;
  };
  w.hs = take(n);
  w.hd = take(n);
  w.hsl = take(n * K);
  w.hdl = take(n * K);
  w.gemm = p + off;
  w.used = off;
  return w;
}

// the chain that fixes a logit's bits: acc = fma(w_k, relu(a_k + b_k), acc) for k = 0 .. D - 1, + b_out
__device__ __forceinline__ float loo_chain(const float* __restrict__ a, const float* __restrict__ b,
                                           const float* __restrict__ w_out, int D, int ldh, float b_out) {
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float acc = 0.f;
  for (int v = 0; v < ldh / 4; ++v) {  // (rows start 16-B aligned: ldh % 4 == 0; the pad columns are not read as values)
    const float4 x = a4[v], y = b4[v];
    const float xe[4] = {x.x, x.y, x.z, x.w}, ye[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = 4 * v + e;
      if (kk < D) acc = fmaf(w_out[kk], fmaxf(xe[e] + ye[e], 0.f), acc);
    }
  }
  return acc + b_out;
}

// thread t: pair p = t / (1 + 2 K), chain c = t % (1 + 2 K): 0 the base, 1 .. K the source's row c - 1 varied,
// K + 1 .. 2 K the destination's
__global__ void __launch_bounds__(LOO_BLOCK) loo_rows(int64_t n, int K, int64_t P, int D, int ldh,
                                                      const int32_t* __restrict__ count,
                                                      const int64_t* __restrict__ src_row,
                                                      const int64_t* __restrict__ dst_row,
                                                      const float* __restrict__ hs, const float* __restrict__ hd,
                                                      const float* __restrict__ hsl, const float* __restrict__ hdl,
                                                      const float* __restrict__ w_out,
                                                      const float* __restrict__ b_out, float* __restrict__ base,
                                                      float* __restrict__ src_logit, float* __restrict__ dst_logit,
                                                      int64_t* __restrict__ status) {
  const int nch = 1 + 2 * K;
  const int64_t t = blockIdx.x * (int64_t)LOO_BLOCK + threadIdx.x;
  if (t >= P * nch) return;
  const int64_t p = t / nch;
  const int ch = (int)(t - p * nch);
  const int64_t s = src_row[p], d = dst_row[p];
  float lg = LOO_QNAN;
  if (s >= 0 && s < n && d >= 0 && d < n) {
    const float* a = hs + s * ldh;
    const float* b = hd + d * ldh;
    if (ch >= 1 && ch <= K) {
      const int j = ch - 1;
      if (j < min(max(count[s], 0), K)) a = hsl + (s * K + j) * ldh;
    } else if (ch > K) {
      const int j = ch - 1 - K;
      if (j < min(max(count[d], 0), K)) b = hdl + (d * K + j) * ldh;
    }
    lg = loo_chain(a, b, w_out, D, ldh, b_out[0]);
  } else if (ch == 0) {
    *status = 1;
  }
  if (ch == 0) base[p] = lg;
  else if (ch <= K) src_logit[p * K + (ch - 1)] = lg;
  else dst_logit[p * K + (ch - 1 - K)] = lg;
}

bool sizes_ok(int64_t n, int64_t K, int64_t P, int64_t d_in, int64_t D) {
  return n >= 0 && K >= 1 && K <= 64 && P >= 0 && d_in >= 1 && d_in < (1 << 30) && D >= 1 && D <= LOO_DMAX &&
         n < (int64_t(1) << 24) && P < (int64_t(1) << 24);
}

size_t gemm_bytes(int64_t n, int64_t K, int64_t d_in, int64_t D) {
  return n > 0 ? std::max(tgnx_gemm_f32_ws_bytes(n, D, d_in), tgnx_gemm_f32_ws_bytes(n * K, D, d_in)) : 0;
}

}  // namespace

extern "C" {

size_t tgnx_link_predictor_loo_ws_bytes(int64_t n, int64_t K, int64_t P, int64_t d_in, int64_t D) {
  if (!sizes_ok(n, K, P, d_in, D)) return 256;
  return carve_ws(nullptr, n, K, D).used + align256(gemm_bytes(n, K, d_in, D)) + 256;
}

int tgnx_link_predictor_loo(int64_t n, int64_t K, int64_t P, int64_t d_in, int64_t D, const float* z,
                            const float* loo_z, const int32_t* count, const int64_t* src_row, const int64_t* dst_row,
                            const float* w_src, const float* b_src, const float* w_dst, const float* b_dst,
                            const float* w_out, const float* b_out, float* base, float* src_logit, float* dst_logit,
                            int64_t* status, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "tgnx_link_predictor_loo";
  TGNX_CHECK_ARG(sizes_ok(n, K, P, d_in, D),
                 "%s: bad sizes (0 <= n, P < 2^24, 1 <= K <= 64, d_in >= 1, 1 <= D <= %d)", who, (int)LOO_DMAX);
  TGNX_CHECK_ARG(w_src && w_dst && w_out && b_out && ws && status, "%s: null pointer", who);
  TGNX_CHECK_ARG(n == 0 || (z && loo_z && count), "%s: null pointer", who);
  TGNX_CHECK_ARG(P == 0 || (src_row && dst_row && base && src_logit && dst_logit), "%s: null pointer", who);
  TGNX_CHECK_ARG(ws_bytes >= tgnx_link_predictor_loo_ws_bytes(n, K, P, d_in, D), "%s: workspace too small", who);
  if (P == 0) return TGNX_OK;
  hipStream_t s = as_stream(stream);
  const LooWs w = carve_ws(ws, n, K, D);
  const int64_t ldh = ld_of(D);
  const size_t gb = ws_bytes - w.used;
  if (n > 0) {
    const struct { const float* a; int64_t rows; const float* wt; const float* bias; float* out; } jobs[4] = {
        {z, n, w_src, b_src, w.hs}, {z, n, w_dst, b_dst, w.hd},
        {loo_z, n * K, w_src, b_src, w.hsl}, {loo_z, n * K, w_dst, b_dst, w.hdl}};
    for (const auto& j : jobs) {
      const int rc = tgnx_gemm_f32(j.rows, D, d_in, j.a, d_in, 0, j.wt, d_in, 1, j.out, ldh, j.bias, 0, w.gemm, gb, stream);
      if (rc != TGNX_OK) return rc;
    }
  }
  const int64_t threads = P * (1 + 2 * K);
  probe_begin(TGNX_K_LOO_ROWS, s);
  launch_k(loo_rows, dim3((unsigned)((threads + LOO_BLOCK - 1) / LOO_BLOCK)), dim3(LOO_BLOCK), 0u, s, n, (int)K, P,
           (int)D, (int)ldh, count, src_row, dst_row, (const float*)w.hs, (const float*)w.hd, (const float*)w.hsl,
           (const float*)w.hdl, w_out, b_out, base, src_logit, dst_logit, status);
  probe_end(TGNX_K_LOO_ROWS, s);
  TGNX_LAUNCH_CHECK("loo_rows");
  return TGNX_OK;
}

}  // extern "C"
