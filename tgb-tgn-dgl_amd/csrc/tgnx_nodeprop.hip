// Node property prediction (TGB's tgbn-* task): NodePredictor (modules/decoder.py:30-41), its soft-target
// cross-entropy and NDCG@k.
//
//   tgnx_node_predictor       logits = W2 relu(W1 z + b1) + b2: two launches of the f32 MFMA GEMM core (tgnx_gemm.h),
//                             bias + ReLU and bias in the epilogues
//   tgnx_node_predictor_bwd   dh = (dlogits W2) (h > 0) on the core with the mask in the epilogue (split-K over the
//                             classes + fixup when C > 256); the plain contractions on tgnx_gemm_f32, the bias
//                             gradients on tgnx_col_sum
//   tgnx_node_loss_ndcg       the row kernel: a wave per row of logits stages the row and its targets in LDS once and
//                             gives the row's loss, dlogits and NDCG@k
//
// Determinism: no float atomics.  A row belongs to one wave whatever the grid; its f32 sums run lane-strided over the
// 64-class chunks in increasing order and then across the wave (wave_sum_f / wave_max_f: DPP + permlane swaps), its
// float64 DCG / IDCG terms are added in class order by every lane alike.
#include <math.h>

#include <algorithm>

#include "tgnx_gemm.h"

using namespace tgnx;

namespace {

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// ------------------------------------------------------------------ the head's GEMMs
// C[m, n] = relu(v + bias[n])
struct EpiBiasRelu {
  float* C;
  const float* bias;
  int ldc;
  template <class T>
  __device__ void operator()(const T& t) const {
#pragma unroll
    for (int i = 0; i < T::per; ++i) {
      const int r = T::row_of(i), cc = T::col_of(i), m = t.m0 + r, n = t.n0 + cc;
      if (m < t.M && n < t.N) C[(int64_t)m * ldc + n] = fmaxf(t(r, cc) + (bias ? bias[n] : 0.f), 0.f);
    }
  }
};
// C[m, n] = v [gate[m, n] > 0]   (the ReLU's backward; gate = the hidden rows)
struct EpiReluMask {
  float* C;
  const float* gate;
  int ldc;
  template <class T>
  __device__ void operator()(const T& t) const {
    float g[T::per];
#pragma unroll
    for (int i = 0; i < T::per; ++i) {
      const int m = min(t.m0 + T::row_of(i), t.M - 1), n = min(t.n0 + T::col_of(i), t.N - 1);
      g[i] = gate[(int64_t)m * ldc + n];
    }
#pragma unroll
    for (int i = 0; i < T::per; ++i) {
      const int r = T::row_of(i), cc = T::col_of(i), m = t.m0 + r, n = t.n0 + cc;
      if (m < t.M && n < t.N) C[(int64_t)m * ldc + n] = g[i] > 0.f ? t(r, cc) : 0.f;
    }
  }
};

// a GEMM with one of the epilogues above, shaped as tgnx_gemm_f32 shapes its own (gemm_api_big / gemm_api_shape; the
// partials of a split K take tgnx_gemm_f32_ws_bytes(M, N, K) bytes)
template <class AL, class BL, class EPI>
void head_gemm(int64_t M, int64_t N, int64_t K, const AL& al, const BL& bl, const EPI& epi, float* part, hipStream_t s) {
  auto run = [&](auto cfg) {
    using CFG = decltype(cfg);
    const GemmShape g = gemm_api_shape<CFG>(M, N, K);
    gemm_launch<CFG>(g, al, bl, epi, part, s);
    if (g.deferred) gemm_fixup_launch(0, NoTail{}, s, gemm_fix<CFG>(g, part, epi));
  };
  if (gemm_api_big(M, N)) run(G64{});
  else run(GD{});
}

// ------------------------------------------------------------------ the row kernel
// W waves per workgroup, a row per wave; LDS: per wave the row's logits and targets, each padded to whole 64-class
// chunks (pad: logit -inf, target 0).  The wave never meets a workgroup barrier, so a wave past the rows just leaves.
template <int W>
__global__ void __launch_bounds__(W* WAVE) node_rows(int64_t M, int C, int k, const float* __restrict__ logits,
                                                     const float* __restrict__ y, const double* __restrict__ cum,
                                                     float scale, float* __restrict__ loss, float* __restrict__ dlogits,
                                                     double* __restrict__ ndcg) {
  extern __shared__ __attribute__((aligned(16))) float node_lds[];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * (int64_t)W + wv;
  if (row >= M) return;
  const int nch = (C + WAVE - 1) / WAVE, Cp = nch * WAVE;
  float* ls = node_lds + (size_t)wv * 2 * Cp;
  float* ys = ls + Cp;
  const float* lr = logits + row * C;
  const float* yr = y + row * C;
  float mx = -INFINITY;
  for (int j = 0; j < nch; ++j) {
    const int c = j * WAVE + lane;
    const bool in = c < C;
    const float l = in ? lr[c] : -INFINITY, t = in ? yr[c] : 0.f;
    ls[c] = l;
    ys[c] = t;
    mx = fmaxf(mx, l);
  }
  mx = wave_max_f(mx);
  float se = 0.f, sy = 0.f, syl = 0.f;
  for (int j = 0; j < nch; ++j) {  // lane-strided partial sums, chunks in increasing order
    const int c = j * WAVE + lane;
    const float l = ls[c], t = ys[c];
    se += expf(l - mx);  // (pad: exp(-inf) = 0)
    sy += t;
    syl += c < C ? t * l : 0.f;
  }
  se = wave_sum_f(se);
  sy = wave_sum_f(sy);
  syl = wave_sum_f(syl);
  const float lse = mx + logf(se);
  if (loss && lane == 0) loss[row] = lse * sy - syl;
  if (dlogits) {
    float* dr = dlogits + row * C;
    for (int j = 0; j < nch; ++j) {
      const int c = j * WAVE + lane;
      if (c < C) dr[c] = (expf(ls[c] - lse) * sy - ys[c]) * scale;
    }
  }
  if (!ndcg) return;
  // every lane of the wave has written its LDS entries above; the counts below read the whole row
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double dcg = 0.0, idcg = 0.0;
  for (int j = 0; j < nch; ++j) {  // classes with a positive target, in class order
    const float lj = ls[j * WAVE + lane], yj = ys[j * WAVE + lane];
    unsigned long long todo = __ballot(yj > 0.f);
    while (todo) {  // (wave-uniform)
      const int b = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
      todo &= todo - 1;
      const float lc = lane_f(lj, b), yc = lane_f(yj, b);
      int gt = 0, eq = 0, gty = 0, eqy = 0;  // exact counts: ballots, no float sums
      for (int i = 0; i < nch; ++i) {
        const int c = i * WAVE + lane;
        const bool in = c < C;
        const float li = ls[c], yi = ys[c];
        gt += __popcll(__ballot(in && li > lc));
        eq += __popcll(__ballot(in && li == lc));
        gty += __popcll(__ballot(yi > yc));
        eqy += __popcll(__ballot(yi == yc));
      }
      // the class shares ranks gt + 1 .. gt + eq with its ties: the mean of their discounts (0 beyond rank k)
      dcg += (double)yc * (cum[min(gt + eq, k)] - cum[min(gt, k)]) / (double)max(eq, 1);
      idcg += (double)yc * (cum[min(gty + eqy, k)] - cum[min(gty, k)]) / (double)max(eqy, 1);
    }
  }
  if (lane == 0) ndcg[row] = idcg > 0.0 ? dcg / idcg : 0.0;
}

// out[0] = scale Σ_i x[i]: thread t adds rows t, t + 256, ... in order, then the wave, then the four waves in order
__global__ void __launch_bounds__(256) rows_mean(int64_t M, const float* __restrict__ x, float scale,
                                                 float* __restrict__ out) {
  __shared__ float part[4];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < M; i += 256) s += x[i];
  s = wave_sum_f(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (((part[0] + part[1]) + part[2]) + part[3]) * scale;
}

bool node_dims_ok(int64_t M, int64_t D, int64_t C) {
  return M >= 0 && M < (int64_t(1) << 24) && D >= 1 && D <= TGNX_NODE_MAX_D && C >= 1 && C <= TGNX_NODE_MAX_C;
}

}  // namespace

extern "C" {

size_t tgnx_node_predictor_ws_bytes(int64_t M, int64_t D, int64_t C) {
  if (!node_dims_ok(M, D, C) || M == 0) return 256;
  return align256((size_t)M * D * 4) + std::max(tgnx_gemm_f32_ws_bytes(M, D, D), tgnx_gemm_f32_ws_bytes(M, C, D));
}

int tgnx_node_predictor(int64_t M, int64_t D, int64_t C, const float* z, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* logits, float* h, void* ws, size_t ws_bytes,
                        void* stream) {
  TGNX_CHECK_ARG(node_dims_ok(M, D, C),
                 "tgnx_node_predictor: bad sizes (0 <= M < 2^24, 1 <= D <= %d, 1 <= C <= %d; got M %lld D %lld C %lld)",
                 TGNX_NODE_MAX_D, TGNX_NODE_MAX_C, (long long)M, (long long)D, (long long)C);
  if (M == 0) return TGNX_OK;
  TGNX_CHECK_ARG(z && w1 && w2 && logits && ws, "tgnx_node_predictor: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_node_predictor_ws_bytes(M, D, C), "tgnx_node_predictor: workspace too small");
  hipStream_t s = as_stream(stream);
  char* p = reinterpret_cast<char*>(ws);
  float* hid = h ? h : reinterpret_cast<float*>(p);
  float* part = reinterpret_cast<float*>(p + align256((size_t)M * D * 4));
  const int Mi = (int)M, Di = (int)D, Ci = (int)C;
  head_gemm(M, D, D, LoadRowK{z, Mi, Di, Di}, LoadRowK{w1, Di, Di, Di}, EpiBiasRelu{hid, b1, Di}, part, s);
  TGNX_LAUNCH_CHECK("tgnx_node_predictor (hidden)");
  head_gemm(M, C, D, LoadRowK{hid, Mi, Di, Di}, LoadRowK{w2, Ci, Di, Di}, EpiStore{logits, b2, Ci, 0}, part, s);
  TGNX_LAUNCH_CHECK("tgnx_node_predictor (out)");
  return TGNX_OK;
}

size_t tgnx_node_predictor_bwd_ws_bytes(int64_t M, int64_t D, int64_t C) {
  if (!node_dims_ok(M, D, C) || M == 0) return 256;
  size_t g = tgnx_gemm_f32_ws_bytes(M, D, C);
  g = std::max(g, std::max(tgnx_gemm_f32_ws_bytes(C, D, M), tgnx_gemm_f32_ws_bytes(D, D, M)));
  g = std::max(g, tgnx_gemm_f32_ws_bytes(M, D, D));
  return align256((size_t)M * D * 4) + align256(g) +
         std::max(tgnx_col_sum_ws_bytes(M, C), tgnx_col_sum_ws_bytes(M, D));
}

int tgnx_node_predictor_bwd(int64_t M, int64_t D, int64_t C, const float* dlogits, const float* z, const float* h,
                            const float* w1, const float* w2, float* dz, float* dw1, float* db1, float* dw2,
                            float* db2, void* ws, size_t ws_bytes, void* stream) {
  TGNX_CHECK_ARG(node_dims_ok(M, D, C),
                 "tgnx_node_predictor_bwd: bad sizes (0 <= M < 2^24, 1 <= D <= %d, 1 <= C <= %d; got M %lld D %lld C "
                 "%lld)",
                 TGNX_NODE_MAX_D, TGNX_NODE_MAX_C, (long long)M, (long long)D, (long long)C);
  hipStream_t s = as_stream(stream);
  if (M == 0) {  // no rows: the parameter gradients are zero
    if (dw1) TGNX_HIP_CHECK(hipMemsetAsync(dw1, 0, D * D * 4, s));
    if (db1) TGNX_HIP_CHECK(hipMemsetAsync(db1, 0, D * 4, s));
    if (dw2) TGNX_HIP_CHECK(hipMemsetAsync(dw2, 0, C * D * 4, s));
    if (db2) TGNX_HIP_CHECK(hipMemsetAsync(db2, 0, C * 4, s));
    return TGNX_OK;
  }
  TGNX_CHECK_ARG(dlogits && z && h && w1 && w2 && ws, "tgnx_node_predictor_bwd: null pointer");
  TGNX_CHECK_ARG(ws_bytes >= tgnx_node_predictor_bwd_ws_bytes(M, D, C), "tgnx_node_predictor_bwd: workspace too small");
  char* p = reinterpret_cast<char*>(ws);
  const size_t hb = align256((size_t)M * D * 4);
  const size_t gb = ws_bytes - hb - std::max(tgnx_col_sum_ws_bytes(M, C), tgnx_col_sum_ws_bytes(M, D));
  float* dh = reinterpret_cast<float*>(p);
  void* gws = p + hb;
  void* cws = p + hb + gb;
  const size_t cb = ws_bytes - hb - gb;
  int rc;
  if (dw2) {  // dW2 = dlogits^T h
    rc = tgnx_gemm_f32(C, D, M, dlogits, C, 1, h, D, 0, dw2, D, nullptr, 0, gws, gb, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (db2) {
    rc = tgnx_col_sum(M, C, dlogits, C, db2, cws, cb, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (!(dz || dw1 || db1)) return TGNX_OK;
  // dh = (dlogits W2) [h > 0]: B element (k = class, n) = w2[k * D + n]
  const int Mi = (int)M, Di = (int)D, Ci = (int)C;
  head_gemm(M, D, C, LoadRowK{dlogits, Mi, Ci, Ci}, LoadKRow{w2, Di, Ci, Di}, EpiReluMask{dh, h, Di},
            reinterpret_cast<float*>(gws), s);
  TGNX_LAUNCH_CHECK("tgnx_node_predictor_bwd (dh)");
  if (dw1) {  // dW1 = dh^T z
    rc = tgnx_gemm_f32(D, D, M, dh, D, 1, z, D, 0, dw1, D, nullptr, 0, gws, gb, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (db1) {
    rc = tgnx_col_sum(M, D, dh, D, db1, cws, cb, stream);
    if (rc != TGNX_OK) return rc;
  }
  if (dz) {  // dz = dh W1
    rc = tgnx_gemm_f32(M, D, D, dh, D, 0, w1, D, 0, dz, D, nullptr, 0, gws, gb, stream);
    if (rc != TGNX_OK) return rc;
  }
  return TGNX_OK;
}

int tgnx_node_loss_ndcg(int64_t M, int64_t C, int32_t k, const float* logits, const float* y, const double* cum,
                        float scale, float* loss_rows, float* loss_mean, float* dlogits, double* ndcg, void* stream) {
  TGNX_CHECK_ARG(M >= 0 && M < (int64_t(1) << 31) && C >= 1 && C <= TGNX_NODE_MAX_C,
                 "tgnx_node_loss_ndcg: bad sizes (0 <= M < 2^31, 1 <= C <= %d; got M %lld C %lld)", TGNX_NODE_MAX_C,
                 (long long)M, (long long)C);
  TGNX_CHECK_ARG(k >= 1 && k <= TGNX_NODE_MAX_K, "tgnx_node_loss_ndcg: k must be in [1, %d], got %d", TGNX_NODE_MAX_K,
                 (int)k);
  TGNX_CHECK_ARG(!loss_mean || loss_rows, "tgnx_node_loss_ndcg: loss_mean needs loss_rows");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    if (loss_mean) TGNX_HIP_CHECK(hipMemsetAsync(loss_mean, 0, 4, s));
    return TGNX_OK;
  }
  TGNX_CHECK_ARG(logits && y && (!ndcg || cum), "tgnx_node_loss_ndcg: null pointer");
  const int Cp = (int)((C + WAVE - 1) / WAVE) * WAVE;
  // LDS: 8 Cp bytes per wave; four waves up to 2,048 classes (<= 64 KB), two beyond
  if (Cp <= 2048) {
    constexpr int W = 4;
    hipLaunchKernelGGL(node_rows<W>, dim3((unsigned)((M + W - 1) / W)), dim3(W * WAVE), (size_t)W * 2 * Cp * 4, s, M,
                       (int)C, (int)k, logits, y, cum, scale, loss_rows, dlogits, ndcg);
  } else {
    constexpr int W = 2;
    hipLaunchKernelGGL(node_rows<W>, dim3((unsigned)((M + W - 1) / W)), dim3(W * WAVE), (size_t)W * 2 * Cp * 4, s, M,
                       (int)C, (int)k, logits, y, cum, scale, loss_rows, dlogits, ndcg);
  }
  TGNX_LAUNCH_CHECK("node_rows");
  if (loss_mean) {
    hipLaunchKernelGGL(rows_mean, dim3(1), dim3(256), 0, s, M, (const float*)loss_rows, scale, loss_mean);
    TGNX_LAUNCH_CHECK("rows_mean");
  }
  return TGNX_OK;
}

}  // extern "C"
